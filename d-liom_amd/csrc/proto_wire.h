// The proto3 wire format as far as the library's messages need it (grid_proto.cc, compressed_cloud.hip): varints, packed
// repeated scalars, sub-messages, doubles with implicit presence, and skipping what a parser does not know.
#ifndef DLIOM_CSRC_PROTO_WIRE_H_
#define DLIOM_CSRC_PROTO_WIRE_H_

#include <cstdint>
#include <cstring>
#include <vector>

namespace dliom {
namespace wire {

inline void put_varint(std::vector<uint8_t>* out, uint64_t v) {
  while (v >= 0x80) {
    out->push_back(static_cast<uint8_t>(v) | 0x80);
    v >>= 7;
  }
  out->push_back(static_cast<uint8_t>(v));
}
inline int varint_size(uint64_t v) {
  int n = 1;
  while (v >= 0x80) {
    v >>= 7;
    ++n;
  }
  return n;
}

inline void put_packed(std::vector<uint8_t>* out, int field, const std::vector<uint8_t>& payload) {
  if (payload.empty()) return;  // proto3: empty repeated fields are not emitted
  put_varint(out, static_cast<uint64_t>(field) << 3 | 2);
  put_varint(out, payload.size());
  out->insert(out->end(), payload.begin(), payload.end());
}

inline bool get_varint(const uint8_t*& p, const uint8_t* end, uint64_t* v) {
  *v = 0;
  for (int shift = 0; shift < 64 && p < end; shift += 7) {
    const uint8_t b = *p++;
    *v |= static_cast<uint64_t>(b & 0x7F) << shift;
    if ((b & 0x80) == 0) return true;
  }
  return false;
}

inline void put_double_field(std::vector<uint8_t>* out, int field, double v) {
  if (v == 0.0) return;  // proto3 implicit presence, as the C++ runtime decides it (x != 0)
  put_varint(out, static_cast<uint64_t>(field) << 3 | 1);
  uint64_t bits;
  std::memcpy(&bits, &v, 8);
  for (int i = 0; i < 8; ++i) out->push_back(static_cast<uint8_t>(bits >> (8 * i)));
}
inline void put_float_field(std::vector<uint8_t>* out, int field, float v) {
  if (v == 0.f) return;  // the same rule in float: -0.0 is dropped, NaN is written
  put_varint(out, static_cast<uint64_t>(field) << 3 | 5);
  uint32_t bits;
  std::memcpy(&bits, &v, 4);
  for (int i = 0; i < 4; ++i) out->push_back(static_cast<uint8_t>(bits >> (8 * i)));
}
inline void put_message(std::vector<uint8_t>* out, int field, const std::vector<uint8_t>& payload) {
  put_varint(out, static_cast<uint64_t>(field) << 3 | 2);  // a present sub-message is emitted even when empty
  put_varint(out, payload.size());
  out->insert(out->end(), payload.begin(), payload.end());
}
inline void put_bytes(std::vector<uint8_t>* out, int field, const uint8_t* p, int64_t n) {
  put_varint(out, static_cast<uint64_t>(field) << 3 | 2);
  put_varint(out, static_cast<uint64_t>(n));
  out->insert(out->end(), p, p + n);
}
inline bool skip_field(const uint8_t*& p, const uint8_t* end, unsigned wire) {
  uint64_t v;
  switch (wire) {
    case 0: return get_varint(p, end, &v);
    case 1: if (end - p < 8) return false; p += 8; return true;
    case 2: if (!get_varint(p, end, &v) || static_cast<uint64_t>(end - p) < v) return false; p += v; return true;
    case 5: if (end - p < 4) return false; p += 4; return true;
    default: return false;
  }
}
// doubles of a Vector3d / Quaterniond message into dst[field - 1]
inline bool parse_doubles(const uint8_t* p, const uint8_t* end, double* dst, int max_field) {
  while (p < end) {
    uint64_t tag;
    if (!get_varint(p, end, &tag)) return false;
    const unsigned wire = static_cast<unsigned>(tag & 7), field = static_cast<unsigned>(tag >> 3);
    if (wire == 1 && field >= 1 && field <= static_cast<unsigned>(max_field)) {
      if (end - p < 8) return false;
      uint64_t bits = 0;
      for (int i = 0; i < 8; ++i) bits |= static_cast<uint64_t>(p[i]) << (8 * i);
      std::memcpy(&dst[field - 1], &bits, 8);
      p += 8;
    } else if (!skip_field(p, end, wire)) {
      return false;
    }
  }
  return true;
}

// transform::proto::Rigid3d of (x, y, z, qw, qx, qy, qz): transform::ToProto(Rigid3d) sets both sub-messages
inline void put_rigid3d(std::vector<uint8_t>* out, int field, const double pose7[7]) {
  std::vector<uint8_t> translation, rotation, pose;
  for (int i = 0; i < 3; ++i) put_double_field(&translation, i + 1, pose7[i]);  // Vector3d x, y, z
  put_double_field(&rotation, 1, pose7[4]);                                      // Quaterniond x, y, z, w
  put_double_field(&rotation, 2, pose7[5]);
  put_double_field(&rotation, 3, pose7[6]);
  put_double_field(&rotation, 4, pose7[3]);
  put_message(&pose, 1, translation);
  put_message(&pose, 2, rotation);
  put_message(out, field, pose);
}
// transform::proto::Vector3f of (x, y, z): 0 to 15 payload bytes, always emitted (every caller has set the sub-message)
inline void put_vector3f(std::vector<uint8_t>* out, int field, const float xyz[3]) {
  std::vector<uint8_t> payload;
  for (int i = 0; i < 3; ++i) put_float_field(&payload, i + 1, xyz[i]);
  put_message(out, field, payload);
}
// floats of a Vector3f message into dst[field - 1]; absent fields keep what dst holds
inline bool parse_floats(const uint8_t* p, const uint8_t* end, float* dst, int max_field) {
  while (p < end) {
    uint64_t tag;
    if (!get_varint(p, end, &tag) || (tag >> 3) == 0) return false;
    const unsigned wire = static_cast<unsigned>(tag & 7);
    const uint64_t field = tag >> 3;
    if (wire == 5 && field >= 1 && field <= static_cast<uint64_t>(max_field)) {
      if (end - p < 4) return false;
      uint32_t bits = 0;
      for (int i = 0; i < 4; ++i) bits |= static_cast<uint32_t>(p[i]) << (8 * i);
      std::memcpy(&dst[field - 1], &bits, 4);
      p += 4;
    } else if (!skip_field(p, end, wire)) {
      return false;
    }
  }
  return true;
}
// ... and back: translation into t (x, y, z), rotation into q (x, y, z, w); absent fields keep what t and q hold
inline bool parse_rigid3d(const uint8_t* r, const uint8_t* rend, double t[3], double q[4]) {
  while (r < rend) {
    uint64_t rtag, rlen;
    if (!get_varint(r, rend, &rtag)) return false;
    if ((rtag & 7) == 2 && ((rtag >> 3) == 1 || (rtag >> 3) == 2)) {
      if (!get_varint(r, rend, &rlen) || static_cast<uint64_t>(rend - r) < rlen) return false;
      const bool ok = (rtag >> 3) == 1 ? parse_doubles(r, r + rlen, t, 3) : parse_doubles(r, r + rlen, q, 4);
      if (!ok) return false;
      r += rlen;
    } else if (!skip_field(r, rend, static_cast<unsigned>(rtag & 7))) {
      return false;
    }
  }
  return true;
}

}  // namespace wire
}  // namespace dliom

#endif  // DLIOM_CSRC_PROTO_WIRE_H_
