// dliom.h "gzip on the device": the statement on one host thread (dliom_gzip_host), and the size bound.  The caller's
// common::FastGzipString for protos too small to be worth a launch; what the kernels of gzip.hip are compared with.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/dliom.h"
#include "gzip_format.h"

namespace dliom {
namespace {

using gz::Bits;

static constexpr gz::CrcTables kCrc = gz::make_crc_tables();

struct BitWriter {
  std::vector<uint8_t>* out;
  uint64_t acc = 0;
  unsigned held = 0;
  void put(uint32_t v, unsigned n) {
    acc |= static_cast<uint64_t>(v) << held;
    held += n;
    while (held >= 8) {
      out->push_back(static_cast<uint8_t>(acc));
      acc >>= 8;
      held -= 8;
    }
  }
  void to_byte() {
    if (held > 0) {
      out->push_back(static_cast<uint8_t>(acc));
      acc = 0;
      held = 0;
    }
  }
};

struct Token {
  uint16_t at, length, distance;  // distance 0: the literal b[at]
};

// The chunk's candidates: its 3-byte keys sorted with their positions; a position's neighbour below with an equal key is
// the greatest earlier position that starts with the same three bytes.
void candidates(const uint8_t* b, int len, std::vector<uint16_t>* distance) {
  distance->assign(static_cast<size_t>(len), 0);
  if (len < 3) return;
  std::vector<uint64_t> keys(static_cast<size_t>(len - 2));
  for (int i = 0; i + 3 <= len; ++i)
    keys[i] = (static_cast<uint64_t>(b[i]) << 28 | static_cast<uint64_t>(b[i + 1]) << 20 | static_cast<uint64_t>(b[i + 2]) << 12) |
              static_cast<uint64_t>(i);
  std::sort(keys.begin(), keys.end());
  for (size_t r = 1; r < keys.size(); ++r)
    if ((keys[r] >> 12) == (keys[r - 1] >> 12)) (*distance)[keys[r] & 4095u] = static_cast<uint16_t>((keys[r] & 4095u) - (keys[r - 1] & 4095u));
}

void parse(const uint8_t* b, int len, std::vector<Token>* tokens, uint32_t* token_bits) {
  std::vector<uint16_t> distance;
  candidates(b, len, &distance);
  tokens->clear();
  *token_bits = 0;
  int i = 0;
  while (i < len) {
    Token t{static_cast<uint16_t>(i), 1, 0};
    if (distance[i] != 0) {
      const int cap = std::min(gz::kMaxMatch, len - i), j = i - distance[i];
      int l = 0;
      while (l < cap && b[j + l] == b[i + l]) ++l;
      if (l >= 3) {
        t.length = static_cast<uint16_t>(l);
        t.distance = distance[i];
      }
    }
    *token_bits += t.distance != 0 ? gz::match_bits(t.length, t.distance).n : gz::literal_bits(b[i]).n;
    tokens->push_back(t);
    i += t.length;
  }
}

void put_stored_header(std::vector<uint8_t>* out, bool final_block, unsigned len) {
  out->push_back(final_block ? 1 : 0);
  out->push_back(static_cast<uint8_t>(len));
  out->push_back(static_cast<uint8_t>(len >> 8));
  out->push_back(static_cast<uint8_t>(~len));
  out->push_back(static_cast<uint8_t>(~len >> 8));
}

void put_chunk(const uint8_t* b, int len, bool last, std::vector<uint8_t>* out) {
  std::vector<Token> tokens;
  uint32_t token_bits = 0;
  parse(b, len, &tokens, &token_bits);
  if (gz::stored_form_bytes(static_cast<uint32_t>(len)) < gz::fixed_form_bytes(token_bits)) {
    put_stored_header(out, last, static_cast<unsigned>(len));
    out->insert(out->end(), b, b + len);
    return;
  }
  BitWriter w{out};
  w.put(2u, 3);  // BFINAL 0, BTYPE 01
  for (const Token& t : tokens) {
    const Bits bits = t.distance != 0 ? gz::match_bits(t.length, t.distance) : gz::literal_bits(b[t.at]);
    w.put(bits.v, bits.n);
  }
  w.put(0u, 7);                // end of block
  w.put(last ? 1u : 0u, 3);    // the empty stored block that brings the stream to a byte boundary
  w.to_byte();
  out->push_back(0x00);
  out->push_back(0x00);
  out->push_back(0xff);
  out->push_back(0xff);
}

uint32_t crc32_of(const uint8_t* b, int64_t n) {
  uint32_t r = 0xffffffffu;
  for (int64_t i = 0; i < n; ++i) r = kCrc.byte[(r ^ b[i]) & 0xffu] ^ (r >> 8);
  return ~r;
}

}  // namespace
}  // namespace dliom

using namespace dliom;

extern "C" {

int64_t dliom_gzip_bound(int64_t n) {
  if (n < 0) return -1;
  const int64_t chunks = std::max<int64_t>(1, (n + gz::kChunk - 1) / gz::kChunk);
  return gz::kHeaderBytes + gz::kTrailerBytes + n + 5 * chunks;
}

int dliom_gzip_host(const uint8_t* bytes, int64_t n, uint8_t* out, int64_t capacity, int64_t* size) {
  if (size == nullptr || out == nullptr || n < 0 || capacity < 0 || (n > 0 && bytes == nullptr)) return DLIOM_ERR_INVALID_ARGUMENT;
  if (n > DLIOM_GZIP_MAX_SEGMENT) return DLIOM_ERR_TOO_LARGE;
  std::vector<uint8_t> member;
  member.reserve(static_cast<size_t>(dliom_gzip_bound(n)));
  for (unsigned b = 0; b < gz::kHeaderBytes; ++b) member.push_back(static_cast<uint8_t>(gz::header_byte(b)));
  const int64_t chunks = std::max<int64_t>(1, (n + gz::kChunk - 1) / gz::kChunk);
  for (int64_t c = 0; c < chunks; ++c) {
    const int64_t at = c * gz::kChunk;
    put_chunk(bytes + at, static_cast<int>(std::min<int64_t>(gz::kChunk, n - at)), c + 1 == chunks, &member);
  }
  const uint32_t crc = crc32_of(bytes, n), length = static_cast<uint32_t>(n);
  for (int k = 0; k < 4; ++k) member.push_back(static_cast<uint8_t>(crc >> (8 * k)));
  for (int k = 0; k < 4; ++k) member.push_back(static_cast<uint8_t>(length >> (8 * k)));
  *size = static_cast<int64_t>(member.size());
  if (*size > capacity) return DLIOM_ERR_CAPACITY;
  std::memcpy(out, member.data(), member.size());
  return DLIOM_OK;
}

}  // extern "C"
