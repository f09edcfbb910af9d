// csrc/point_cloud2_layout.h under -fsanitize=address,undefined: a few thousand random and hostile messages -- field
// tables with offsets and counts up to 2^32 - 1, datatypes outside 1 .. 8, duplicate and missing names, steps of 0, sizes
// that overflow 32 bits when multiplied, data buffers allocated to the byte (a read past the last record is a finding).
// Every accepted plan is checked: each field the plan names lies inside a record, every record inside the buffer.
//   point_cloud2_layout_check <messages> <seed>   prints "accepted A refused R" and exits 0
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../d-liom_amd/csrc/point_cloud2_layout.h"

namespace {

std::mt19937_64 rng;
uint32_t below(uint32_t n) { return static_cast<uint32_t>(rng() % n); }

uint32_t hostile32() {
  switch (below(6)) {
    case 0:
      return 0;
    case 1:
      return 0xFFFFFFFFu;
    case 2:
      return 0x80000000u;
    case 3:
      return 0xFFFFFFFFu - below(16);
    default:
      return below(64);
  }
}

int fail(const char* what, int message) {
  std::printf("message %d: %s\n", message, what);
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  const int messages = argc > 1 ? std::atoi(argv[1]) : 4000;
  rng.seed(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
  const char* kNames[] = {"x", "y", "z", "t", "time", "timestamp", "intensity", "ring", "", "xx"};
  int accepted = 0, refused = 0;
  for (int k = 0; k < messages; ++k) {
    const bool hostile = below(3) == 0;
    const int mode = hostile && below(8) == 0 ? static_cast<int>(below(9)) - 2 : static_cast<int>(below(6));
    dliom_point_cloud2 m{};
    m.point_step = hostile ? hostile32() : 12 + below(40);
    m.width = hostile && below(2) ? hostile32() : below(20);
    m.height = hostile && below(2) ? hostile32() : below(4);
    m.row_step = hostile && below(2) ? hostile32() : m.width * m.point_step + below(9);
    m.is_bigendian = below(40) == 0;
    m.stamp_sec = static_cast<uint32_t>(rng());
    m.stamp_nsec = hostile ? hostile32() : below(1000000000u);
    // the fields: what the mode needs at random places inside the record, some wrong on purpose
    std::vector<std::unique_ptr<std::string>> names;
    std::vector<dliom_point_field> fields;
    const int num = static_cast<int>(below(9));
    for (int f = 0; f < num; ++f) {
      dliom_point_field pf{};
      names.emplace_back(new std::string(kNames[f < 7 && below(8) != 0 ? f : below(10)]));
      pf.name = below(200) == 0 ? nullptr : names.back()->c_str();
      const std::string& s = *names.back();
      pf.datatype = s == "t" ? 6 : s == "timestamp" ? 8 : s == "intensity" ? (mode == 5 ? 2 : 7) : 7;
      if (below(12) == 0) pf.datatype = below(11);
      if (hostile && below(10) == 0) pf.datatype = hostile32();
      pf.count = below(15) == 0 ? (hostile ? hostile32() : below(4)) : 1;
      pf.offset = hostile && below(4) == 0 ? hostile32() : (m.point_step > 8 ? below(m.point_step - 7) : below(4));
      fields.push_back(pf);
    }
    m.num_fields = below(100) == 0 ? -1 : static_cast<int32_t>(fields.size());
    m.fields = fields.empty() && below(2) ? nullptr : fields.data();
    if (fields.empty()) m.num_fields = m.num_fields < 0 ? -1 : 0;
    // the buffer: exactly what the message says it has, when that is allocatable; else a size without bytes behind it
    const uint64_t rows = static_cast<uint64_t>(m.height) * m.row_step;
    std::vector<uint8_t> bytes;
    if (rows <= (1u << 20) && below(10) != 0) {
      m.data_size = rows;
      if (below(10) == 0 && rows > 0) m.data_size = rows - 1 - below(static_cast<uint32_t>(rows));
      bytes.resize(m.data_size);
      for (uint8_t& b : bytes) b = static_cast<uint8_t>(rng());
    } else {
      m.data_size = below(2) ? 0 : below(1000);
      bytes.resize(m.data_size);
    }
    m.data = bytes.empty() ? nullptr : bytes.data();
    dliom::PointCloud2Plan plan{};
    int64_t time = 0;
    const int status = dliom::point_cloud2_plan(below(500) == 0 ? nullptr : &m, mode, &plan, &time);
    if (status != DLIOM_OK) {
      if (status != DLIOM_ERR_INVALID_ARGUMENT) return fail("a status that is neither", k);
      ++refused;
      continue;
    }
    ++accepted;
    if (plan.n != static_cast<uint64_t>(m.height) * m.width || plan.n >= dliom::kPc2MaxPoints) return fail("n", k);
    if (plan.used_bytes > m.data_size) return fail("used_bytes beyond the buffer", k);
    if (plan.n > 0 && static_cast<uint64_t>((plan.n - 1) / m.width) * m.row_step + static_cast<uint64_t>((plan.n - 1) % m.width) * m.point_step +
                              m.point_step != plan.used_bytes)
      return fail("the last record's end", k);
    const uint64_t ends[5] = {plan.off_x + 4ull, plan.off_y + 4ull, plan.off_z + 4ull,
                              plan.time_kind == dliom::kPc2TimeNone ? 0ull : plan.off_time + (plan.time_kind == dliom::kPc2TimeFloat64 ? 8ull : 4ull),
                              plan.intensity_kind == dliom::kPc2IntensityFloat32 ? plan.off_intensity + 4ull
                              : plan.intensity_kind == dliom::kPc2IntensityUint8 ? plan.off_intensity + 1ull : 0ull};
    for (uint64_t e : ends)
      if (e > m.point_step) return fail("a field outside its record", k);
    if (mode <= 2 && plan.n == 0) return fail("a timed mode accepted an empty message", k);
    if (time != dliom::point_cloud2_stamp(m.stamp_sec, m.stamp_nsec) && mode > 1) return fail("the stamp moved in a mode that keeps it", k);
  }
  std::printf("accepted %d refused %d\n", accepted, refused);
  return 0;
}
