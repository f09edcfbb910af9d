// float_text.h against the C library: the text of a float must be snprintf("%.6g") of the promoted value, with "-nan" for
// a NaN whose sign bit is set (what glibc prints; stated in dliom.h so that the check does not depend on it).  The header
// is compiled with DLIOM_FLOAT_TEXT_CHECK: every width it claims is an assertion that aborts.
//
//   float_text_check          every 4099th bit pattern of all 2^32 (about a million values), plus the named ties
//   float_text_check --all    all 2^32 bit patterns, on at most 16 threads
//
// Prints one line: "float_text_check: <checked> patterns, <mismatches> mismatches, longest text <n>, multiword <k>".
// Exit status 0 only without mismatches and with no text above 12 characters.
#define DLIOM_FLOAT_TEXT_CHECK 1
#include "float_text.h"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

namespace {

struct Tally {
  uint64_t checked = 0, mismatches = 0, wide = 0;
  int longest = 0;
};

void check_bits(uint32_t bits, Tally* t) {
  float value;
  std::memcpy(&value, &bits, 4);
  char want[32];
  int want_length;
  if (value != value) {
    want_length = std::snprintf(want, sizeof want, "%s", (bits >> 31) ? "-nan" : "nan");
  } else {
    want_length = std::snprintf(want, sizeof want, "%.6g", static_cast<double>(value));
  }
  int wide = 0;
  const dliom::FloatText got = dliom::float_text_of_bits(bits, &wide);
  char text[16];
  for (int i = 0; i < got.length && i < 16; ++i) text[i] = static_cast<char>(dliom::ft_char(got, i));
  ++t->checked;
  t->wide += static_cast<uint64_t>(wide);
  t->longest = std::max(t->longest, got.length);
  if (got.length != want_length || std::memcmp(text, want, static_cast<size_t>(want_length)) != 0) {
    if (t->mismatches < 10)
      std::fprintf(stderr, "bits 0x%08x: got '%.*s', want '%s'\n", bits, got.length, text, want);
    ++t->mismatches;
  }
}

}  // namespace

int main(int argc, char** argv) {
  const bool all = argc > 1 && std::strcmp(argv[1], "--all") == 0;
  Tally total;
  if (all) {
    const unsigned threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<Tally> parts(threads);
    std::vector<std::thread> pool;
    for (unsigned k = 0; k < threads; ++k)
      pool.emplace_back([k, threads, &parts] {
        for (uint64_t b = k; b < (uint64_t{1} << 32); b += threads) check_bits(static_cast<uint32_t>(b), &parts[k]);
      });
    for (std::thread& th : pool) th.join();
    for (const Tally& p : parts) {
      total.checked += p.checked;
      total.mismatches += p.mismatches;
      total.wide += p.wide;
      total.longest = std::max(total.longest, p.longest);
    }
  } else {
    for (uint64_t b = 0; b < (uint64_t{1} << 32); b += 4099) check_bits(static_cast<uint32_t>(b), &total);
    const float named[] = {1000.125f, 100.0625f, 10.03125f, 1.015625f, 100000.5f, 100001.5f, 1234565.0f,
                           999999.5f, 9999995.0f, 0.0001f,  0.00001f,  1e-45f,    3.4028235e38f};
    for (float v : named)
      for (int sign = 0; sign < 2; ++sign) {
        uint32_t bits;
        std::memcpy(&bits, &v, 4);
        check_bits(bits | (static_cast<uint32_t>(sign) << 31), &total);
      }
  }
  std::printf("float_text_check%s: %llu patterns, %llu mismatches, longest text %d, multiword %llu\n", all ? " --all" : "",
              static_cast<unsigned long long>(total.checked), static_cast<unsigned long long>(total.mismatches), total.longest,
              static_cast<unsigned long long>(total.wide));
  return total.mismatches == 0 && total.longest <= dliom::kFloatTextMax ? 0 : 1;
}
