// The tables and code bits of d-liom_amd/csrc/gzip_format.h as hex text, for tests/test_gzip_format_host.py to compare with
// arithmetic of its own (polynomials over GF(2), zlib's CRC-32, RFC 1951's tables): every entry of CrcTables,
// fixed_symbol(0..285), match_bits over all lengths at the distances given as arguments and over all distances at the
// lengths 3 and 258, and crc_mul of seeded pairs.
// Stand-alone: g++ -std=c++17 -O2, and once more with -fsanitize=address,undefined.
//   gzip_format_check <distance> ...
// Lines: "byte", "shift16", "pow2" (the words), "sym" (v n pairs), "m <length> <distance> <v> <n>", "mul <a> <b> <product>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../d-liom_amd/csrc/gzip_format.h"

using namespace dliom;

namespace {
constexpr gz::CrcTables kTables = gz::make_crc_tables();

void words(const char* name, const uint32_t* w, int n) {
  std::printf("%s", name);
  for (int i = 0; i < n; ++i) std::printf(" %08x", w[i]);
  std::printf("\n");
}

void match(uint32_t length, uint32_t distance) {
  const gz::Bits b = gz::match_bits(length, distance);
  std::printf("m %u %u %x %u\n", length, distance, b.v, b.n);
}
}  // namespace

int main(int argc, char** argv) {
  words("byte", kTables.byte, 256);
  words("shift16", kTables.shift16, 256);
  words("pow2", kTables.pow2, 32);
  std::printf("sym");
  for (uint32_t s = 0; s <= 285u; ++s) {
    const gz::Bits b = gz::fixed_symbol(s);
    std::printf(" %x %u", b.v, b.n);
  }
  std::printf("\n");
  for (int i = 1; i < argc; ++i) {
    const long d = std::strtol(argv[i], nullptr, 10);
    if (d < 1 || d > 32768) {
      std::fprintf(stderr, "a distance is 1..32768: %s\n", argv[i]);
      return 2;
    }
    for (uint32_t l = 3; l <= 258u; ++l) match(l, static_cast<uint32_t>(d));
  }
  for (uint32_t d = 1; d <= 32768u; ++d) {
    match(3u, d);
    match(258u, d);
  }
  uint64_t x = 0x9e3779b97f4a7c15ull;  // xorshift64
  for (int i = 0; i < 400; ++i) {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    // the corners first: zero, x^0, single bits at both ends
    const uint32_t a = i == 0 ? 0u : i == 1 ? gz::kCrcOne : i == 2 ? 1u : static_cast<uint32_t>(x >> 32);
    const uint32_t b = i == 3 ? 0u : i == 4 ? gz::kCrcOne : i == 5 ? 1u : static_cast<uint32_t>(x);
    std::printf("mul %08x %08x %08x\n", a, b, gz::crc_mul(a, b));
  }
  return 0;
}
