// The byte format of dliom.h "gzip on the device" (DESIGN.md section 3.31), stated once for the host encoder
// (gzip_host.cc) and the kernels (gzip.hip): a token's bits, the sizes of a chunk's two forms, and CRC-32 as arithmetic
// on polynomials over GF(2) modulo the reflected 0xEDB88320, which is what lets chunks be summed independently.
#ifndef DLIOM_CSRC_GZIP_FORMAT_H_
#define DLIOM_CSRC_GZIP_FORMAT_H_

#include <cstdint>

#ifdef __HIPCC__
#define DLIOM_GZ_HD __host__ __device__ inline
#else
#define DLIOM_GZ_HD inline
#endif

namespace dliom {
namespace gz {

constexpr int kChunk = 4096;  // DLIOM_GZIP_CHUNK
constexpr int kMaxMatch = 258;
constexpr int kHeaderBytes = 10, kTrailerBytes = 8;
// 1f 8b 08 00 00 00 00 00 04 03: deflate, no flags, no time, "fastest", Unix
DLIOM_GZ_HD unsigned header_byte(unsigned b) { return b == 0u ? 0x1fu : b == 1u ? 0x8bu : b == 2u ? 0x08u : b == 8u ? 0x04u : b == 9u ? 0x03u : 0u; }

// a token's bits in stream order: bit 0 of v goes out first
struct Bits {
  uint32_t v, n;
};

// the low n (<= 16) bits of x, mirrored
DLIOM_GZ_HD uint32_t mirror(uint32_t x, uint32_t n) {
  x = ((x & 0x5555u) << 1) | ((x >> 1) & 0x5555u);
  x = ((x & 0x3333u) << 2) | ((x >> 2) & 0x3333u);
  x = ((x & 0x0f0fu) << 4) | ((x >> 4) & 0x0f0fu);
  x = ((x & 0x00ffu) << 8) | ((x >> 8) & 0x00ffu);
  return x >> (16u - n);
}

DLIOM_GZ_HD uint32_t floor_log2(uint32_t x) {  // x >= 1
  uint32_t r = 0;
  while (x >>= 1) ++r;
  return r;
}

// RFC 1951 3.2.6: a literal / length symbol's fixed code, mirrored (Huffman codes go out most significant bit first)
DLIOM_GZ_HD Bits fixed_symbol(uint32_t s) {
  if (s < 144u) return Bits{mirror(0x30u + s, 8), 8};
  if (s < 256u) return Bits{mirror(0x190u + (s - 144u), 9), 9};
  if (s < 280u) return Bits{mirror(s - 256u, 7), 7};
  return Bits{mirror(0xc0u + (s - 280u), 8), 8};
}

DLIOM_GZ_HD Bits literal_bits(uint32_t byte) { return fixed_symbol(byte); }

// (length 3..258, distance 1..32768): length symbol, its extra bits, the 5-bit distance code mirrored, its extra bits;
// extra bits are plain integers, least significant bit first.  At most 8 + 5 + 5 + 13 = 31 bits.
DLIOM_GZ_HD Bits match_bits(uint32_t length, uint32_t distance) {
  uint32_t symbol, extra_bits = 0, extra = 0;
  if (length <= 10u) {
    symbol = 254u + length;
  } else if (length == 258u) {
    symbol = 285u;
  } else {
    const uint32_t m = length - 3u;
    extra_bits = floor_log2(m) - 2u;
    symbol = 257u + 4u * (extra_bits + 1u) + ((m >> extra_bits) - 4u);
    extra = m & ((1u << extra_bits) - 1u);
  }
  Bits b = fixed_symbol(symbol);
  b.v |= extra << b.n;
  b.n += extra_bits;
  uint32_t code, dist_bits = 0, dist_extra = 0;
  if (distance <= 4u) {
    code = distance - 1u;
  } else {
    const uint32_t m = distance - 1u, lg = floor_log2(m);
    dist_bits = lg - 1u;
    code = 2u * lg + ((m >> dist_bits) & 1u);
    dist_extra = m & ((1u << dist_bits) - 1u);
  }
  b.v |= mirror(code, 5) << b.n;
  b.n += 5u;
  b.v |= dist_extra << b.n;
  b.n += dist_bits;
  return b;
}

// bytes of a chunk's two forms; token_bits: the sum over its tokens
DLIOM_GZ_HD uint32_t fixed_form_bytes(uint32_t token_bits) { return (3u + token_bits + 7u + 3u + 7u) / 8u + 4u; }
DLIOM_GZ_HD uint32_t stored_form_bytes(uint32_t len) { return len + 5u; }

// ---- CRC-32 ----
// A 32-bit word is a polynomial of degree < 32, bit 31 the coefficient of x^0 (the reflected convention of the
// table-driven algorithm).  Feeding a zero byte to the register multiplies it by x^8, and the register is linear in
// (register, data), so for a message M of n bytes
//   crc32(M) = ~( 0xffffffff * x^(8n)  ^  raw(M) ),   raw(A | B) = raw(A) * x^(8 |B|) ^ raw(B)
// with raw() the register run from 0 without the final complement.
constexpr uint32_t kCrcPoly = 0xedb88320u;
constexpr uint32_t kCrcOne = 0x80000000u;  // x^0

DLIOM_GZ_HD constexpr uint32_t crc_mul(uint32_t a, uint32_t b) {  // a * b mod P
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (kCrcOne >> i)) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}

struct CrcTables {
  uint32_t byte[256];    // the register after one byte from 0: the classic table
  uint32_t shift16[256]; // x^(8 * 16 * m)
  uint32_t pow2[32];     // x^(8 * 2^k)
};

constexpr CrcTables make_crc_tables() {
  CrcTables t{};
  for (uint32_t b = 0; b < 256; ++b) {
    uint32_t r = b;
    for (int k = 0; k < 8; ++k) r = (r & 1u) ? (r >> 1) ^ kCrcPoly : r >> 1;
    t.byte[b] = r;
  }
  t.pow2[0] = kCrcOne >> 8;
  for (int k = 1; k < 32; ++k) t.pow2[k] = crc_mul(t.pow2[k - 1], t.pow2[k - 1]);
  t.shift16[0] = kCrcOne;
  for (int m = 1; m < 256; ++m) t.shift16[m] = crc_mul(t.shift16[m - 1], t.pow2[4]);
  return t;
}

}  // namespace gz
}  // namespace dliom

#endif  // DLIOM_CSRC_GZIP_FORMAT_H_
