// Gzip members made on the device (dliom.h "gzip on the device").  The work item is a chunk of
// 4096 bytes of a segment; a call compresses K segments of one device buffer in one launch chain:
//   chunk    one workgroup a chunk, everything in LDS -- matches (the 3-byte keys sorted stably with their positions: a
//            position's neighbour below with an equal key is its candidate; the extension length of every position),
//            parse (the greedy token chain out of next[i] by pointer doubling), emit (bit lengths, their scan, the codes
//            OR-ed into the stream; the fixed or stored decision; the chunk's bytes into a slot), and the chunk's share
//            of its segment's CRC-32, already multiplied to its place, XOR-ed into the segment's word
//   scan     of the chunks' sizes, a segment's header and trailer counted with its first and last chunk
//   sizes    the segments' offsets into page-locked memory, then the completion word: the call's ONE polled read-back
//   gather   header, chunks and trailer to their final offsets
// and one download of exactly the compressed bytes.  Integer only; nothing waits for another workgroup.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

#include "device_common.h"
#include "gzip_format.h"
#include "pinned_layout.h"

namespace dliom {
namespace {

constexpr int kThreads = 256;
constexpr int kItems = gz::kChunk / kThreads;  // positions a lane
static_assert(kItems * kThreads == gz::kChunk && gz::kChunk == DLIOM_GZIP_CHUNK, "a lane's positions tile the chunk");
constexpr int kInWords = gz::kChunk / 4 + 4;            // the chunk and zeros behind it: the extension reads two words ahead
constexpr int kOutWords = (gz::kChunk + 5 + 3) / 4;     // a chunk's form never exceeds the stored one
constexpr int kSlotBytes = 4 * (kOutWords + 2);         // the gather reads one word past the form's last
constexpr unsigned kNoKey = 1u << 24;                   // a position with fewer than three bytes left
constexpr int kKeyBits = 25;
constexpr int64_t kMaxSegment = DLIOM_GZIP_MAX_SEGMENT;
constexpr int64_t kGroupSegments = static_cast<int64_t>(kPinGzipSizes.bytes / 8) - 2;  // of one launch chain

__constant__ gz::CrcTables kCrc = gz::make_crc_tables();

__device__ __forceinline__ uint32_t crc_mul_dev(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll 8
  for (int i = 0; i < 32; ++i) {
    p ^= (a & (gz::kCrcOne >> i)) ? b : 0u;
    b = (b >> 1) ^ ((b & 1u) ? gz::kCrcPoly : 0u);
  }
  return p;
}

// the largest s in [0, k) with chunk_first[s] <= c
__device__ __forceinline__ unsigned segment_of(const unsigned* __restrict__ chunk_first, unsigned k, unsigned c) {
  unsigned lo = 0, hi = k - 1u;
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo + 1u) >> 1);
    if (chunk_first[mid] <= c) lo = mid; else hi = mid - 1u;
  }
  return lo;
}

struct ChunkArgs {
  const unsigned char* in;
  const long long* seg_off;      // k + 1, into `in`
  const unsigned* chunk_first;   // k + 1
  unsigned k, chunks;
  unsigned prefix;               // bytes in front of a member: 8 for a size prefix, else 0
  unsigned char* slots;          // kSlotBytes a chunk
  unsigned* sizes;               // a chunk's bytes
  unsigned long long* placed;    // chunks + 1: those bytes plus what the segment puts around them; the last entry 0
  unsigned* crc;                 // k, zeroed: the segments' registers
  unsigned* stored;              // zeroed: chunks in stored form
};

// four bytes from byte p of the LDS copy
__device__ __forceinline__ unsigned load4(const unsigned* w, unsigned p) {
  return __builtin_amdgcn_alignbyte(w[(p >> 2) + 1u], w[p >> 2], p & 3u);
}

__global__ __launch_bounds__(kThreads) void gzip_chunk_kernel(ChunkArgs a) {
  using Sort = hipcub::BlockRadixSort<unsigned, kThreads, kItems, unsigned>;
  using Scan = hipcub::BlockScan<unsigned, kThreads>;
  __shared__ union {
    typename Sort::TempStorage sort;
    struct {
      unsigned out[kOutWords];
      unsigned short length[gz::kChunk];  // a position's token length
      typename Scan::TempStorage scan;
    } emit;
  } u;
  __shared__ unsigned in_w[kInWords];
  __shared__ unsigned short dist[gz::kChunk], nxt[gz::kChunk + 8];
  __shared__ unsigned char start[gz::kChunk + 8];
  __shared__ unsigned edge_key[kThreads], edge_pos[kThreads], wave_crc[kThreads / 64];
  const unsigned char* in_b = reinterpret_cast<const unsigned char*>(in_w);
  const unsigned t = threadIdx.x, c = blockIdx.x;
  const unsigned s = segment_of(a.chunk_first, a.k, c);
  const unsigned first_chunk = a.chunk_first[s], end_chunk = a.chunk_first[s + 1u];
  const bool first = c == first_chunk, last = c + 1u == end_chunk;
  const long long seg_len = a.seg_off[s + 1u] - a.seg_off[s];
  const long long at = static_cast<long long>(c - first_chunk) * gz::kChunk;
  const unsigned len = static_cast<unsigned>(min(static_cast<long long>(gz::kChunk), seg_len - at));
  const unsigned char* src = a.in + a.seg_off[s] + at;

  for (unsigned i = t; i < 4u * kInWords; i += kThreads) reinterpret_cast<unsigned char*>(in_w)[i] = i < len ? src[i] : 0;
  __syncthreads();

  // ---- matches: candidates ----
  unsigned keys[kItems], pos[kItems];
#pragma unroll
  for (int e = 0; e < kItems; ++e) {
    const unsigned i = t * kItems + e;
    pos[e] = i;
    keys[e] = i + 3u <= len ? (static_cast<unsigned>(in_b[i]) << 16 | static_cast<unsigned>(in_b[i + 1u]) << 8 | in_b[i + 2u]) : kNoKey;
  }
  Sort(u.sort).Sort(keys, pos, 0, kKeyBits);  // stable: equal keys keep their positions ascending
  edge_key[t] = keys[kItems - 1];
  edge_pos[t] = pos[kItems - 1];
  __syncthreads();  // (and the sort's storage is free: u.emit lies over it)
#pragma unroll
  for (int e = 0; e < kItems; ++e) {
    const unsigned below_key = e > 0 ? keys[e > 0 ? e - 1 : 0] : (t > 0 ? edge_key[t - 1u] : kNoKey);
    const unsigned below_pos = e > 0 ? pos[e > 0 ? e - 1 : 0] : (t > 0 ? edge_pos[t - 1u] : 0u);
    dist[pos[e]] = keys[e] != kNoKey && keys[e] == below_key ? static_cast<unsigned short>(pos[e] - below_pos) : 0;
  }
  for (unsigned w = t; w < kOutWords; w += kThreads) u.emit.out[w] = 0u;
  __syncthreads();

  // ---- matches: every position's extension; next[i] ----
#pragma unroll 4
  for (int e = 0; e < kItems; ++e) {
    const unsigned i = e * kThreads + t;
    unsigned l = 1u;
    const unsigned d = dist[i];
    if (d != 0u) {  // (then i + 3 <= len and three bytes are equal)
      const unsigned cap = min(static_cast<unsigned>(gz::kMaxMatch), len - i), j = i - d;
      l = 0u;
      while (l < cap) {
        const unsigned x = load4(in_w, i + l) ^ load4(in_w, j + l);
        if (x != 0u) {
          l += static_cast<unsigned>(__ffs(static_cast<int>(x)) - 1) >> 3;
          break;
        }
        l += 4u;
      }
      l = min(l, cap);
    }
    u.emit.length[i] = static_cast<unsigned short>(l);
    nxt[i] = static_cast<unsigned short>(min(i + l, len));
    start[i] = i == 0u ? 1 : 0;
  }
  if (t < 8u) {
    nxt[gz::kChunk + t] = static_cast<unsigned short>(len);
    start[gz::kChunk + t] = 0;
  }
  __syncthreads();

  // ---- parse: the token starts are what the chain from 0 reaches; round r marks the starts 2^r tokens behind a marked
  // one and doubles every jump, so twelve rounds reach all of a chain of at most 4096 tokens ----
  for (int round = 0; round < 12; ++round) {
    unsigned short jump[kItems];
#pragma unroll
    for (int e = 0; e < kItems; ++e) {
      const unsigned i = e * kThreads + t;
      const unsigned n = nxt[i];
      if (start[i] != 0) start[n] = 1;  // (a start marked in this very round may mark on: its target is on the chain too)
      jump[e] = nxt[n];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kItems; ++e) nxt[e * kThreads + t] = jump[e];
    __syncthreads();
  }

  // ---- emit ----
  gz::Bits bits[kItems];
  unsigned mine = 0;
#pragma unroll
  for (int e = 0; e < kItems; ++e) {
    const unsigned i = t * kItems + e;
    bits[e] = gz::Bits{0u, 0u};
    if (i < len && start[i] != 0) {
      const unsigned d = dist[i], l = u.emit.length[i];
      bits[e] = d != 0u && l >= 3u ? gz::match_bits(l, d) : gz::literal_bits(in_b[i]);
    }
    mine += bits[e].n;
  }
  unsigned before, token_bits;
  Scan(u.emit.scan).ExclusiveSum(mine, before, token_bits);
  const unsigned fixed_bytes = gz::fixed_form_bytes(token_bits), stored_bytes = gz::stored_form_bytes(len);
  const bool stored = stored_bytes < fixed_bytes;
  const unsigned size = stored ? stored_bytes : fixed_bytes;
  if (!stored) {
    unsigned o = 3u + before;
#pragma unroll
    for (int e = 0; e < kItems; ++e) {
      if (bits[e].n != 0u) {
        const unsigned sh = o & 31u;
        atomicOr(&u.emit.out[o >> 5], bits[e].v << sh);
        if (sh + bits[e].n > 32u) atomicOr(&u.emit.out[(o >> 5) + 1u], bits[e].v >> (32u - sh));
        o += bits[e].n;
      }
    }
    if (t == 0u) {
      atomicOr(&u.emit.out[0], 2u);  // BFINAL 0, BTYPE 01
      const unsigned final_bit = 3u + token_bits + 7u;  // behind the end-of-block code: the empty stored block's BFINAL
      if (last) atomicOr(&u.emit.out[final_bit >> 5], 1u << (final_bit & 31u));
      for (unsigned b = fixed_bytes - 2u; b < fixed_bytes; ++b) atomicOr(&u.emit.out[b >> 2], 0xffu << (8u * (b & 3u)));
    }
  }
  __syncthreads();
  unsigned* slot = reinterpret_cast<unsigned*>(a.slots + static_cast<size_t>(c) * kSlotBytes);
  for (unsigned w = t; 4u * w < size; w += kThreads) {
    unsigned word;
    if (stored) {
      word = 0u;
#pragma unroll
      for (unsigned k = 0; k < 4u; ++k) {
        const unsigned b = 4u * w + k;
        const unsigned byte = b == 0u ? (last ? 1u : 0u) : b == 1u ? (len & 0xffu) : b == 2u ? (len >> 8) : b == 3u ? (~len & 0xffu)
                              : b == 4u ? ((~len >> 8) & 0xffu) : (b - 5u < len ? in_b[b - 5u] : 0u);
        word |= byte << (8u * k);
      }
    } else {
      word = u.emit.out[w];
    }
    slot[w] = word;
  }
  if (t == 0u) {
    a.sizes[c] = size;
    a.placed[c] = size + (first ? gz::kHeaderBytes + a.prefix : 0u) + (last ? gz::kTrailerBytes : 0u);
    if (c + 1u == a.chunks) a.placed[a.chunks] = 0ull;
    if (stored) atomicAdd(a.stored, 1u);
  }

  // ---- CRC-32: the chunk's bytes right-aligned in 4096 (zeros in front change nothing from register 0), sixteen a lane,
  // every lane's register multiplied to its place; then the chunk's to its place in the segment ----
  unsigned r = 0u;
#pragma unroll
  for (int e = 0; e < kItems; ++e) {
    const int i = static_cast<int>(t * kItems + e) - static_cast<int>(gz::kChunk - len);
    const unsigned byte = i >= 0 ? in_b[i] : 0u;
    r = kCrc.byte[(r ^ byte) & 0xffu] ^ (r >> 8);
  }
  r = crc_mul_dev(r, kCrc.shift16[kThreads - 1u - t]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) r ^= static_cast<unsigned>(__shfl_xor(static_cast<int>(r), off, 64));
  if ((t & 63u) == 0u) wave_crc[t >> 6] = r;
  __syncthreads();
  if (t < 64u) {
    // lanes 0..31: x^(8 * bytes behind the chunk) as the product of the powers its bits name; lanes 32..63: x^(8 * len)
    const unsigned long long behind = static_cast<unsigned long long>(seg_len - at - len);
    const unsigned bit = t & 31u;
    const bool set = t < 32u ? ((behind >> bit) & 1ull) != 0ull : ((len >> bit) & 1u) != 0u;
    unsigned p = set ? kCrc.pow2[bit] : gz::kCrcOne;
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) p = crc_mul_dev(p, static_cast<unsigned>(__shfl_xor(static_cast<int>(p), off, 64)));
    const unsigned by_len = static_cast<unsigned>(__shfl(static_cast<int>(p), 32, 64));
    if (t == 0u) {
      unsigned reg = wave_crc[0] ^ wave_crc[1] ^ wave_crc[2] ^ wave_crc[3];
      if (first) reg ^= crc_mul_dev(0xffffffffu, by_len);  // the register's start value, moved behind the chunk
      atomicXor(&a.crc[s], crc_mul_dev(reg, p));
    }
  }
}

// One workgroup: the segments' offsets in the output and the stored count into page-locked memory, then the completion word.
__global__ __launch_bounds__(kThreads) void gzip_sizes_kernel(const unsigned* __restrict__ chunk_first, unsigned k,
                                                              const unsigned long long* __restrict__ placed_before,
                                                              const unsigned* __restrict__ stored, unsigned long long* pinned,
                                                              unsigned* done_word, unsigned done_seq) {
  for (unsigned s = threadIdx.x; s <= k; s += kThreads) pinned[1u + s] = placed_before[chunk_first[s]];
  if (threadIdx.x == 0) pinned[0] = *stored;
  if (done_word != nullptr) {
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
      __threadfence_system();
      *reinterpret_cast<volatile unsigned*>(done_word) = done_seq;
    }
  }
}

struct GatherArgs {
  const long long* seg_off;
  const unsigned* chunk_first;
  unsigned k, prefix;
  const unsigned char* slots;
  const unsigned* sizes;
  const unsigned long long* placed_before;  // chunks + 1, the last the total
  const unsigned* crc;
  unsigned char* out;  // 256-byte aligned
};

// A chunk's bytes from its slot to their place: whole dwords of the output as dwords (two slot words funnelled into one),
// the bytes in front of the first and behind the last bytewise; the first chunk's lane 0 .. 17 write the size prefix and
// the header, the last chunk's the trailer.
__global__ __launch_bounds__(kThreads) void gzip_gather_kernel(GatherArgs a) {
  const unsigned t = threadIdx.x, c = blockIdx.x;
  const unsigned s = segment_of(a.chunk_first, a.k, c);
  const bool first = c == a.chunk_first[s], last = c + 1u == a.chunk_first[s + 1u];
  const unsigned long long block = a.placed_before[c];
  const unsigned lead = first ? gz::kHeaderBytes + a.prefix : 0u;
  const unsigned size = a.sizes[c];
  const unsigned long long to = block + lead;
  const unsigned* slot = reinterpret_cast<const unsigned*>(a.slots + static_cast<size_t>(c) * kSlotBytes);
  const unsigned char* slot_b = reinterpret_cast<const unsigned char*>(slot);
  const unsigned head = min(size, static_cast<unsigned>((4ull - (to & 3ull)) & 3ull));
  const unsigned words = (size - head) / 4u, tail_at = head + 4u * words;
  if (t < head) a.out[to + t] = slot_b[t];
  unsigned* out_w = reinterpret_cast<unsigned*>(a.out + to + head);
  for (unsigned w = t; w < words; w += kThreads) {
    const unsigned p = head + 4u * w;
    out_w[w] = __builtin_amdgcn_alignbyte(slot[(p >> 2) + 1u], slot[p >> 2], p & 3u);
  }
  if (t < size - tail_at) a.out[to + tail_at + t] = slot_b[tail_at + t];
  if (first && t >= 64u && t < 64u + lead) {
    const unsigned b = t - 64u;
    unsigned byte;
    if (b < a.prefix) {
      const unsigned long long member = a.placed_before[a.chunk_first[s + 1u]] - block - a.prefix;
      byte = static_cast<unsigned>(member >> (8u * b)) & 0xffu;
    } else {
      byte = gz::header_byte(b - a.prefix);
    }
    a.out[block + b] = static_cast<unsigned char>(byte);
  }
  if (last && t >= 128u && t < 128u + gz::kTrailerBytes) {
    const unsigned b = t - 128u;
    const unsigned word = b < 4u ? ~a.crc[s] : static_cast<unsigned>(a.seg_off[s + 1u] - a.seg_off[s]);
    a.out[to + size + b] = static_cast<unsigned char>(word >> (8u * (b & 3u)));
  }
}

bool launched() { return hipGetLastError() == hipSuccess; }

int64_t chunks_of(int64_t n) { return std::max<int64_t>(1, (n + gz::kChunk - 1) / gz::kChunk); }

// One launch chain: the segments [0, k) of `d_in` (k <= kGroupSegments).  Fills out_offsets[0..k] relative to this group's
// first byte; downloads to `out` if the bytes fit `capacity`, else *fits = false.  Waits for the stream before it returns.
int gzip_group(dliom_ctx* ctx, const unsigned char* d_in, const int64_t* offsets, int64_t k, unsigned prefix, uint8_t* out, int64_t capacity,
               int64_t* out_offsets, dliom_gzip_stats* stats, bool* fits) {
  std::vector<long long> seg_off(static_cast<size_t>(k) + 1);
  std::vector<unsigned> chunk_first(static_cast<size_t>(k) + 1);
  int64_t chunks = 0, bound = 0;
  for (int64_t s = 0; s <= k; ++s) {
    seg_off[s] = offsets[s];
    chunk_first[s] = static_cast<unsigned>(chunks);
    if (s < k) {
      chunks += chunks_of(offsets[s + 1] - offsets[s]);
      bound += dliom_gzip_bound(offsets[s + 1] - offsets[s]) + prefix;
    }
  }
  if (chunks > INT32_MAX) return DLIOM_ERR_TOO_LARGE;
  size_t scan_tmp = 0;
  DLIOM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tmp, static_cast<const unsigned long long*>(nullptr),
                                                 static_cast<unsigned long long*>(nullptr), static_cast<int>(chunks + 1), ctx->stream));
  const size_t o_first = align256(8 * (k + 1)), o_zero = o_first + align256(4 * (k + 1)), zero_bytes = align256(4 * (k + 1)),
               o_sizes = o_zero + zero_bytes, o_placed = o_sizes + align256(4 * chunks), o_before = o_placed + align256(8 * (chunks + 1)),
               o_tmp = o_before + align256(8 * (chunks + 1)), o_slots = o_tmp + align256(scan_tmp),
               o_out = o_slots + align256(static_cast<size_t>(chunks) * kSlotBytes), total = o_out + align256(static_cast<size_t>(bound));
  DLIOM_TRY(ctx->gzip.reserve(total));
  char* base = ctx->gzip.as<char>();
  hipStream_t st = ctx->stream;
  auto wait = [&](int status) {
    if (hipStreamSynchronize(st) != hipSuccess && status == DLIOM_OK) status = DLIOM_ERR_HIP;
    ++ctx->host_syncs;
    return status;
  };
  ChunkArgs a;
  a.in = d_in;
  a.seg_off = reinterpret_cast<const long long*>(base);
  a.chunk_first = reinterpret_cast<const unsigned*>(base + o_first);
  a.k = static_cast<unsigned>(k);
  a.chunks = static_cast<unsigned>(chunks);
  a.prefix = prefix;
  a.slots = reinterpret_cast<unsigned char*>(base + o_slots);
  a.sizes = reinterpret_cast<unsigned*>(base + o_sizes);
  a.placed = reinterpret_cast<unsigned long long*>(base + o_placed);
  a.crc = reinterpret_cast<unsigned*>(base + o_zero);
  a.stored = a.crc + k;
  unsigned long long* before = reinterpret_cast<unsigned long long*>(base + o_before);
  // (the host arrays live until the wait at every way out below)
  if (hipMemcpyAsync(base, seg_off.data(), 8 * (k + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(base + o_first, chunk_first.data(), 4 * (k + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(base + o_zero, 0, zero_bytes, st) != hipSuccess)
    return wait(DLIOM_ERR_HIP);
  hipLaunchKernelGGL(gzip_chunk_kernel, dim3(a.chunks), dim3(kThreads), 0, st, a);
  if (!launched()) return wait(DLIOM_ERR_HIP);
  if (hipcub::DeviceScan::ExclusiveSum(base + o_tmp, scan_tmp, a.placed, before, static_cast<int>(chunks + 1), st) != hipSuccess)
    return wait(DLIOM_ERR_HIP);
  unsigned long long* pinned = pinned_at<unsigned long long>(ctx, kPinGzipSizes);
  const unsigned seq = ctx->done_word != nullptr ? next_done_seq(ctx) : 0u;
  hipLaunchKernelGGL(gzip_sizes_kernel, dim3(1), dim3(kThreads), 0, st, a.chunk_first, a.k, before, a.stored, pinned, ctx->done_word, seq);
  if (!launched()) return wait(DLIOM_ERR_HIP);
  GatherArgs g;
  g.seg_off = a.seg_off;
  g.chunk_first = a.chunk_first;
  g.k = a.k;
  g.prefix = prefix;
  g.slots = a.slots;
  g.sizes = a.sizes;
  g.placed_before = before;
  g.crc = a.crc;
  g.out = reinterpret_cast<unsigned char*>(base + o_out);
  hipLaunchKernelGGL(gzip_gather_kernel, dim3(a.chunks), dim3(kThreads), 0, st, g);
  if (!launched()) return wait(DLIOM_ERR_HIP);
  if (ctx->done_word != nullptr) {
    const int st_wait = wait_done(ctx, st, ctx->done_word, seq, 150 + static_cast<int>(std::min<int64_t>(chunks / 8, 100000)));
    if (st_wait != DLIOM_OK) return wait(st_wait);
  } else if (hipStreamSynchronize(st) != hipSuccess) {
    return DLIOM_ERR_HIP;
  }
  for (int64_t s = 0; s <= k; ++s) out_offsets[s] = static_cast<int64_t>(pinned[1 + s]);
  if (stats != nullptr) {
    stats->chunks += chunks;
    stats->chunks_stored += static_cast<int64_t>(pinned[0]);
    ++stats->read_backs;
  }
  const int64_t bytes = out_offsets[k];
  if (bytes > bound) return wait(DLIOM_ERR_INTERNAL);
  *fits = out != nullptr && bytes <= capacity;
  if (*fits && bytes > 0) {
    if (hipMemcpyAsync(out, base + o_out, static_cast<size_t>(bytes), hipMemcpyDeviceToHost, st) != hipSuccess) return wait(DLIOM_ERR_HIP);
    if (stats != nullptr) stats->bytes_downloaded += bytes;
  }
  return wait(DLIOM_OK);
}

int check_offsets(const int64_t* offsets, int64_t k) {
  if (offsets == nullptr || k < 0 || offsets[0] < 0) return DLIOM_ERR_INVALID_ARGUMENT;
  for (int64_t s = 0; s < k; ++s)
    if (offsets[s + 1] < offsets[s]) return DLIOM_ERR_INVALID_ARGUMENT;
  for (int64_t s = 0; s < k; ++s)
    if (offsets[s + 1] - offsets[s] > kMaxSegment) return DLIOM_ERR_TOO_LARGE;
  return DLIOM_OK;
}

}  // namespace

int gzip_on_device(dliom_ctx* ctx, const uint8_t* d_in, const int64_t* offsets, int64_t k, bool size_prefix, uint8_t* out, int64_t capacity,
                   int64_t* out_offsets, dliom_gzip_stats* stats) {
  out_offsets[0] = 0;
  bool all_fit = true;
  for (int64_t g0 = 0; g0 < k; g0 += kGroupSegments) {
    const int64_t g = std::min(kGroupSegments, k - g0), at = out_offsets[g0];
    bool fits = false;
    // (a group behind one that did not fit still runs: the offsets are owed, its bytes are not)
    DLIOM_TRY(gzip_group(ctx, d_in, offsets + g0, g, size_prefix ? 8u : 0u, all_fit ? out + at : nullptr, all_fit ? capacity - at : 0,
                         out_offsets + g0, stats, &fits));
    for (int64_t s = 1; s <= g; ++s) out_offsets[g0 + s] += at;
    out_offsets[g0] = at;
    all_fit = all_fit && fits;
  }
  return all_fit ? DLIOM_OK : DLIOM_ERR_CAPACITY;
}

}  // namespace dliom

using namespace dliom;

extern "C" {

int dliom_gzip_segments(dliom_ctx* ctx, const uint8_t* bytes, const int64_t* offsets, int64_t k, uint8_t* out, int64_t capacity,
                        int64_t* out_offsets, dliom_gzip_stats* stats) {
  if (ctx == nullptr || out == nullptr || out_offsets == nullptr || capacity < 0) return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_TRY(check_offsets(offsets, k));
  const int64_t n = offsets[k] - offsets[0];
  if (n > 0 && bytes == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  if (stats != nullptr) *stats = dliom_gzip_stats{0, 0, 0, 0};
  out_offsets[0] = 0;
  if (k == 0) return DLIOM_OK;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  DLIOM_TRY(ctx->gzip_in.reserve(static_cast<size_t>(std::max<int64_t>(n, 1))));
  // (pageable memory: the copy has left `bytes` when the call returns)
  if (n > 0) DLIOM_HIP_TRY(hipMemcpyAsync(ctx->gzip_in.p, bytes + offsets[0], static_cast<size_t>(n), hipMemcpyHostToDevice, ctx->stream));
  std::vector<int64_t> rel(static_cast<size_t>(k) + 1);
  for (int64_t s = 0; s <= k; ++s) rel[s] = offsets[s] - offsets[0];
  const int st = gzip_on_device(ctx, ctx->gzip_in.as<uint8_t>(), rel.data(), k, false, out, capacity, out_offsets, stats);
  if (st != DLIOM_OK && st != DLIOM_ERR_CAPACITY) (void)hipStreamSynchronize(ctx->stream);  // the upload may still read `bytes`
  return st;
}

int dliom_gzip(dliom_ctx* ctx, const uint8_t* bytes, int64_t n, uint8_t* out, int64_t capacity, int64_t* size, dliom_gzip_stats* stats) {
  if (size == nullptr || n < 0) return DLIOM_ERR_INVALID_ARGUMENT;
  const int64_t offsets[2] = {0, n};
  int64_t out_offsets[2] = {0, 0};
  const int st = dliom_gzip_segments(ctx, bytes, offsets, 1, out, capacity, out_offsets, stats);
  if (st == DLIOM_OK || st == DLIOM_ERR_CAPACITY) *size = out_offsets[1];
  return st;
}

}  // extern "C"
