// The head of the point-cloud export on the device: HandleMessage's per-point loop (cartographer_ros/assets_writer.cc:
// 119-160) over transform::TransformInterpolationBuffer (transform/transform_interpolation_buffer.{h,cc},
// transform/timestamped_transform.cc:22-37), equal to the reference bit for bit.
//
// For point i of a message:   time = cloud_time + FromSeconds(t_i);   dropped unless buffer.Has(time);
//   tracking_to_map = buffer.Lookup(time)                  lower_bound over the node times, double slerp, linear blend
//   sensor_to_map   = (tracking_to_map * sensor_to_tracking).cast<float>()
//   out_i           = sensor_to_map * p_i                  float
// The kept points keep their order; the origin is the translation of the last kept point's sensor_to_map.
//
// A dliom_trajectory holds the nodes in HBM and, per interval of neighbouring nodes, what the slerp needs of the
// interval alone: d = q0 . q1, theta = acos |d| and sin theta -- computed once on the HOST, with glibc, when the
// trajectory is made.  What is left per point are sin((1 - f) theta) and sin(f theta): the only two operations in which
// the device (OCML) and the reference's host (glibc) can differ.  Every point whose seven casts to float could land on
// another float under the documented bounds of the two libraries is recorded, recomputed on the host with glibc and
// redone if it differs (assemble_pose is ONE source for both sides): equality is proven per call, not sampled.
#include <cmath>
#include <cstring>
#include <vector>

#include "device_common.h"

namespace dliom {
namespace {

constexpr int kBlock = 256;
constexpr int kRing = 120;                     // records a launch keeps in the words that are read back anyway
enum { kWordBadTime = 0, kWordRecords = 1, /* 2, 7: free */ kWordOrigin = 3 /* 3 floats */, kWordLast = 6, kHeadWords = 8 };
constexpr int kRecordWords = 8;                // point index, bits of the seven floats (tx ty tz qw qx qy qz)
constexpr int kWords = kHeadWords + kRecordWords * kRing;  // 968: one job of read_kept beside the count and the maximum
static_assert(4 * (2 + kWords) <= kPinReadback.bytes && kWords <= 1024, "the call's one read-back: count, maximum, words");
constexpr double kTicksPerSecond = 1e7;        // common::Time: 100 ns

struct AssembleArgs {
  const int64_t* times;  // node times, ascending
  const double* poses;   // 7 a node: tx ty tz qw qx qy qz
  const double* arcs;    // 4 a node: of the interval that ENDS at the node: duration [s], theta, sin theta, d
  int64_t nodes;
  int64_t cloud_time;
  double st[3], sq[4];   // sensor_to_tracking
  double st_max;         // max_k |st[k]|
  int wide;              // record every point of the sin branch (a mount the bound was not derived for; test hooks)
  int perturb;           // libdliom_hooks.so only: the device's rotation is moved by some float ulp for every other time
};

// Eigen Quaterniond product, SSE2 evaluation order (host_math.h::qmul_d), host and device
__host__ __device__ inline void quat_mul(const double* a, const double* b, double* r) {
  const double aw = a[0], ax = a[1], ay = a[2], az = a[3];
  const double bw = b[0], bx = b[1], by = b[2], bz = b[3];
  const double t1x = aw * bx + ay * bz, t1y = aw * by + ay * bw;
  const double t2x = az * bx - ax * bz, t2y = az * by - ax * bw;
  const double u1z = aw * bz - ay * bx, u1w = aw * bw - ay * by;
  const double u2z = az * bz + ax * bx, u2w = az * bw + ax * by;
  r[1] = t1x - t2y;
  r[2] = t1y + t2x;
  r[3] = u1z + u2w;
  r[0] = u1w - u2z;
}

// common::FromSeconds(t): duration_cast of a double count of seconds to 100 ns ticks truncates; undefined (refused) for
// a product that is not finite or not below 2^63 in magnitude
__host__ __device__ inline bool ticks_of(float t, int64_t* ticks) {
  const double x = static_cast<double>(t) * kTicksPerSecond;
  if (!(fabs(x) < 9223372036854775808.0)) return false;
  *ticks = static_cast<int64_t>(x);
  return true;
}
__host__ __device__ inline int64_t time_of(int64_t cloud_time, int64_t ticks) {
  return static_cast<int64_t>(static_cast<uint64_t>(cloud_time) + static_cast<uint64_t>(ticks));
}

__host__ __device__ inline bool has_time(const AssembleArgs& a, int64_t time) {
  return a.nodes > 0 && a.times[0] <= time && time <= a.times[a.nodes - 1];
}

// lookup_pose: buffer.Lookup(time) for a time the buffer has, translation o and rotation r (w x y z), with dr[k], how far
// r[k] can be from the host's.  assemble_pose: (Lookup(time) * sensor_to_tracking) before the cast, v = tx ty tz qw qx qy qz.
// ONE source for the kernel and for the host's check: `sin` is the device's (OCML) there and glibc's here.
// *libm_path: the slerp took its sin branch; only then can the two sides differ, and b[k] bounds by how much:
//
//   Documented bounds: the device's double sin is within 4 ulp (OpenCL full profile, what OCML is built to), glibc's
//   within 1 ulp, so two results for one argument differ by <= 5 u relative, u = 2^-52.  theta, sin theta and the
//   arguments (1 - f) theta, f theta are the same doubles on both sides (IEEE operations on the same inputs).  e = 10 u:
//   the 5 u doubled, the margin the de-skew's bound takes as well.  Two different inputs of a correctly rounded operation
//   give results at most |difference| + 1 ulp apart.
//     scale0, scale1 (quotients by the same sin theta):           relative  es = e + 2 u
//     r[k] = scale0 q0[k] + scale1 q1[k]:    dr[k] = (es + 3 u) (|scale0 q0[k]| + |scale1 q1[k]|),  D = max_k dr[k]
//     rotation qq = r * sq (Hamilton product, |r[k]|, |sq[k]| <= 1.031):   dq[k] = sum_j |sq[perm_k(j)]| dr[j] + 14 u
//     normalisation, z2 = |qq|^2 in [0.96, 1.04]:  z2 moves by <= 2 sum_j |qq[j]| dq[j] + 4 u z2, its root by half of that
//       relative plus one rounding, the quotient by one more:   b[3 + k] = 1.03 dq[k] + |v[3 + k]| (1.05 sum + 8 u)
//     translation r * st + o  (o, the blended translation, has no sin in it), S = max |st[k]|, rho = max |r[k]| <= 1.031:
//       uv = 2 (r x st): 4 D S + 8 u rho S;   r x uv: 16 rho D S + 32 u rho^2 S;   r_w uv: 8 rho D S + 12 u rho^2 S;
//       three additions: u (3 S + 28 rho^2 S + |o[k]|), |o[k]| <= |v[k]| + 13.8 S
//                                                                b[k] = 25 D S + 100 u S + 2 u |v[k]|
//   A pose outside those assumptions (|qq|^2 outside [0.96, 1.04], a mount quaternion that is not a unit quaternion)
//   makes *wide true: the point is checked on the host whatever its casts.
__host__ __device__ inline void lookup_pose(const AssembleArgs& a, int64_t time, double o[3], double r[4], double dr[4],
                                            bool* libm_path) {
  int64_t lo = 0, hi = a.nodes;  // std::lower_bound: the first node with node.time >= time
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a.times[mid] < time) lo = mid + 1;
    else hi = mid;
  }
  const double* pe = a.poses + 7 * lo;
  *libm_path = false;
  if (a.times[lo] == time) {  // end->time == time: end->transform
    for (int k = 0; k < 3; ++k) o[k] = pe[k];
    for (int k = 0; k < 4; ++k) {
      r[k] = pe[3 + k];
      dr[k] = 0.0;
    }
    return;
  }
  // Interpolate(*std::prev(end), *end, time)
  const double* ps = pe - 7;
  const double* arc = a.arcs + 4 * lo;
  const double factor = (static_cast<double>(time - a.times[lo - 1]) / kTicksPerSecond) / arc[0];
  for (int k = 0; k < 3; ++k) o[k] = ps[k] + (pe[k] - ps[k]) * factor;
  // Eigen::Quaterniond(start).slerp(factor, end): 1 - epsilon threshold, sign flip for d < 0, no renormalisation
  const double one = 1.0 - 2.220446049250313e-16;
  const double d = arc[3];
  double scale0, scale1;
  if (fabs(d) >= one) {
    scale0 = 1.0 - factor;
    scale1 = factor;
  } else {
    const double theta = arc[1], sin_theta = arc[2];  // acos(absD), sin(theta): the interval's, glibc's on both sides
    scale0 = sin((1.0 - factor) * theta) / sin_theta;
    scale1 = sin(factor * theta) / sin_theta;
    *libm_path = true;
  }
  if (d < 0.0) scale1 = -scale1;
#if defined(DLIOM_TEST_HOOKS) && defined(__HIP_DEVICE_COMPILE__)
  if (a.perturb && *libm_path && (time & 1) == 0) scale1 *= 1.0 + 16.0 / 16777216.0;
#endif
  const double u = 2.220446049250313e-16, es = 12.0 * u;
  for (int k = 0; k < 4; ++k) {
    r[k] = scale0 * ps[3 + k] + scale1 * pe[3 + k];
    dr[k] = (es + 3.0 * u) * (fabs(scale0 * ps[3 + k]) + fabs(scale1 * pe[3 + k]));
  }
}

__host__ __device__ inline void assemble_pose(const AssembleArgs& a, int64_t time, double v[7], double b[7], bool* libm_path,
                                              bool* wide) {
  double o[3], r[4], dr[4];
  lookup_pose(a, time, o, r, dr, libm_path);
  *wide = a.wide != 0;
  // tracking_to_map * sensor_to_tracking: translation r * st + o, rotation (r * sq).normalized()
  {
    const double* s = a.st;
    double uvx = r[2] * s[2] - r[3] * s[1], uvy = r[3] * s[0] - r[1] * s[2], uvz = r[1] * s[1] - r[2] * s[0];
    uvx += uvx;
    uvy += uvy;
    uvz += uvz;
    const double cx = r[2] * uvz - r[3] * uvy, cy = r[3] * uvx - r[1] * uvz, cz = r[1] * uvy - r[2] * uvx;
    v[0] = ((s[0] + r[0] * uvx) + cx) + o[0];
    v[1] = ((s[1] + r[0] * uvy) + cy) + o[1];
    v[2] = ((s[2] + r[0] * uvz) + cz) + o[2];
  }
  double qq[4];
  quat_mul(r, a.sq, qq);
  const double z2 = (qq[1] * qq[1] + qq[3] * qq[3]) + (qq[2] * qq[2] + qq[0] * qq[0]);
  if (z2 > 0.0) {
    const double nrm = sqrt(z2);
    for (int k = 0; k < 4; ++k) v[3 + k] = qq[k] / nrm;
  } else {
    for (int k = 0; k < 4; ++k) v[3 + k] = qq[k];
  }
  if (!*libm_path) return;
  const double u = 2.220446049250313e-16;
  const double big = fmax(fmax(dr[0], dr[1]), fmax(dr[2], dr[3]));
  for (int k = 0; k < 3; ++k) b[k] = 25.0 * big * a.st_max + 100.0 * u * a.st_max + 2.0 * u * fabs(v[k]);
  const double s0 = fabs(a.sq[0]), s1 = fabs(a.sq[1]), s2 = fabs(a.sq[2]), s3 = fabs(a.sq[3]);
  const double dq[4] = {dr[0] * s0 + dr[1] * s1 + dr[2] * s2 + dr[3] * s3 + 14.0 * u, dr[0] * s1 + dr[1] * s0 + dr[2] * s3 + dr[3] * s2 + 14.0 * u,
                        dr[0] * s2 + dr[1] * s3 + dr[2] * s0 + dr[3] * s1 + 14.0 * u, dr[0] * s3 + dr[1] * s2 + dr[2] * s1 + dr[3] * s0 + 14.0 * u};
  const double sum = fabs(qq[0]) * dq[0] + fabs(qq[1]) * dq[1] + fabs(qq[2]) * dq[2] + fabs(qq[3]) * dq[3];
  for (int k = 0; k < 4; ++k) b[3 + k] = 1.03 * dq[k] + fabs(v[3 + k]) * (1.05 * sum + 8.0 * u);
  if (!(z2 >= 0.96 && z2 <= 1.04) || !(big < 1e-9)) *wide = true;
}

// Could the cast of v land on another float if v were off by up to `bound`?  (preprocess.hip's test)
__host__ __device__ inline bool cast_moves(double v, double bound) {
  const float f = static_cast<float>(v);
  return static_cast<float>(v + bound) != f || static_cast<float>(v - bound) != f;
}

// sensor_to_map * p in float: rotate_point plus the translation
__device__ __forceinline__ void transform_point(const float f[7], float px, float py, float pz, float* x, float* y, float* z) {
  float rx, ry, rz;
  rotate_point(Quat4{f[3], f[4], f[5], f[6]}, px, py, pz, rx, ry, rz);
  *x = rx + f[0];
  *y = ry + f[1];
  *z = rz + f[2];
}

// Point i: keep[i] = Has(time_i); the transformed point goes to x/y/z[i] (compacted by compact.hip's scatter).  Returns the
// norm word of a kept point, else 0.
__device__ __forceinline__ unsigned assemble_point(const AssembleArgs& a, const float4* __restrict__ points, unsigned i,
                                                   float* __restrict__ x, float* __restrict__ y, float* __restrict__ z,
                                                   unsigned* __restrict__ keep, unsigned* __restrict__ words, int only_records) {
  const float4 p = points[i];
  int64_t ticks;
  if (!ticks_of(p.w, &ticks)) {
    if (!only_records) {
      atomicOr(&words[kWordBadTime], 1u);
      keep[i] = 0u;
    }
    return 0u;
  }
  const int64_t time = time_of(a.cloud_time, ticks);
  if (!has_time(a, time)) {
    if (!only_records) keep[i] = 0u;
    return 0u;
  }
  double v[7], b[7];
  bool libm_path, wide;
  assemble_pose(a, time, v, b, &libm_path, &wide);
  float f[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) f[k] = static_cast<float>(v[k]);
  if (libm_path) {
    bool ambiguous = wide;
#pragma unroll
    for (int k = 0; k < 7; ++k) ambiguous = ambiguous || cast_moves(v[k], b[k]);
    if (ambiguous) {
      const unsigned r = atomicAdd(only_records ? words : words + kWordRecords, 1u);
      if (only_records || r < static_cast<unsigned>(kRing)) {
        unsigned* rec = only_records ? words + 1 + kRecordWords * static_cast<size_t>(r) : words + kHeadWords + kRecordWords * r;
        rec[0] = i;
#pragma unroll
        for (int k = 0; k < 7; ++k) rec[1 + k] = __float_as_uint(f[k]);
      }
    }
  }
  if (only_records) return 0u;
  float ox, oy, oz;
  transform_point(f, p.x, p.y, p.z, &ox, &oy, &oz);
  x[i] = ox;
  y[i] = oy;
  z[i] = oz;
  keep[i] = 1u;
  return norm_word(ox, oy, oz);
}

// One point a thread.  words: the call's device words (kWords of them, layout above); max_sq: the compaction's.  only_records:
// nothing but the records is written, into `words` = [count | records] with room for every point (after a ring overflowed).
__global__ __launch_bounds__(kBlock) void assemble_kernel(AssembleArgs a, const float4* __restrict__ points, unsigned n,
                                                          float* __restrict__ x, float* __restrict__ y, float* __restrict__ z,
                                                          unsigned* __restrict__ keep, unsigned* __restrict__ words,
                                                          unsigned* __restrict__ max_sq, int only_records) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  const unsigned word = i < n ? assemble_point(a, points, i, x, y, z, keep, words, only_records) : 0u;
  if (!only_records) note_kept(word, max_sq);
}

// "We use the last transform for the origin": sensor_to_map * Zero of the last kept point, found in the scan of the keep
// flags (the first index at which the inclusive sum reaches its total).  One thread.
__global__ void assemble_origin_kernel(AssembleArgs a, const float4* __restrict__ points, unsigned n,
                                       const unsigned* __restrict__ inclusive, unsigned* __restrict__ words) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const unsigned total = inclusive[n - 1];
  if (total == 0u) return;
  unsigned lo = 0, hi = n - 1;
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo) >> 1);
    if (inclusive[mid] < total) lo = mid + 1;
    else hi = mid;
  }
  int64_t ticks;
  if (!ticks_of(points[lo].w, &ticks)) return;  // (cannot happen: the point was kept)
  double v[7], b[7];
  bool libm_path, wide;
  assemble_pose(a, time_of(a.cloud_time, ticks), v, b, &libm_path, &wide);
  float f[7];
  for (int k = 0; k < 7; ++k) f[k] = static_cast<float>(v[k]);
  float ox, oy, oz;
  transform_point(f, 0.f, 0.f, 0.f, &ox, &oy, &oz);
  words[kWordOrigin] = __float_as_uint(ox);
  words[kWordOrigin + 1] = __float_as_uint(oy);
  words[kWordOrigin + 2] = __float_as_uint(oz);
  words[kWordLast] = lo;
}

// The points the host's check found different: redone with the host's seven floats.  fixes: kRecordWords words each.
__global__ void assemble_fix_kernel(const float4* __restrict__ points, unsigned n, float* __restrict__ x, float* __restrict__ y,
                                    float* __restrict__ z, const unsigned* __restrict__ fixes, int num_fixes, unsigned last,
                                    unsigned* __restrict__ words) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= num_fixes) return;
  const unsigned i = fixes[kRecordWords * j];
  if (i >= n) return;
  float f[7];
  for (int k = 0; k < 7; ++k) f[k] = __uint_as_float(fixes[kRecordWords * j + 1 + k]);
  const float4 p = points[i];
  transform_point(f, p.x, p.y, p.z, &x[i], &y[i], &z[i]);
  if (i == last) {
    float ox, oy, oz;
    transform_point(f, 0.f, 0.f, 0.f, &ox, &oy, &oz);
    words[kWordOrigin] = __float_as_uint(ox);
    words[kWordOrigin + 1] = __float_as_uint(oy);
    words[kWordOrigin + 2] = __float_as_uint(oz);
  }
}

// Every record once more on the HOST -- assemble_pose with glibc's sin, the reference's own -- against the floats the
// device cast.  The points that differ (never observed outside the hooks build) go to *fixes with the host's floats.
void check_records(const AssembleArgs& host_args, const float* points_xyzt, int64_t n, const unsigned* recs, size_t count,
                   std::vector<unsigned>* fixes) {
  for (size_t r = 0; r < count; ++r) {
    const unsigned* rec = recs + kRecordWords * r;
    if (rec[0] >= static_cast<uint64_t>(n)) continue;
    int64_t ticks;
    if (!ticks_of(points_xyzt[4 * static_cast<size_t>(rec[0]) + 3], &ticks)) continue;
    double v[7], b[7];
    bool libm_path, wide;
    assemble_pose(host_args, time_of(host_args.cloud_time, ticks), v, b, &libm_path, &wide);
    unsigned bits[7];
    bool same = true;
    for (int k = 0; k < 7; ++k) {
      const float f = static_cast<float>(v[k]);
      std::memcpy(&bits[k], &f, 4);
      same = same && bits[k] == rec[1 + k];
    }
    if (!same) {
      fixes->push_back(rec[0]);
      for (int k = 0; k < 7; ++k) fixes->push_back(bits[k]);
    }
  }
}

inline unsigned blocks_of(int64_t n) { return dliom::blocks_of(n, kBlock); }

bool pose_is_finite(const double* p) {
  for (int k = 0; k < 7; ++k)
    if (!std::isfinite(p[k])) return false;
  return true;
}

}  // namespace
}  // namespace dliom

using namespace dliom;

struct dliom_trajectory {
  dliom_ctx* ctx = nullptr;  // null: a host-only buffer (dliom_trajectory_lookup); not touched by destroy
  int device = 0;            // of d_base
  std::vector<int64_t> times;
  std::vector<double> poses, arcs;
  void* d_base = nullptr;  // times | poses | arcs, uploaded by the first call that needs them
  AssembleArgs view(bool device) const {
    AssembleArgs a{};
    const size_t n = times.size();
    if (device) {
      char* b = static_cast<char*>(d_base);
      a.times = reinterpret_cast<const int64_t*>(b);
      a.poses = reinterpret_cast<const double*>(b + align256(8 * n));
      a.arcs = reinterpret_cast<const double*>(b + align256(8 * n) + align256(56 * n));
    } else {
      a.times = times.data();
      a.poses = poses.data();
      a.arcs = arcs.data();
    }
    a.nodes = static_cast<int64_t>(n);
    return a;
  }
  int upload() {
    if (d_base != nullptr || times.empty()) return DLIOM_OK;
    const size_t n = times.size();
    const size_t o1 = align256(8 * n), o2 = o1 + align256(56 * n), total = o2 + align256(32 * n);
    void* base = nullptr;
    DLIOM_HIP_TRY(hipMalloc(&base, total));
    char* b = static_cast<char*>(base);
    if (hipMemcpyAsync(b, times.data(), 8 * n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(b + o1, poses.data(), 56 * n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(b + o2, arcs.data(), 32 * n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) {
      (void)hipFree(base);
      return DLIOM_ERR_HIP;
    }
    d_base = base;
    device = ctx->device;
    return DLIOM_OK;
  }
};

extern "C" {

int dliom_trajectory_create(dliom_ctx* ctx, const int64_t* times, const double* poses7, int64_t n, dliom_trajectory** out) {
  if (out == nullptr || n < 0 || (n > 0 && (times == nullptr || poses7 == nullptr))) return DLIOM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  for (int64_t i = 1; i < n; ++i)
    if (times[i] < times[i - 1]) return DLIOM_ERR_INVALID_ARGUMENT;  // Push: CHECK_GE(time, latest_time())
  dliom_trajectory* t = new dliom_trajectory;
  t->ctx = ctx;
  t->times.assign(times, times + n);
  t->poses.assign(poses7, poses7 + 7 * n);
  t->arcs.assign(4 * static_cast<size_t>(n), 0.0);
  for (int64_t i = 1; i < n; ++i) {
    const double* a = poses7 + 7 * (i - 1) + 3;  // w x y z
    const double* b = a + 7;
    double* arc = &t->arcs[4 * static_cast<size_t>(i)];
    arc[0] = static_cast<double>(times[i] - times[i - 1]) / kTicksPerSecond;  // common::ToSeconds(end.time - start.time)
    const double d = (a[1] * b[1] + a[3] * b[3]) + (a[2] * b[2] + a[0] * b[0]);  // coeffs().dot(): two Packet2d, then predux
    arc[3] = d;
    if (!(std::fabs(d) >= 1.0 - 2.220446049250313e-16)) {
      arc[1] = std::acos(std::fabs(d));
      arc[2] = std::sin(arc[1]);
    }
  }
  *out = t;
  return DLIOM_OK;
}

int dliom_trajectory_destroy(dliom_trajectory* t) {
  if (t == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  if (t->d_base != nullptr) {
    // (the context may be gone already: hipFree waits for the device's outstanding work itself)
    (void)hipSetDevice(t->device);
    (void)hipFree(t->d_base);
  }
  delete t;
  return DLIOM_OK;
}

int dliom_trajectory_size(const dliom_trajectory* t, int64_t* n) {
  if (t == nullptr || n == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *n = static_cast<int64_t>(t->times.size());
  return DLIOM_OK;
}

int dliom_trajectory_lookup(const dliom_trajectory* t, int64_t time, int* has, double pose7[7]) {
  if (t == nullptr || has == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  AssembleArgs a = t->view(false);
  *has = has_time(a, time) ? 1 : 0;
  if (*has == 0 || pose7 == nullptr) return DLIOM_OK;
  double dr[4];
  bool libm_path;
  lookup_pose(a, time, pose7, pose7 + 3, dr, &libm_path);
  return DLIOM_OK;
}

}  // extern "C"

// intensities (host, n floats, may be null): uploaded once beside the points; the kept ones are gathered by the indices the
// scatter leaves in scratch into *kept_intensities (an empty block of the caller's; left empty when nothing is kept).
// device_points: both are in HBM already (internal.h); the points the check records are fetched from there.
int dliom::assemble_from_sensor_points(dliom_ctx* ctx, dliom_trajectory* traj, int64_t cloud_time, const float* points_xyzt,
                                       const DevicePoints* device_points, int64_t n, const double sensor_to_tracking[7],
                                       dliom_cloud** out, float origin[3], int32_t* kept_index, int64_t capacity, int64_t* num_kept,
                                       const float* intensities, AttrBlock* kept_intensities) {
  const bool on_device = device_points != nullptr;
  if (ctx == nullptr || traj == nullptr || traj->ctx != ctx || sensor_to_tracking == nullptr || out == nullptr || origin == nullptr ||
      num_kept == nullptr || n < 0 || n > INT32_MAX || capacity < 0 || (n > 0 && !on_device && points_xyzt == nullptr) ||
      (n > 0 && on_device && device_points->xyzt == nullptr) || !pose_is_finite(sensor_to_tracking))
    return DLIOM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  *num_kept = 0;
  if (n == 0) return DLIOM_OK;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  DLIOM_TRY(traj->upload());
  AssembleArgs a = traj->view(true);
  a.cloud_time = cloud_time;
  for (int k = 0; k < 3; ++k) a.st[k] = sensor_to_tracking[k];
  for (int k = 0; k < 4; ++k) a.sq[k] = sensor_to_tracking[3 + k];
  a.st_max = std::fmax(std::fabs(a.st[0]), std::fmax(std::fabs(a.st[1]), std::fabs(a.st[2])));
  const double sn = (a.sq[1] * a.sq[1] + a.sq[3] * a.sq[3]) + (a.sq[2] * a.sq[2] + a.sq[0] * a.sq[0]);
  a.wide = (sn >= 0.98 && sn <= 1.02) ? 0 : 1;
#ifdef DLIOM_TEST_HOOKS  // libdliom_hooks.so: 4 records every point of the sin branch (the ring overflows), 5 also perturbs
  if (ctx->tuning[DLIOM_TUNE_RESERVED_TEST_HOOK] >= 4) a.wide = 1;
  if (ctx->tuning[DLIOM_TUNE_RESERVED_TEST_HOOK] == 5) a.perturb = 1;
#endif
  // behind the compaction's scratch: words | raw points | x | y | z | intensities (raw points, intensities: host input only)
  const unsigned un = static_cast<unsigned>(n);
  const size_t per = align256(4 * static_cast<size_t>(n)), raw = on_device ? 0 : align256(16 * static_cast<size_t>(n)),
               wb = align256(4 * kWords);
  CompactScratch s;
  DLIOM_TRY(carve_compact(ctx, n, &s, wb + raw + 3 * per + (intensities != nullptr ? per : 0), 4 * kHeadWords));
  char* base = static_cast<char*>(s.extra);
  unsigned* words = reinterpret_cast<unsigned*>(base);
  const float4* d_points = on_device ? device_points->xyzt : reinterpret_cast<const float4*>(base + wb);
  float* x = reinterpret_cast<float*>(base + wb + raw);
  float* y = reinterpret_cast<float*>(base + wb + raw + per);
  float* z = reinterpret_cast<float*>(base + wb + raw + 2 * per);
  const float* d_intensities = on_device ? device_points->intensities : nullptr;
  if (!on_device) {
    DLIOM_HIP_TRY(hipMemcpyAsync(base + wb, points_xyzt, 16 * static_cast<size_t>(n), hipMemcpyHostToDevice, ctx->stream));
    if (intensities != nullptr) {
      float* staged = reinterpret_cast<float*>(base + wb + raw + 3 * per);
      DLIOM_HIP_TRY(hipMemcpyAsync(staged, intensities, 4 * static_cast<size_t>(n), hipMemcpyHostToDevice, ctx->stream));
      d_intensities = staged;
    }
  }
  hipLaunchKernelGGL(assemble_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, a, d_points, un, x, y, z, s.keep, words, s.max_sq, 0);
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_TRY(scan_kept(ctx, n, s));
  hipLaunchKernelGGL(assemble_origin_kernel, dim3(1), dim3(64), 0, ctx->stream, a, d_points, un, s.inclusive, words);
  DLIOM_HIP_TRY(hipGetLastError());
  const GatherJob words_job{words, static_cast<unsigned>(kWords)};
  int64_t kept;
  float max_sq;
  std::vector<unsigned> head(kWords);  // (a copy: the pinned block is reused by the calls below)
  DLIOM_TRY(read_kept(ctx, n, s, &words_job, &kept, &max_sq, head.data()));
  if (head[kWordBadTime] != 0u) return DLIOM_ERR_INVALID_ARGUMENT;  // nothing was written
  *num_kept = kept;
  if (kept_index != nullptr && capacity < kept) return DLIOM_ERR_CAPACITY;
  if (kept == 0) return DLIOM_OK;  // the reference returns nullptr for such a message
  // ---- the check: recorded points against glibc
  const unsigned recorded = head[kWordRecords];
  ctx->assemble_recorded += recorded;
  if (recorded > 0) {
    AssembleArgs h = traj->view(false);
    h.cloud_time = cloud_time;
    std::memcpy(h.st, a.st, sizeof a.st);
    std::memcpy(h.sq, a.sq, sizeof a.sq);
    h.st_max = a.st_max;
    std::vector<unsigned> fixes;
    std::vector<float> fetched;  // a decoded message's points, for the recorded ones' times (rare: one more synchronise)
    if (on_device) {
      fetched.resize(4 * static_cast<size_t>(n));
      DLIOM_HIP_TRY(hipMemcpyAsync(fetched.data(), d_points, 16 * static_cast<size_t>(n), hipMemcpyDeviceToHost, ctx->stream));
      DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
      ++ctx->host_syncs;
      points_xyzt = fetched.data();
    }
    if (recorded <= static_cast<unsigned>(kRing)) {
      check_records(h, points_xyzt, n, head.data() + kHeadWords, recorded, &fixes);
      ctx->assemble_recomputed += recorded;
    } else {
      // more records than the ring holds: a records-only pass over every point into a list with room for all of them
      ++ctx->assemble_overflows;
      const size_t list_words = 1 + kRecordWords * static_cast<size_t>(n);
      DLIOM_TRY(ctx->sort_tmp.reserve(4 * list_words));
      unsigned* d_list = ctx->sort_tmp.as<unsigned>();
      DLIOM_HIP_TRY(hipMemsetAsync(d_list, 0, 4, ctx->stream));
      hipLaunchKernelGGL(assemble_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, ctx->stream, a, d_points, un, x, y, z, s.keep, d_list, s.max_sq, 1);
      DLIOM_HIP_TRY(hipGetLastError());
      unsigned count = 0;
      DLIOM_HIP_TRY(hipMemcpyAsync(&count, d_list, 4, hipMemcpyDeviceToHost, ctx->stream));
      DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
      ++ctx->host_syncs;
      if (count > un) return DLIOM_ERR_INTERNAL;
      std::vector<unsigned> recs(kRecordWords * static_cast<size_t>(count));
      if (count > 0) {
        DLIOM_HIP_TRY(hipMemcpy(recs.data(), d_list + 1, 4 * recs.size(), hipMemcpyDeviceToHost));
        check_records(h, points_xyzt, n, recs.data(), count, &fixes);
      }
      ctx->assemble_recomputed += count;
    }
    if (!fixes.empty()) {  // the device's cast differs from glibc's for these points -- glibc's is the reference's
      const int nf = static_cast<int>(fixes.size() / kRecordWords);
      ctx->assemble_fixed += nf;
      DLIOM_TRY(ctx->sort_tmp.reserve(4 * fixes.size()));
      DLIOM_HIP_TRY(hipMemcpyAsync(ctx->sort_tmp.p, fixes.data(), 4 * fixes.size(), hipMemcpyHostToDevice, ctx->stream));
      hipLaunchKernelGGL(assemble_fix_kernel, dim3(dliom::blocks_of(nf, 64)), dim3(64), 0, ctx->stream, d_points, un, x, y, z,
                         ctx->sort_tmp.as<unsigned>(), nf, head[kWordLast], words);
      DLIOM_HIP_TRY(hipGetLastError());
      const FillJob zero_max{s.max_sq, 4, 0u};
      DLIOM_TRY(fill_multi(ctx, &zero_max, 1));
      DLIOM_TRY(max_of_kept(ctx, x, y, z, n, s));
      DLIOM_HIP_TRY(hipMemcpyAsync(head.data(), words, 4 * kHeadWords, hipMemcpyDeviceToHost, ctx->stream));
      DLIOM_HIP_TRY(hipMemcpyAsync(&max_sq, s.max_sq, 4, hipMemcpyDeviceToHost, ctx->stream));
      DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));  // `fixes` dies with this scope
      ++ctx->host_syncs;
    }
  }
  // ---- the cloud: the kept points in input order, and their intensities by the indices the scatter leaves in scratch
  DLIOM_TRY(emit_kept(ctx, x, y, z, n, s, kept, max_sq, out, kept_index));
  if (d_intensities != nullptr) {
    int st = kept_intensities->alloc(ctx, static_cast<size_t>(kept));
    if (st == DLIOM_OK) st = gather_batch_attributes(ctx, s.index, kept, d_intensities, nullptr, kept_intensities->p, nullptr);
    if (st != DLIOM_OK) {
      dliom_cloud_destroy(*out);
      *out = nullptr;
      kept_intensities->release(ctx);
      return st;
    }
  }
  std::memcpy(origin, &head[kWordOrigin], 12);
  return DLIOM_OK;
}

extern "C" {

int dliom_cloud_from_sensor_points(dliom_ctx* ctx, dliom_trajectory* traj, int64_t cloud_time, const float* points_xyzt, int64_t n,
                                   const double sensor_to_tracking[7], dliom_cloud** out, float origin[3], int32_t* kept_index,
                                   int64_t capacity, int64_t* num_kept) {
  return assemble_from_sensor_points(ctx, traj, cloud_time, points_xyzt, nullptr, n, sensor_to_tracking, out, origin, kept_index,
                                     capacity, num_kept, nullptr, nullptr);
}

// the batch of either input: the points and intensities from the host, or a decoded message's in HBM
static int batch_from_points(dliom_ctx* ctx, dliom_trajectory* traj, int64_t cloud_time, const float* points_xyzt, const float* intensities,
                             const DevicePoints* device_points, int64_t n, const double sensor_to_tracking[7], dliom_points_batch** out) {
  if (out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  dliom_cloud* cloud = nullptr;
  float origin[3] = {0.f, 0.f, 0.f};
  int64_t kept = 0;
  AttrBlock kept_intensities;
  DLIOM_TRY(assemble_from_sensor_points(ctx, traj, cloud_time, points_xyzt, device_points, n, sensor_to_tracking, &cloud, origin, nullptr,
                                        0, &kept, intensities, &kept_intensities));
  if (cloud == nullptr) return DLIOM_OK;  // nothing kept: the reference returns nullptr
  dliom_points_batch* b = new dliom_points_batch;
  b->ctx = ctx;
  b->cloud = cloud;
  std::memcpy(b->origin, origin, 12);
  b->intensities = kept_intensities;
  *out = b;
  return DLIOM_OK;
}

int dliom_points_batch_from_sensor_points(dliom_ctx* ctx, dliom_trajectory* traj, int64_t cloud_time, const float* points_xyzt,
                                          const float* intensities, int64_t n, const double sensor_to_tracking[7],
                                          dliom_points_batch** out) {
  return batch_from_points(ctx, traj, cloud_time, points_xyzt, intensities, nullptr, n, sensor_to_tracking, out);
}

int dliom_points_batch_from_timed_cloud(dliom_ctx* ctx, dliom_trajectory* traj, int64_t cloud_time, const dliom_timed_cloud* points,
                                        const double sensor_to_tracking[7], dliom_points_batch** out) {
  if (ctx == nullptr || out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  DevicePoints d{nullptr, nullptr};
  int64_t n = 0;
  DLIOM_TRY(timed_cloud_view(points, ctx, &n, &d.xyzt, &d.intensities, nullptr));
  bool has_origin_index = false;
  DLIOM_TRY(timed_cloud_origin_index(points, &has_origin_index, nullptr));
  if (has_origin_index) return DLIOM_ERR_INVALID_ARGUMENT;  // two sensors' merged ranges: not a message's points
  return batch_from_points(ctx, traj, cloud_time, nullptr, nullptr, &d, n, sensor_to_tracking, out);
}

int dliom_assemble_check_stats(const dliom_ctx* ctx, int64_t* recorded, int64_t* recomputed, int64_t* fixed, int64_t* ring_overflows) {
  if (ctx == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  if (recorded != nullptr) *recorded = ctx->assemble_recorded;
  if (recomputed != nullptr) *recomputed = ctx->assemble_recomputed;
  if (fixed != nullptr) *fixed = ctx->assemble_fixed;
  if (ring_overflows != nullptr) *ring_overflows = ctx->assemble_overflows;
  return DLIOM_OK;
}

}  // extern "C"
