// Host side of an RTCSM3D match's candidate tables: the search window, the (2A+1)^3 candidate rotations
// normalized(q_init * q_r) and the (2L+1)^3 candidate translations q_init * t_j + t_init, in the reference's float
// arithmetic (real_time_correlative_scan_matcher_3d.cc:55-95; candidate c = j * R + r in generation order z, y, x,
// rz, ry, rx).  Host code only (rtcsm3d.hip, tests/cpp/rtcsm_candidates_check.cc): no HIP, no context.
//
// This runs between the previous scan's last kernel and the match's first launch, with the GPU idle,
// so it does per match only what depends on the initial pose:
//  * the transform rotations q_r and their angles depend on the window alone: a Candidates object keeps them, one array
//    a component, while (A, step) stay what they were -- and since the step follows every scan's range, rebuilding them
//    takes sin / cos / atan2 for the (A + 1)^3 rotation vectors without a negative component only (generate_candidates);
//  * the R products normalized(q_init * q_r) are one loop over those arrays that the compiler vectorises -- every lane
//    the IEEE multiply / add / sqrt / divide sequence of host_math.h's qmul and qnormalized, without contraction -- and
//    go straight into the table the kernels read (compose_rotations); rot(r) gives the same bits for one rotation;
//  * fill_candidate_tables writes the tables where they are staged, not into a buffer to be copied there.
//  * rotation_spread, what the LDS-box kernel's group table is made of, takes atan2 for the few lanes that can decide it.
#ifndef DLIOM_CSRC_RTCSM_CANDIDATES_H_
#define DLIOM_CSRC_RTCSM_CANDIDATES_H_

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/dliom.h"
#include "host_math.h"

namespace dliom {

struct Candidates {
  dliom_rtcsm_window w;
  PoseF init;
  int table_A = -1;  // the window the rotation table below was made for
  float table_step = 0.f;
  std::vector<float> raw_w, raw_x, raw_y, raw_z;  // q_r (transform rotation), R entries each
  std::vector<float> r_angle;                      // GetAngle(transform) per rotation
  std::vector<QF> octant_q;                        // q_r and its angle for rx, ry, rz >= 0: what the table is made from
  std::vector<float> octant_angle;
  std::vector<double> octant_unit;                 // q_r / ||q_r|| in double, 4 an entry (w, x, y, z): see unit_raw
  std::vector<double> unit_raw;                    // the same for every rotation, 4 an entry (the box kernel's group table)
  std::vector<F3> trans;                           // candidate translation init.q * t_j + init.t
  std::vector<float> t_norm;                       // ||t_j||
  size_t num_rotations() const { return r_angle.size(); }
  QF rot_raw(size_t r) const { return QF{raw_w[r], raw_x[r], raw_y[r], raw_z[r]}; }
  QF rot(size_t r) const { return qnormalized(qmul(init.q, rot_raw(r))); }  // candidate rotation normalized(init.q * q_r)
};

// rtcsm_3d.cc:58-70
inline void compute_window(const dliom_rtcsm_options& o, float resolution, float cloud_max_norm_value,
                           dliom_rtcsm_window* w) {
  w->linear_window_size = static_cast<int>(std::lround(o.linear_search_window / resolution));
  float max_scan_range = 3.f * resolution;
  max_scan_range = std::max(cloud_max_norm_value, max_scan_range);
  const float kSafetyMargin = 1.f - 1e-3f;
  const float res2 = resolution * (resolution * 1.f);
  const float range2 = max_scan_range * (max_scan_range * 1.f);
  w->angular_step_size = kSafetyMargin * std::acos(1.f - res2 / (2.f * range2));
  w->angular_window_size =
      static_cast<int>(std::lround(o.angular_search_window / w->angular_step_size));
  w->max_scan_range = max_scan_range;
  const int64_t tl = 2 * static_cast<int64_t>(w->linear_window_size) + 1;
  const int64_t ta = 2 * static_cast<int64_t>(w->angular_window_size) + 1;
  w->num_translations = tl * tl * tl;
  w->num_rotations = ta * ta * ta;
  w->num_candidates = w->num_translations * w->num_rotations;
}

// out4[4 i ..] = qnormalized(qmul(a, (bw[i], bx[i], by[i], bz[i]))) as (w, x, y, z), i < n: host_math.h's two functions
// written as one loop over arrays, operation for operation.  The zero-norm branch of qnormalized is a select, so that
// nothing keeps the loop from four (or eight) rotations an instruction; contraction stays off whatever the file's flags.
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
inline void compose_rotations(const QF& a, const float* __restrict__ bw, const float* __restrict__ bx,
                              const float* __restrict__ by, const float* __restrict__ bz, size_t n, float* __restrict__ out4) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float aw = a.w, ax = a.x, ay = a.y, az = a.z;
  for (size_t i = 0; i < n; ++i) {
    const float x = (ax * bw[i] - az * by[i]) + (ay * bz[i] + aw * bx[i]);
    const float y = (ay * bw[i] - ax * bz[i]) + (az * bx[i] + aw * by[i]);
    const float z = (az * bw[i] - ay * bx[i]) + (ax * by[i] + aw * bz[i]);
    const float w = (aw * bw[i] - ax * bx[i]) - (az * bz[i] + ay * by[i]);
    const float z2 = (x * x + z * z) + (y * y + w * w);
    const float len = std::sqrt(z2);
    const bool scale = z2 > 0.f;
    out4[4 * i] = scale ? w / len : w;
    out4[4 * i + 1] = scale ? x / len : x;
    out4[4 * i + 2] = scale ? y / len : y;
    out4[4 * i + 3] = scale ? z / len : z;
  }
}

// The window, the initial pose, the rotation table (when the window changed) and the translations of a match.  A
// Candidates object that lives from match to match keeps its arrays' capacity: the steady state allocates nothing.
inline void generate_candidates(const dliom_rtcsm_options& o, float resolution, float max_norm, const double init7[7],
                                Candidates* c) {
  compute_window(o, resolution, max_norm, &c->w);
  c->init.t = F3{static_cast<float>(init7[0]), static_cast<float>(init7[1]), static_cast<float>(init7[2])};
  c->init.q = QF{static_cast<float>(init7[3]), static_cast<float>(init7[4]),
                 static_cast<float>(init7[5]), static_cast<float>(init7[6])};
  const int L = c->w.linear_window_size, A = c->w.angular_window_size;
  const float step = c->w.angular_step_size;
  if (c->table_A != A || c->table_step != step || c->r_angle.size() != static_cast<size_t>(c->w.num_rotations)) {
    c->table_A = -1;  // (not valid while it is being rebuilt: an exception below leaves it so)
    // The step follows the scan's range, so this runs for nearly every scan of a moving sensor.  angle_axis_to_quaternion
    // and rotation_angle see a rotation vector's components only through their squares (sqnorm3, norm3) and are linear in
    // them otherwise, and (-r) * step = -(r * step) exactly: sin, cos and atan2 are evaluated for the (A + 1)^3 vectors
    // (|rx|, |ry|, |rz|) * step, by the two functions themselves, and the other (2A + 1)^3 - (A + 1)^3 rotations are those
    // with signs put back -- the same bits as a call per rotation (tests/cpp/rtcsm_candidates_check.cc).
    const size_t A1 = static_cast<size_t>(A) + 1;
    c->octant_q.resize(A1 * A1 * A1);
    c->octant_angle.resize(A1 * A1 * A1);
    c->octant_unit.resize(4 * A1 * A1 * A1);
    c->unit_raw.resize(4 * static_cast<size_t>(c->w.num_rotations));
    for (int rz = 0; rz <= A; ++rz)
      for (int ry = 0; ry <= A; ++ry)
        for (int rx = 0; rx <= A; ++rx) {
          const size_t k = (static_cast<size_t>(rz) * A1 + ry) * A1 + rx;
          c->octant_q[k] = angle_axis_to_quaternion(F3{rx * step, ry * step, rz * step});
          c->octant_angle[k] = rotation_angle(c->octant_q[k]);
          const QF& f = c->octant_q[k];  // (a component's sign changes neither the norm nor, beyond its own, the quotient)
          const double nn = std::sqrt(double(f.w) * f.w + double(f.x) * f.x + double(f.y) * f.y + double(f.z) * f.z);
          const double unit[4] = {f.w / nn, f.x / nn, f.y / nn, f.z / nn};
          std::memcpy(&c->octant_unit[4 * k], unit, sizeof unit);
        }
    for (std::vector<float>* v : {&c->raw_w, &c->raw_x, &c->raw_y, &c->raw_z, &c->r_angle})
      v->resize(static_cast<size_t>(c->w.num_rotations));
    size_t r = 0;
    for (int rz = -A; rz <= A; ++rz)
      for (int ry = -A; ry <= A; ++ry)
        for (int rx = -A; rx <= A; ++rx, ++r) {
          const size_t k = (static_cast<size_t>(std::abs(rz)) * A1 + std::abs(ry)) * A1 + std::abs(rx);
          const QF& q = c->octant_q[k];
          c->raw_w[r] = q.w;
          c->raw_x[r] = rx < 0 ? -q.x : q.x;
          c->raw_y[r] = ry < 0 ? -q.y : q.y;
          c->raw_z[r] = rz < 0 ? -q.z : q.z;
          c->r_angle[r] = c->octant_angle[k];
          const double* u = &c->octant_unit[4 * k];
          double* out = &c->unit_raw[4 * r];
          out[0] = u[0];
          out[1] = rx < 0 ? -u[1] : u[1];
          out[2] = ry < 0 ? -u[2] : u[2];
          out[3] = rz < 0 ? -u[3] : u[3];
        }
    c->table_A = A;
    c->table_step = step;
  }
  c->trans.clear();
  c->t_norm.clear();
  for (int z = -L; z <= L; ++z)
    for (int y = -L; y <= L; ++y)
      for (int x = -L; x <= L; ++x) {
        const F3 t{x * resolution, y * resolution, z * resolution};
        c->t_norm.push_back(norm3(t));
        c->trans.push_back(add3(qrot(c->init.q, t), c->init.t));
      }
}

// Spread of `cnt` consecutive rotations [r0, r0 + cnt) of the table around their centre lane r0 + cnt / 2, in double: with
// d_l = conj(q_centre) * q_l (unit quaternions, d_l.w >= 0) and delta_l = (angle_l / |d_l.xyz|) d_l.xyz its rotation
// vector, the per-axis minimum `lo` and maximum `hi` of delta_l and the largest angle_l = 2 atan2(|d_l.xyz|, d_l.w) -- what
// the LDS-box kernel's group table is made of (rtcsm3d.hip).
//
// The step follows every scan's range, so this runs every match, and atan2 a lane was two thirds of it.  Only seven of the
// cnt lanes decide the result, so the angles are first taken from atan's series (|error| < 2.2e-12 for a tangent <= 0.2:
// the next term, t^15 / 15; lanes beyond it, or with d_l.xyz = 0, get atan2 at once), then every lane that can still hold
// an extreme within kSlack = 1e-9 relative -- fifty times the series' error, and the extreme's own lane is always among
// them -- is redone with atan2, and the extremes are taken over those exact values alone.  lo, hi and max_angle are thus
// the bits a loop with atan2 for every lane gives (tests/cpp/rtcsm_candidates_check.cc holds them against that loop).
struct RotationSpread {
  double lo[3], hi[3], max_angle;
};
inline void rotation_spread(const Candidates& c, int r0, int cnt, RotationSpread* out) {
  constexpr double kSlack = 1e-9, kSeriesMax = 0.2;
  static thread_local std::vector<double> scratch;
  scratch.resize(9 * static_cast<size_t>(cnt));
  double *d0 = scratch.data(), *d1 = d0 + cnt, *d2 = d1 + cnt, *d3 = d2 + cnt, *vn = d3 + cnt, *ang = vn + cnt;
  double *v1 = ang + cnt, *v2 = v1 + cnt, *v3 = v2 + cnt;  // the rotation vectors from the first angles
  const double* u = &c.unit_raw[4 * static_cast<size_t>(r0)];
  const double* qc = u + 4 * static_cast<size_t>(cnt / 2);
  const double a0 = qc[0], a1 = -qc[1], a2 = -qc[2], a3 = -qc[3];  // d = conj(qc) * q
  for (int l = 0; l < cnt; ++l) {
    const double* q = u + 4 * static_cast<size_t>(l);
    const double e0 = a0 * q[0] - a1 * q[1] - a2 * q[2] - a3 * q[3], e1 = a0 * q[1] + a1 * q[0] + a2 * q[3] - a3 * q[2];
    const double e2 = a0 * q[2] - a1 * q[3] + a2 * q[0] + a3 * q[1], e3 = a0 * q[3] + a1 * q[2] - a2 * q[1] + a3 * q[0];
    const bool flip = e0 < 0;
    d0[l] = flip ? -e0 : e0;
    d1[l] = flip ? -e1 : e1;
    d2[l] = flip ? -e2 : e2;
    d3[l] = flip ? -e3 : e3;
    vn[l] = std::sqrt(d1[l] * d1[l] + d2[l] * d2[l] + d3[l] * d3[l]);
  }
  const auto exact_angle = [&](int l) { return 2.0 * std::atan2(vn[l], d0[l]); };
  for (int l = 0; l < cnt; ++l) {  // (lanes the series does not cover hold garbage until the loop below)
    const double t = vn[l] / d0[l], s = t * t;
    ang[l] = 2.0 * (t * (1.0 + s * (-1.0 / 3 + s * (1.0 / 5 + s * (-1.0 / 7 + s * (1.0 / 9 + s * (-1.0 / 11 + s * (1.0 / 13))))))));
  }
  double low_of_hi[3] = {-1e300, -1e300, -1e300}, high_of_lo[3] = {1e300, 1e300, 1e300}, low_of_angle = 0.0;
  for (int l = 0; l < cnt; ++l) {
    if (!(vn[l] > 1e-300 && vn[l] <= kSeriesMax * d0[l])) ang[l] = exact_angle(l);
    const double k = vn[l] > 1e-300 ? ang[l] / vn[l] : 2.0;
    v1[l] = k * d1[l];
    v2[l] = k * d2[l];
    v3[l] = k * d3[l];
    const double v[3] = {v1[l], v2[l], v3[l]};
    for (int a = 0; a < 3; ++a) {
      const double slack = std::fabs(v[a]) * kSlack;
      low_of_hi[a] = std::max(low_of_hi[a], v[a] - slack);
      high_of_lo[a] = std::min(high_of_lo[a], v[a] + slack);
    }
    low_of_angle = std::max(low_of_angle, ang[l] * (1.0 - kSlack));
  }
  for (int a = 0; a < 3; ++a) {
    out->lo[a] = 1e300;
    out->hi[a] = -1e300;
  }
  out->max_angle = 0.0;
  for (int l = 0; l < cnt; ++l) {
    const double v[3] = {v1[l], v2[l], v3[l]};
    bool decides = ang[l] * (1.0 + kSlack) >= low_of_angle;
    for (int a = 0; a < 3; ++a) {
      const double slack = std::fabs(v[a]) * kSlack;
      decides = decides || v[a] + slack >= low_of_hi[a] || v[a] - slack <= high_of_lo[a];
    }
    if (!decides) continue;
    const double angle = exact_angle(l);
    const double k = vn[l] > 1e-300 ? angle / vn[l] : 2.0;
    const double dv[3] = {k * d1[l], k * d2[l], k * d3[l]};
    out->max_angle = std::max(out->max_angle, angle);
    for (int a = 0; a < 3; ++a) {
      out->lo[a] = std::min(out->lo[a], dv[a]);
      out->hi[a] = std::max(out->hi[a], dv[a]);
    }
  }
}

// Where the tables of a match lie in the block the kernels read: [rot R x 16 | trans T x 12 | t_norm T x 4 |
// r_angle R x 4 | trans4 T x 16], every part on a multiple of 256 bytes.
struct CandidateTableLayout {
  size_t rot = 0, trans = 0, t_norm = 0, r_angle = 0, trans4 = 0, total = 0;
};
inline CandidateTableLayout candidate_table_layout(size_t R, size_t T) {
  const auto up = [](size_t bytes) { return (bytes + 255) & ~static_cast<size_t>(255); };
  CandidateTableLayout l;
  l.trans = l.rot + up(R * 16);
  l.t_norm = l.trans + up(T * 12);
  l.r_angle = l.t_norm + up(T * 4);
  l.trans4 = l.r_angle + up(R * 4);
  l.total = l.trans4 + up(T * 16);
  return l;
}

// Writes the tables into `dst` (l.total bytes, 16-byte aligned; the bytes between the parts are zeroed).
inline void fill_candidate_tables(const Candidates& c, const CandidateTableLayout& l, char* dst) {
  const size_t R = c.num_rotations(), T = c.trans.size();
  const auto pad = [dst](size_t from, size_t to) { std::memset(dst + from, 0, to - from); };
  compose_rotations(c.init.q, c.raw_w.data(), c.raw_x.data(), c.raw_y.data(), c.raw_z.data(), R,
                    reinterpret_cast<float*>(dst + l.rot));
  pad(l.rot + R * 16, l.trans);
  float* ht = reinterpret_cast<float*>(dst + l.trans);
  float* h4 = reinterpret_cast<float*>(dst + l.trans4);
  for (size_t i = 0; i < T; ++i) {
    const F3& t = c.trans[i];
    ht[3 * i] = t.x;
    ht[3 * i + 1] = t.y;
    ht[3 * i + 2] = t.z;
    h4[4 * i] = t.x;
    h4[4 * i + 1] = t.y;
    h4[4 * i + 2] = t.z;
    h4[4 * i + 3] = 0.f;
  }
  pad(l.trans + T * 12, l.t_norm);
  std::memcpy(dst + l.t_norm, c.t_norm.data(), T * 4);
  pad(l.t_norm + T * 4, l.r_angle);
  std::memcpy(dst + l.r_angle, c.r_angle.data(), R * 4);
  pad(l.r_angle + R * 4, l.trans4);
  pad(l.trans4 + T * 16, l.total);
}

}  // namespace dliom

#endif  // DLIOM_CSRC_RTCSM_CANDIDATES_H_
