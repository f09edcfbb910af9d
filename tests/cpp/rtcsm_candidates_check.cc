// The host prep of an RTCSM3D match (d-liom_amd/csrc/rtcsm_candidates.h) against the scalar functions of host_math.h it
// restates: rot[i], trans[j], t_norm and r_angle bit for bit, for random initial poses and windows with A = 1, 5 and 9;
// and the spreads of the box kernel's group table against the loop that took atan2 for every lane, bit for bit as well.
// Stand-alone: g++ -std=c++17 -O3 -ffp-contract=off (the library's host flags), and once more with
// -fsanitize=address,undefined.  One Candidates object serves every case, as a context's match state does, so the
// rotation table is rebuilt exactly when the window changes.  Prints "ok cases <n> rotations <sum of R> spreads <blocks>".
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../d-liom_amd/csrc/rtcsm_candidates.h"

using namespace dliom;

namespace {

// What rtcsm3d.hip's generate_candidates computed one rotation and one translation at a time.
struct Scalar {
  std::vector<QF> rot, raw;
  std::vector<float> r_angle;
  std::vector<F3> trans;
  std::vector<float> t_norm;
};
void scalar_candidates(const dliom_rtcsm_window& w, float resolution, const double init7[7], Scalar* s) {
  const F3 it{static_cast<float>(init7[0]), static_cast<float>(init7[1]), static_cast<float>(init7[2])};
  const QF iq{static_cast<float>(init7[3]), static_cast<float>(init7[4]), static_cast<float>(init7[5]),
              static_cast<float>(init7[6])};
  const int L = w.linear_window_size, A = w.angular_window_size;
  const float step = w.angular_step_size;
  s->rot.clear();
  s->raw.clear();
  s->r_angle.clear();
  s->trans.clear();
  s->t_norm.clear();
  for (int rz = -A; rz <= A; ++rz)
    for (int ry = -A; ry <= A; ++ry)
      for (int rx = -A; rx <= A; ++rx) {
        const QF q = angle_axis_to_quaternion(F3{rx * step, ry * step, rz * step});
        s->raw.push_back(q);
        s->r_angle.push_back(rotation_angle(q));
        s->rot.push_back(qnormalized(qmul(iq, q)));
      }
  for (int z = -L; z <= L; ++z)
    for (int y = -L; y <= L; ++y)
      for (int x = -L; x <= L; ++x) {
        const F3 t{x * resolution, y * resolution, z * resolution};
        s->t_norm.push_back(norm3(t));
        s->trans.push_back(add3(qrot(iq, t), it));
      }
}

bool same(const void* a, const void* b, size_t bytes) { return std::memcmp(a, b, bytes) == 0; }

// The spread of the rotations [r0, r0 + cnt) around their centre lane as rtcsm3d.hip's group table computed it: every lane
// normalised in double, atan2 for every lane.
void scalar_spread(const std::vector<QF>& raw, int r0, int cnt, RotationSpread* out) {
  auto qd = [&](int r, double q[4]) {
    const QF& f = raw[static_cast<size_t>(r)];
    const double nn = std::sqrt(double(f.w) * f.w + double(f.x) * f.x + double(f.y) * f.y + double(f.z) * f.z);
    q[0] = f.w / nn; q[1] = f.x / nn; q[2] = f.y / nn; q[3] = f.z / nn;
  };
  double qc[4];
  qd(r0 + cnt / 2, qc);
  double lo3[3] = {1e300, 1e300, 1e300}, hi3[3] = {-1e300, -1e300, -1e300}, th = 0.0;
  for (int l = 0; l < cnt; ++l) {
    double q[4];
    qd(r0 + l, q);
    const double a0 = qc[0], a1 = -qc[1], a2 = -qc[2], a3 = -qc[3];
    double dq[4] = {a0 * q[0] - a1 * q[1] - a2 * q[2] - a3 * q[3], a0 * q[1] + a1 * q[0] + a2 * q[3] - a3 * q[2],
                    a0 * q[2] - a1 * q[3] + a2 * q[0] + a3 * q[1], a0 * q[3] + a1 * q[2] - a2 * q[1] + a3 * q[0]};
    if (dq[0] < 0) for (double& v : dq) v = -v;
    const double vn = std::sqrt(dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3]);
    const double ang = 2.0 * std::atan2(vn, dq[0]);
    const double k = vn > 1e-300 ? ang / vn : 2.0;
    const double dv[3] = {k * dq[1], k * dq[2], k * dq[3]};
    th = std::max(th, ang);
    for (int a = 0; a < 3; ++a) {
      lo3[a] = std::min(lo3[a], dv[a]);
      hi3[a] = std::max(hi3[a], dv[a]);
    }
  }
  for (int a = 0; a < 3; ++a) {
    out->lo[a] = lo3[a];
    out->hi[a] = hi3[a];
  }
  out->max_angle = th;
}

int fail(int k, const char* what) {
  std::printf("case %d: %s differs\n", k, what);
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  const int cases = argc > 1 ? std::atoi(argv[1]) : 1000;
  std::mt19937 rng(20240521u);
  std::uniform_real_distribution<double> uni(-1.0, 1.0);
  std::normal_distribution<double> gauss(0.0, 1.0);
  Candidates c;  // one object for every case
  Scalar s;
  std::vector<char> tables;
  long long rotations = 0, spreads = 0;
  const int windows[3] = {1, 5, 9};
  for (int k = 0; k < cases; ++k) {
    const int A = windows[k % 3], L = 1 + (k / 3) % 2;
    const float resolution = (k / 6) % 2 == 0 ? 0.1f : 0.05f;
    const float max_norm = static_cast<float>(5.0 + 40.0 * (uni(rng) * 0.5 + 0.5));
    dliom_rtcsm_options o;
    std::memset(&o, 0, sizeof o);
    o.linear_search_window = (L + 0.25) * resolution;
    o.translation_delta_cost_weight = 0.1;
    o.rotation_delta_cost_weight = 0.1;
    dliom_rtcsm_window probe;
    o.angular_search_window = 1.0;
    compute_window(o, resolution, max_norm, &probe);
    o.angular_search_window = (A + 0.25) * static_cast<double>(probe.angular_step_size);
    double init7[7];
    for (int a = 0; a < 3; ++a) init7[a] = 30.0 * uni(rng);
    double q[4], n2 = 0.0;
    for (double& v : q) {
      v = gauss(rng);
      n2 += v * v;
    }
    // unit quaternions, every tenth case a little off unit length (what a caller's double pose leaves after the cast)
    const double scale = (k % 10 == 9 ? 1.0 + 1e-3 * uni(rng) : 1.0) / std::sqrt(n2);
    for (int a = 0; a < 4; ++a) init7[3 + a] = q[a] * scale;
    if (k % 97 == 96) init7[3] = init7[4] = init7[5] = init7[6] = 0.0;  // the zero quaternion: qnormalized's other branch

    generate_candidates(o, resolution, max_norm, init7, &c);
    if (c.w.angular_window_size != A || c.w.linear_window_size != L) return fail(k, "the window (test set-up)");
    scalar_candidates(c.w, resolution, init7, &s);
    const size_t R = s.rot.size(), T = s.trans.size();
    rotations += static_cast<long long>(R);
    if (c.num_rotations() != R || c.trans.size() != T || c.t_norm.size() != T) return fail(k, "a table's size");
    if (!same(c.r_angle.data(), s.r_angle.data(), R * 4)) return fail(k, "r_angle");
    if (!same(c.trans.data(), s.trans.data(), T * sizeof(F3))) return fail(k, "trans");
    if (!same(c.t_norm.data(), s.t_norm.data(), T * 4)) return fail(k, "t_norm");
    for (size_t r = 0; r < R; ++r) {
      const QF one = c.rot(r);
      if (!same(&one, &s.rot[r], sizeof(QF))) return fail(k, "rot(r)");
      // the box kernel's group table normalises q_r in double
      const QF f = s.raw[r];
      const double nn = std::sqrt(double(f.w) * f.w + double(f.x) * f.x + double(f.y) * f.y + double(f.z) * f.z);
      const double unit[4] = {f.w / nn, f.x / nn, f.y / nn, f.z / nn};
      if (c.unit_raw.size() != 4 * R || !same(&c.unit_raw[4 * r], unit, sizeof unit)) return fail(k, "unit_raw");
      const QF raw = c.rot_raw(r);
      if (!same(&raw, &f, sizeof(QF))) return fail(k, "rot_raw(r)");
    }
    // the group table's spreads: blocks of 256 rotations over the whole window, of 192 and of 64 over a shard of it, and
    // once a case one block over everything (relative angles far beyond the series' range when A = 9)
    const int Ri = static_cast<int>(R);
    const int shards[4][3] = {{0, Ri, 256}, {Ri / 3, Ri - Ri / 5, 192}, {Ri / 2, Ri, 64}, {0, Ri, Ri}};
    for (const auto& sh : shards)
      for (int r0 = sh[0]; r0 < sh[1]; r0 += sh[2]) {
        const int cnt = std::min(sh[2], sh[1] - r0);
        RotationSpread want, got;
        scalar_spread(s.raw, r0, cnt, &want);
        rotation_spread(c, r0, cnt, &got);
        ++spreads;
        if (!same(want.lo, got.lo, sizeof want.lo) || !same(want.hi, got.hi, sizeof want.hi) ||
            !same(&want.max_angle, &got.max_angle, sizeof(double)))
          return fail(k, "a block's spread");
      }
    // the tables as the kernels read them, canaries around
    const CandidateTableLayout l = candidate_table_layout(R, T);
    tables.assign(l.total + 32, static_cast<char>(0x5A));
    char* dst = tables.data() + 16;
    fill_candidate_tables(c, l, dst);
    for (size_t i = 0; i < 16; ++i)
      if (tables[i] != 0x5A || tables[16 + l.total + i] != 0x5A) return fail(k, "a byte outside the tables");
    if (!same(dst + l.rot, s.rot.data(), R * 16)) return fail(k, "the rotation table");
    if (!same(dst + l.t_norm, s.t_norm.data(), T * 4)) return fail(k, "the t_norm table");
    if (!same(dst + l.r_angle, s.r_angle.data(), R * 4)) return fail(k, "the r_angle table");
    for (size_t j = 0; j < T; ++j) {
      const float row4[4] = {s.trans[j].x, s.trans[j].y, s.trans[j].z, 0.f};
      if (!same(dst + l.trans + 12 * j, row4, 12)) return fail(k, "the translation table");
      if (!same(dst + l.trans4 + 16 * j, row4, 16)) return fail(k, "the 16-byte translation table");
    }
    const size_t ends[5][2] = {{l.rot + R * 16, l.trans}, {l.trans + T * 12, l.t_norm}, {l.t_norm + T * 4, l.r_angle},
                               {l.r_angle + R * 4, l.trans4}, {l.trans4 + T * 16, l.total}};
    for (const auto& e : ends)
      for (size_t i = e[0]; i < e[1]; ++i)
        if (dst[i] != 0) return fail(k, "a padding byte");
  }
  std::printf("ok cases %d rotations %lld spreads %lld\n", cases, rotations, spreads);
  return 0;
}
