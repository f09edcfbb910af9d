// CPU model of the submap feature matching as include/dliom.h defines it ("submap feature matching"): plain C++17, one
// thread, no dependency but the header's constants and result structs.  Build with -ffp-contract=off.
//
//   feature_match_model <input> <output>
//
// Input (little endian), by its first int32:
//   0  nearest neighbours: int32 D, nq, nt; float q[nq * D], t[nt * D]
//      -> int32 j0[nq], j1[nq]; float d0[nq], d1[nq]
//   1  hypotheses and refit: int32 M; double threshold; uint64 seed; float from[2 M], to[2 M]
//      -> dliom_feature_ransac_result; double threshold_margin; uint8 mask[M]
//   2  match: int32 D, num_sets, query (index), num_train; dliom_feature_match_options; int32 train[num_train] (indices);
//      per set: int32 count, int32 0, double ox, oy, resolution, float descriptors[count * D], keypoints[count * 2]
//      -> dliom_submap_match[num_train] (key = the set's index); double ratio_margin, threshold_margin, seconds
// The margins say how far the case is from a knife's edge: ratio_margin is the least |d0 - r d1| / (r d1) over the
// queries of the matched pairs, threshold_margin the least |err^2 - thresh^2| / thresh^2 over every evaluated
// (hypothesis, match).
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "dliom.h"

namespace {

struct Reader {
  std::vector<unsigned char> data;
  size_t at = 0;
  template <class T>
  T get() {
    T v;
    if (at + sizeof(T) > data.size()) {
      std::fprintf(stderr, "feature_match_model: input too short\n");
      std::exit(2);
    }
    std::memcpy(&v, data.data() + at, sizeof(T));
    at += sizeof(T);
    return v;
  }
  template <class T>
  std::vector<T> many(size_t n) {
    std::vector<T> v(n);
    if (at + n * sizeof(T) > data.size()) {
      std::fprintf(stderr, "feature_match_model: input too short\n");
      std::exit(2);
    }
    if (n > 0) std::memcpy(v.data(), data.data() + at, n * sizeof(T));
    at += n * sizeof(T);
    return v;
  }
};

struct Writer {
  std::vector<unsigned char> data;
  template <class T>
  void put(const T& v) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(&v);
    data.insert(data.end(), p, p + sizeof(T));
  }
  template <class T>
  void many(const std::vector<T>& v) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    data.insert(data.end(), p, p + v.size() * sizeof(T));
  }
};

const double kInfinity = std::numeric_limits<double>::infinity();

// s(i, j) for four train descriptors at once (four independent chains, each in dimension order)
inline void distances4(const float* q, const float* t0, const float* t1, const float* t2, const float* t3, int D, float s[4]) {
  float a = 0.f, b = 0.f, c = 0.f, e = 0.f;
  for (int d = 0; d < D; ++d) {
    const float da = q[d] - t0[d], db = q[d] - t1[d], dc = q[d] - t2[d], de = q[d] - t3[d];
    a = std::fmaf(da, da, a);
    b = std::fmaf(db, db, b);
    c = std::fmaf(dc, dc, c);
    e = std::fmaf(de, de, e);
  }
  s[0] = a;
  s[1] = b;
  s[2] = c;
  s[3] = e;
}

void nearest_two(const float* q, int nq, const float* t, int nt, int D, std::vector<int32_t>* j0, std::vector<int32_t>* j1,
                 std::vector<float>* d0, std::vector<float>* d1) {
  j0->assign(nq, -1);
  j1->assign(nq, -1);
  d0->assign(nq, 0.f);
  d1->assign(nq, 0.f);
  std::vector<float> s(static_cast<size_t>(nt) + 4);
  for (int i = 0; i < nq; ++i) {
    const float* qi = q + static_cast<size_t>(i) * D;
    int j = 0;
    for (; j + 4 <= nt; j += 4)
      distances4(qi, t + static_cast<size_t>(j) * D, t + static_cast<size_t>(j + 1) * D, t + static_cast<size_t>(j + 2) * D,
                 t + static_cast<size_t>(j + 3) * D, D, &s[j]);
    for (; j < nt; ++j) {
      float acc = 0.f;
      for (int d = 0; d < D; ++d) {
        const float diff = qi[d] - t[static_cast<size_t>(j) * D + d];
        acc = std::fmaf(diff, diff, acc);
      }
      s[j] = acc;
    }
    // the least s, ties to the lowest j; then the same over j != nearest
    int best = 0;
    for (j = 1; j < nt; ++j)
      if (s[j] < s[best]) best = j;
    int second = best == 0 ? 1 : 0;
    for (j = 0; j < nt; ++j)
      if (j != best && s[j] < s[second]) second = j;
    (*j0)[i] = best;
    (*j1)[i] = second;
    (*d0)[i] = std::sqrt(s[best]);
    (*d1)[i] = std::sqrt(s[second]);
  }
}

struct Point {
  float px, py, Px, Py;  // from, to
};
struct Similarity {
  double a, b, tx, ty;
};

void hypothesis_matches(int M, bool enumerated, uint64_t seed, int h, int* i, int* j) {
  if (enumerated) {
    int count = 0;
    for (int a = 0; a < M; ++a)
      for (int b = a + 1; b < M; ++b, ++count)
        if (count == h) {
          *i = a;
          *j = b;
          return;
        }
    std::abort();
  }
  uint64_t z = seed + static_cast<uint64_t>(h);
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const uint32_t a = static_cast<uint32_t>(z) % static_cast<uint32_t>(M);
  uint32_t b = static_cast<uint32_t>(z >> 32) % static_cast<uint32_t>(M - 1);
  if (b >= a) ++b;
  *i = static_cast<int>(a);
  *j = static_cast<int>(b);
}

bool similarity_of(const Point& pi, const Point& pj, Similarity* m) {
  const double pix = pi.px, piy = pi.py, Pix = pi.Px, Piy = pi.Py;
  const double dx = static_cast<double>(pj.px) - pix, dy = static_cast<double>(pj.py) - piy;
  const double ex = static_cast<double>(pj.Px) - Pix, ey = static_cast<double>(pj.Py) - Piy;
  const double den = dx * dx + dy * dy;
  if (den == 0.0) return false;
  m->a = (dx * ex + dy * ey) / den;
  m->b = (dx * ey - dy * ex) / den;
  m->tx = Pix - (m->a * pix - m->b * piy);
  m->ty = Piy - (m->b * pix + m->a * piy);
  return true;
}

double squared_error(const Similarity& m, const Point& p) {
  const double px = p.px, py = p.py;
  const double rx = ((m.a * px - m.b * py) + m.tx) - static_cast<double>(p.Px);
  const double ry = ((m.b * px + m.a * py) + m.ty) - static_cast<double>(p.Py);
  return rx * rx + ry * ry;
}

// -> false: no model.  *margin is lowered to the least |err^2 - thresh^2| / thresh^2 met.
bool estimate(const std::vector<Point>& pts, double threshold, uint64_t seed, Similarity* model, int* inliers, int* hypothesis,
              int* num_hypotheses, std::vector<unsigned char>* mask, double* margin) {
  const int M = static_cast<int>(pts.size());
  const double t2 = threshold * threshold;
  mask->assign(M, 0);
  *inliers = 0;
  *hypothesis = -1;
  const long long all_pairs = static_cast<long long>(M) * (M - 1) / 2;
  const bool enumerated = all_pairs <= DLIOM_FEATURE_RANSAC_HYPOTHESES;
  *num_hypotheses = M < 2 ? 0 : static_cast<int>(enumerated ? all_pairs : DLIOM_FEATURE_RANSAC_HYPOTHESES);
  int best_count = -1;
  Similarity best{};
  for (int h = 0; h < *num_hypotheses; ++h) {
    int i, j;
    hypothesis_matches(M, enumerated, seed, h, &i, &j);
    Similarity m;
    if (!similarity_of(pts[i], pts[j], &m)) continue;  // scores -1
    int count = 0;
    for (int k = 0; k < M; ++k) {
      const double err = squared_error(m, pts[k]);
      count += err <= t2 ? 1 : 0;
      const double edge = std::abs(err - t2) / t2;
      if (edge < *margin) *margin = edge;
    }
    if (count > best_count) {  // ties to the lowest h
      best_count = count;
      best = m;
      *hypothesis = h;
    }
  }
  if (*hypothesis < 0) return false;
  int n = 0;
  double spx = 0.0, spy = 0.0, sPx = 0.0, sPy = 0.0;
  for (int k = 0; k < M; ++k) {
    if (!(squared_error(best, pts[k]) <= t2)) continue;
    (*mask)[k] = 1;
    ++n;
    spx += static_cast<double>(pts[k].px);
    spy += static_cast<double>(pts[k].py);
    sPx += static_cast<double>(pts[k].Px);
    sPy += static_cast<double>(pts[k].Py);
  }
  const double count = static_cast<double>(n);
  const double mpx = spx / count, mpy = spy / count, mPx = sPx / count, mPy = sPy / count;
  double sdd = 0.0, sde = 0.0, sx = 0.0;
  for (int k = 0; k < M; ++k) {
    if (!(*mask)[k]) continue;
    const double dcx = static_cast<double>(pts[k].px) - mpx, dcy = static_cast<double>(pts[k].py) - mpy;
    const double ecx = static_cast<double>(pts[k].Px) - mPx, ecy = static_cast<double>(pts[k].Py) - mPy;
    sdd += dcx * dcx + dcy * dcy;
    sde += dcx * ecx + dcy * ecy;
    sx += dcx * ecy - dcy * ecx;
  }
  if (sdd != 0.0) {
    best.a = sde / sdd;
    best.b = sx / sdd;
    best.tx = mPx - (best.a * mpx - best.b * mpy);
    best.ty = mPy - (best.b * mpx + best.a * mpy);
  }
  *model = best;
  *inliers = n;
  return true;
}

struct Set {
  int count;
  double ox, oy, resolution;
  std::vector<float> descriptors, keypoints;
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: feature_match_model <input> <output>\n");
    return 2;
  }
  Reader in;
  {
    FILE* f = std::fopen(argv[1], "rb");
    if (f == nullptr) return 2;
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    in.data.resize(static_cast<size_t>(size));
    if (size > 0 && std::fread(in.data.data(), 1, in.data.size(), f) != in.data.size()) return 2;
    std::fclose(f);
  }
  Writer out;
  const int mode = in.get<int32_t>();
  if (mode == 0) {
    const int D = in.get<int32_t>(), nq = in.get<int32_t>(), nt = in.get<int32_t>();
    const std::vector<float> q = in.many<float>(static_cast<size_t>(nq) * D), t = in.many<float>(static_cast<size_t>(nt) * D);
    std::vector<int32_t> j0, j1;
    std::vector<float> d0, d1;
    nearest_two(q.data(), nq, t.data(), nt, D, &j0, &j1, &d0, &d1);
    out.many(j0);
    out.many(j1);
    out.many(d0);
    out.many(d1);
  } else if (mode == 1) {
    const int M = in.get<int32_t>();
    const double threshold = in.get<double>();
    const uint64_t seed = in.get<uint64_t>();
    const std::vector<float> from = in.many<float>(2 * static_cast<size_t>(M)), to = in.many<float>(2 * static_cast<size_t>(M));
    std::vector<Point> pts(M);
    for (int k = 0; k < M; ++k) pts[k] = Point{from[2 * k], from[2 * k + 1], to[2 * k], to[2 * k + 1]};
    dliom_feature_ransac_result r;
    std::memset(&r, 0, sizeof(r));
    Similarity m{};
    std::vector<unsigned char> mask;
    double margin = kInfinity;
    const bool found = estimate(pts, threshold, seed, &m, &r.inliers, &r.hypothesis, &r.num_hypotheses, &mask, &margin);
    r.status = found ? DLIOM_FEATURE_MATCHED : DLIOM_FEATURE_NO_MODEL;
    if (found) {
      r.a = m.a;
      r.b = m.b;
      r.tx = m.tx;
      r.ty = m.ty;
      r.scale = std::sqrt(m.a * m.a + m.b * m.b);
      r.theta = std::atan2(m.b, m.a);
    } else {
      r.inliers = 0;
      r.hypothesis = -1;
    }
    out.put(r);
    out.put(margin);
    out.many(mask);
  } else if (mode == 2) {
    const int D = in.get<int32_t>(), num_sets = in.get<int32_t>(), query = in.get<int32_t>(), num_train = in.get<int32_t>();
    const dliom_feature_match_options options = in.get<dliom_feature_match_options>();
    const std::vector<int32_t> train = in.many<int32_t>(num_train);
    std::vector<Set> sets(num_sets);
    for (Set& s : sets) {
      s.count = in.get<int32_t>();
      (void)in.get<int32_t>();
      s.ox = in.get<double>();
      s.oy = in.get<double>();
      s.resolution = in.get<double>();
      s.descriptors = in.many<float>(static_cast<size_t>(s.count) * D);
      s.keypoints = in.many<float>(static_cast<size_t>(s.count) * 2);
    }
    const auto start = std::chrono::steady_clock::now();
    const Set& q = sets[query];
    const double r = options.good_match_ratio_of_distance;
    double ratio_margin = kInfinity, threshold_margin = kInfinity;
    std::vector<dliom_submap_match> results(num_train);
    for (int k = 0; k < num_train; ++k) {
      const Set& t = sets[train[k]];
      dliom_submap_match& o = results[k];
      std::memset(&o, 0, sizeof(o));
      o.key = train[k];
      o.hypothesis = -1;
      o.status = DLIOM_FEATURE_TOO_FEW_KEYPOINTS;
      if (q.count < 2 || t.count < 2) continue;
      std::vector<int32_t> j0, j1;
      std::vector<float> d0, d1;
      nearest_two(q.descriptors.data(), q.count, t.descriptors.data(), t.count, D, &j0, &j1, &d0, &d1);
      std::vector<Point> pts;
      for (int i = 0; i < q.count; ++i) {
        const double bound = r * static_cast<double>(d1[i]);
        const double edge = std::abs(static_cast<double>(d0[i]) - bound) / bound;
        if (edge < ratio_margin) ratio_margin = edge;
        if (!(static_cast<double>(d0[i]) < bound)) continue;
        const int j = j0[i];
        Point p;
        p.px = static_cast<float>(q.ox) + static_cast<float>(static_cast<double>(q.keypoints[2 * i]) * q.resolution);
        p.py = static_cast<float>(q.oy) + static_cast<float>(static_cast<double>(q.keypoints[2 * i + 1]) * q.resolution);
        p.Px = static_cast<float>(t.ox) + static_cast<float>(static_cast<double>(t.keypoints[2 * j]) * q.resolution);
        p.Py = static_cast<float>(t.oy) + static_cast<float>(static_cast<double>(t.keypoints[2 * j + 1]) * q.resolution);
        pts.push_back(p);
      }
      o.good_matches = static_cast<int>(pts.size());
      if (o.good_matches < options.minimum_good_match_num) {
        o.status = DLIOM_FEATURE_TOO_FEW_GOOD_MATCHES;
        continue;
      }
      if (o.good_matches > DLIOM_FEATURE_MAX_GOOD) {
        o.status = DLIOM_ERR_CAPACITY;
        continue;
      }
      Similarity m{};
      int inliers, hypothesis, num_hypotheses;
      std::vector<unsigned char> mask;
      if (!estimate(pts, options.ransac_threshold, options.seed, &m, &inliers, &hypothesis, &num_hypotheses, &mask,
                    &threshold_margin)) {
        o.status = DLIOM_FEATURE_NO_MODEL;
        continue;
      }
      o.inliers = inliers;
      o.hypothesis = hypothesis;
      o.a = m.a;
      o.b = m.b;
      o.tx = m.tx;
      o.ty = m.ty;
      o.scale = std::sqrt(m.a * m.a + m.b * m.b);
      o.theta = std::atan2(m.b, m.a);
      o.status = std::abs(o.scale - 1.0) > options.scale_estimated_tolerance ? DLIOM_FEATURE_SCALE_REJECTED : DLIOM_FEATURE_MATCHED;
    }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
    out.many(results);
    out.put(ratio_margin);
    out.put(threshold_margin);
    out.put(seconds);
  } else {
    std::fprintf(stderr, "feature_match_model: unknown mode %d\n", mode);
    return 2;
  }
  FILE* f = std::fopen(argv[2], "wb");
  if (f == nullptr) return 2;
  if (!out.data.empty() && std::fwrite(out.data.data(), 1, out.data.size(), f) != out.data.size()) return 2;
  std::fclose(f);
  return 0;
}
