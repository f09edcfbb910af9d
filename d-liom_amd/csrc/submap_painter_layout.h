// Host half of the submap painter (dliom.h "painting submap slices into one map"): Matrices, Layout, Inverse and Bound of
// the statement, the occupancy table and the sizing of the tile lists.  Plain C++17 with no HIP in it, so that
// tests/cpp/submap_painter_layout_check.cc can run it under sanitisers as a stand-alone program.  Compiled with
// -ffp-contract=off: every double operation below is one rounding, in the order written.
#ifndef DLIOM_CSRC_SUBMAP_PAINTER_LAYOUT_H_
#define DLIOM_CSRC_SUBMAP_PAINTER_LAYOUT_H_

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/dliom.h"
#include "host_math.h"

namespace dliom {
namespace painter {

constexpr int kPaddingPixel = 5;  // submap_painter.cc:85
constexpr int kTile = DLIOM_SUBMAP_PAINTER_TILE;

struct Matrix {  // cairo_matrix_t: x' = xx*x + xy*y + x0, y' = yx*x + yy*y + y0
  double xx, yx, xy, yy, x0, y0;
};
struct Fixed {  // the inverse in 32.32: U = A x + B y + E, V = C x + D y + G
  int64_t A, B, E, C, D, G;
};
struct Box {  // pixels [x0, x1] x [y0, y1] a slice can reach; x1 < x0: none
  int x0, y0, x1, y1;
};

inline bool finite7(const double* p) {
  for (int i = 0; i < 7; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

inline bool valid(const dliom_submap_slice_description& d) {
  return d.width >= 0 && d.height >= 0 && std::isfinite(d.resolution) && d.resolution > 0. && finite7(d.slice_pose7) &&
         finite7(d.pose7);
}

// Matrices: L of the statement
inline Matrix slice_matrix(const dliom_submap_slice_description& d, double resolution) {
  PoseD a, b;
  for (int i = 0; i < 3; ++i) a.t[i] = d.pose7[i], b.t[i] = d.slice_pose7[i];
  for (int i = 0; i < 4; ++i) a.q[i] = d.pose7[3 + i], b.q[i] = d.slice_pose7[3 + i];
  const PoseD P = pose_mul(a, b);
  const double w = P.q[0], x = P.q[1], y = P.q[2], z = P.q[3];
  const double tx = 2. * x, ty = 2. * y, tz = 2. * z;
  const double r00 = 1. - (ty * y + tz * z), r01 = ty * x - tz * w, r10 = ty * x + tz * w, r11 = 1. - (tx * x + tz * z);
  const double k = 1. / resolution, s = d.resolution;
  return Matrix{(r10 * k) * s, (r00 * k) * s, (-r11 * k) * s, (-r01 * k) * s, P.t[0] * k, -P.t[1] * k};
}

inline void apply(const Matrix& m, double x, double y, double* ox, double* oy) {
  *ox = (m.xx * x + m.xy * y) + m.x0;
  *oy = (m.yx * x + m.yy * y) + m.y0;
}

// Inverse and Bound: DLIOM_OK or DLIOM_ERR_TOO_LARGE
inline int invert(const Matrix& L, const float origin[2], int32_t width, int32_t height, Fixed* out) {
  Matrix F = L;
  F.x0 = L.x0 + static_cast<double>(origin[0]);
  F.y0 = L.y0 + static_cast<double>(origin[1]);
  const double det = F.xx * F.yy - F.yx * F.xy;
  const double inv[6] = {F.yy / det,  -F.xy / det, (F.xy * F.y0 - F.yy * F.x0) / det,
                         -F.yx / det, F.xx / det,  (F.yx * F.x0 - F.xx * F.y0) / det};
  for (double v : inv)
    if (!std::isfinite(v)) return DLIOM_ERR_TOO_LARGE;
  for (int r = 0; r < 2; ++r) {
    const double a = std::fabs(inv[3 * r]), b = std::fabs(inv[3 * r + 1]), e = std::fabs(inv[3 * r + 2]);
    if (!(a <= 1024.) || !(b <= 1024.)) return DLIOM_ERR_TOO_LARGE;
    if (!(a * width + b * height + e + 1. < 536870912.)) return DLIOM_ERR_TOO_LARGE;  // 2^29 texels
  }
  int64_t f[6];
  for (int i = 0; i < 6; ++i) f[i] = static_cast<int64_t>(std::nearbyint(inv[i] * 4294967296.));  // |.| < 2^61
  *out = Fixed{f[0], f[1], f[2], f[3], f[4], f[5]};
  return DLIOM_OK;
}

struct Layout {
  int32_t width = 0, height = 0;
  float origin[2] = {0.f, 0.f};
  std::vector<Matrix> matrices;  // L per slice
};

// Layout: DLIOM_OK, DLIOM_ERR_INVALID_ARGUMENT, DLIOM_ERR_TOO_LARGE, or DLIOM_ERR_CAPACITY with the sizes filled
inline int layout(const dliom_submap_slice_description* slices, int64_t n, double resolution, Layout* out) {
  if (slices == nullptr || n <= 0 || !std::isfinite(resolution) || !(resolution > 0.)) return DLIOM_ERR_INVALID_ARGUMENT;
  for (int64_t i = 0; i < n; ++i)
    if (!valid(slices[i])) return DLIOM_ERR_INVALID_ARGUMENT;
  out->matrices.resize(static_cast<size_t>(n));
  float lo[2] = {0.f, 0.f}, hi[2] = {0.f, 0.f};
  for (int64_t i = 0; i < n; ++i) {
    if (static_cast<int64_t>(slices[i].width) * slices[i].height > DLIOM_XRAY_MAX_PIXELS) return DLIOM_ERR_TOO_LARGE;
    const Matrix L = slice_matrix(slices[i], resolution);
    out->matrices[static_cast<size_t>(i)] = L;
    const double w = slices[i].width, h = slices[i].height;
    const double cx[4] = {0., w, 0., w}, cy[4] = {0., 0., h, h};
    for (int c = 0; c < 4; ++c) {
      double x, y;
      apply(L, cx[c], cy[c], &x, &y);
      const float p[2] = {static_cast<float>(x), static_cast<float>(y)};
      for (int a = 0; a < 2; ++a) {
        if (!std::isfinite(p[a])) return DLIOM_ERR_TOO_LARGE;
        if (i == 0 && c == 0) lo[a] = hi[a] = p[a];
        lo[a] = p[a] < lo[a] ? p[a] : lo[a];
        hi[a] = p[a] > hi[a] ? p[a] : hi[a];
      }
    }
  }
  int64_t size[2];
  for (int a = 0; a < 2; ++a) {
    const float extent = std::ceil(hi[a] - lo[a]);
    if (!(extent < 2147483000.f)) return DLIOM_ERR_TOO_LARGE;
    size[a] = static_cast<int64_t>(extent) + 2 * kPaddingPixel;
    out->origin[a] = -lo[a] + static_cast<float>(kPaddingPixel);
  }
  out->width = static_cast<int32_t>(size[0]);
  out->height = static_cast<int32_t>(size[1]);
  if (size[0] * size[1] > DLIOM_XRAY_MAX_PIXELS) return DLIOM_ERR_CAPACITY;
  return DLIOM_OK;
}

// The pixels a slice can reach.  Pixel (x, y) takes part only if one of its four texels lies in the slice, that is if its
// centre falls into the slice's rectangle grown by half a texel; the 32.32 rounding moves a sample by less than 2^-9 texel
// (x, y < 2^23).  So: the rectangle grown by a whole texel through F, in double, and one more pixel all round.
inline Box reach(const Matrix& L, const float origin[2], int32_t w, int32_t h, int32_t width, int32_t height) {
  if (w == 0 || h == 0) return Box{0, 0, -1, -1};
  Matrix F = L;
  F.x0 = L.x0 + static_cast<double>(origin[0]);
  F.y0 = L.y0 + static_cast<double>(origin[1]);
  const double cx[4] = {-1., w + 1., -1., w + 1.}, cy[4] = {-1., -1., h + 1., h + 1.};
  double lo[2] = {0., 0.}, hi[2] = {0., 0.};
  for (int c = 0; c < 4; ++c) {
    double p[2];
    apply(F, cx[c], cy[c], &p[0], &p[1]);
    for (int a = 0; a < 2; ++a) {
      if (c == 0) lo[a] = hi[a] = p[a];
      lo[a] = p[a] < lo[a] ? p[a] : lo[a];
      hi[a] = p[a] > hi[a] ? p[a] : hi[a];
    }
  }
  const int size[2] = {width, height};
  int b[4];
  for (int a = 0; a < 2; ++a) {
    const double l = std::floor(lo[a]) - 1., u = std::ceil(hi[a]) + 1.;
    b[a] = l < 0. ? 0 : (l > size[a] ? size[a] : static_cast<int>(l));
    b[2 + a] = u > size[a] - 1. ? size[a] - 1 : (u < -1. ? -1 : static_cast<int>(u));
  }
  if (b[2] < b[0] || b[3] < b[1]) return Box{0, 0, -1, -1};  // one spelling of `none`: the kernels' test and tile_pairs agree
  return Box{b[0], b[1], b[2], b[3]};
}

// (tile, slice) pairs of a paint: what the tile lists hold, known on the host without a read-back
inline int64_t tile_pairs(const Box* boxes, int64_t n) {
  int64_t pairs = 0;
  for (int64_t i = 0; i < n; ++i) {
    const Box& b = boxes[i];
    if (b.x1 < b.x0 || b.y1 < b.y0) continue;
    pairs += static_cast<int64_t>(b.x1 / kTile - b.x0 / kTile + 1) * (b.y1 / kTile - b.y0 / kTile + 1);
  }
  return pairs;
}

inline void occupancy_table(int8_t table[256]) {  // msg_conversion.cc:355-360
  for (int c = 0; c < 256; ++c) table[c] = static_cast<int8_t>(std::lround((1. - c / 255.) * 100.));
}

inline void occupancy_origin(const float origin[2], int32_t height, double resolution, double origin_xy[2]) {  // :339-342
  origin_xy[0] = static_cast<double>(-origin[0]) * resolution;
  origin_xy[1] = static_cast<double>(static_cast<float>(-height) + origin[1]) * resolution;
}

}  // namespace painter
}  // namespace dliom

#endif  // DLIOM_CSRC_SUBMAP_PAINTER_LAYOUT_H_
