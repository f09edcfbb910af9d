// CPU model of dliom.h "submap image features": a plain single-threaded restatement of the header's nine steps, the
// reference the device (csrc/surf.hip) is pinned to bit for bit.  Build with -ffp-contract=off (tests/surf_common.py).
//
//   surf_model <input> <output>
// input: int32 mode, then
//   0  W H threshold k | W*H bytes                       -> W*H bytes (step 1)
//   1  W H octave layer | W*H bytes                      -> int32 rows cols | rows*cols float det | rows*cols float trace
//   2  W H threshold k n_octaves n_octave_layers | double hessian_threshold | W*H bytes
//                                                        -> int32 count status | count*7 float | count*64 float (steps 1-8)
//   3  W H | W*H bytes                                   -> (H+1)*(W+1) int32 (step 2)
//   4  N | N*2 float (y, x)                              -> N float (fastAtan2)
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dliom.h"

namespace {

typedef std::vector<uint8_t> Image;

int round_even(float v) { return static_cast<int>(rintf(v)); }  // the default rounding mode: half to even

// ---- step 1 --------------------------------------------------------------------------------------------------------
Image binarize_erode(const Image& in, int W, int H, int threshold, int k) {
  Image bin(in.size()), out(in.size());
  for (size_t i = 0; i < in.size(); ++i) bin[i] = in[i] > threshold ? 255 : 0;
  const int a = k / 2;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      int m = 255;
      for (int dy = 0; dy < k; ++dy)
        for (int dx = 0; dx < k; ++dx) {
          const int yy = y + dy - a, xx = x + dx - a;
          if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
          m = std::min<int>(m, bin[static_cast<size_t>(yy) * W + xx]);
        }
      out[static_cast<size_t>(y) * W + x] = static_cast<uint8_t>(m);
    }
  return out;
}

// ---- step 2 --------------------------------------------------------------------------------------------------------
struct Integral {
  int W = 0, H = 0;  // of the image; the table is (H + 1) x (W + 1)
  std::vector<int32_t> s;
  int32_t at(int y, int x) const { return s[static_cast<size_t>(y) * (W + 1) + x]; }
};

Integral integral_of(const Image& img, int W, int H) {
  Integral I;
  I.W = W;
  I.H = H;
  I.s.assign(static_cast<size_t>(H + 1) * (W + 1), 0);
  for (int y = 0; y < H; ++y) {
    int32_t row = 0;
    for (int x = 0; x < W; ++x) {
      row += img[static_cast<size_t>(y) * W + x];
      I.s[static_cast<size_t>(y + 1) * (W + 1) + x + 1] = I.at(y, x + 1) + row;
    }
  }
  return I;
}

// ---- templates -----------------------------------------------------------------------------------------------------
struct Box {
  int x1, y1, x2, y2;
  float w;
};
const int kDxx[3][5] = DLIOM_SURF_TEMPLATE_DXX;
const int kDyy[3][5] = DLIOM_SURF_TEMPLATE_DYY;
const int kDxy[4][5] = DLIOM_SURF_TEMPLATE_DXY;
const int kWaveX[2][5] = DLIOM_SURF_WAVELET_X;
const int kWaveY[2][5] = DLIOM_SURF_WAVELET_Y;

void resize_template(const int (*src)[5], int n, int old_size, int new_size, Box* dst) {
  const float ratio = static_cast<float>(new_size) / static_cast<float>(old_size);
  for (int k = 0; k < n; ++k) {
    Box b;
    b.x1 = round_even(ratio * static_cast<float>(src[k][0]));
    b.y1 = round_even(ratio * static_cast<float>(src[k][1]));
    b.x2 = round_even(ratio * static_cast<float>(src[k][2]));
    b.y2 = round_even(ratio * static_cast<float>(src[k][3]));
    b.w = static_cast<float>(src[k][4]) / static_cast<float>((b.x2 - b.x1) * (b.y2 - b.y1));
    dst[k] = b;
  }
}

float response(const Integral& I, int x0, int y0, const Box* boxes, int n) {
  float r = 0.f;
  for (int k = 0; k < n; ++k) {
    const Box& b = boxes[k];
    const uint32_t sum = static_cast<uint32_t>(I.at(y0 + b.y1, x0 + b.x1)) + static_cast<uint32_t>(I.at(y0 + b.y2, x0 + b.x2)) -
                         static_cast<uint32_t>(I.at(y0 + b.y2, x0 + b.x1)) - static_cast<uint32_t>(I.at(y0 + b.y1, x0 + b.x2));
    r = r + static_cast<float>(static_cast<int32_t>(sum)) * b.w;
  }
  return r;
}

// ---- step 3 --------------------------------------------------------------------------------------------------------
struct Layer {
  int size = 0, step = 1, rows = 0, cols = 0;
  std::vector<float> det, trace;
};

Layer make_layer(const Integral& I, int octave, int layer) {
  Layer L;
  L.size = (DLIOM_SURF_SIZE0 + DLIOM_SURF_SIZE_INCREMENT * layer) << octave;
  L.step = 1 << octave;
  L.rows = I.H / L.step;
  L.cols = I.W / L.step;
  L.det.assign(static_cast<size_t>(L.rows) * L.cols, 0.f);
  L.trace.assign(static_cast<size_t>(L.rows) * L.cols, 0.f);
  if (L.size > I.H || L.size > I.W) return L;
  Box dxx[3], dyy[3], dxy[4];
  resize_template(kDxx, 3, 9, L.size, dxx);
  resize_template(kDyy, 3, 9, L.size, dyy);
  resize_template(kDxy, 4, 9, L.size, dxy);
  const int samples_i = 1 + (I.H - L.size) / L.step, samples_j = 1 + (I.W - L.size) / L.step, offset = (L.size / 2) / L.step;
  for (int i = 0; i < samples_i; ++i)
    for (int j = 0; j < samples_j; ++j) {
      const float dx = response(I, j * L.step, i * L.step, dxx, 3);
      const float dy = response(I, j * L.step, i * L.step, dyy, 3);
      const float dc = response(I, j * L.step, i * L.step, dxy, 4);
      const size_t at = static_cast<size_t>(i + offset) * L.cols + (j + offset);
      L.det[at] = dx * dy - (0.81f * dc) * dc;
      L.trace[at] = dx + dy;
    }
  return L;
}

// ---- steps 4 and 5 -------------------------------------------------------------------------------------------------
struct KeyPoint {
  float x, y, size, angle, response, octave, sign;
  uint64_t order;  // (~response bits) << 32 | generation index
  float cos_dir = 0.f, sin_dir = 0.f;
};

bool refine(const Layer& below, const Layer& mid, const Layer& above, int i, int j, float* offset) {
  const Layer* Ls[3] = {&below, &mid, &above};
  auto N = [&](int s, int r, int c) { return Ls[s + 1]->det[static_cast<size_t>(i + r) * mid.cols + (j + c)]; };
  const float v = N(0, 0, 0);
  const float bx = -((N(0, 0, 1) - N(0, 0, -1)) * 0.5f), by = -((N(0, 1, 0) - N(0, -1, 0)) * 0.5f),
              bs = -((N(1, 0, 0) - N(-1, 0, 0)) * 0.5f);
  const float axx = (N(0, 0, -1) - 2.f * v) + N(0, 0, 1), ayy = (N(0, -1, 0) - 2.f * v) + N(0, 1, 0),
              ass = (N(-1, 0, 0) - 2.f * v) + N(1, 0, 0);
  const float axy = (((N(0, 1, 1) - N(0, 1, -1)) - N(0, -1, 1)) + N(0, -1, -1)) * 0.25f;
  const float axs = (((N(1, 0, 1) - N(1, 0, -1)) - N(-1, 0, 1)) + N(-1, 0, -1)) * 0.25f;
  const float ays = (((N(1, 1, 0) - N(1, -1, 0)) - N(-1, 1, 0)) + N(-1, -1, 0)) * 0.25f;
  const double a = axx, b = axy, c = axs, d = ayy, e = ays, f = ass, p = bx, q = by, r = bs;
  const double c00 = d * f - e * e, c01 = b * f - c * e, c02 = b * e - c * d;
  const double det = (a * c00 - b * c01) + c * c02;
  if (det == 0.0) return false;
  const double qfer = q * f - e * r, qedr = q * e - d * r, brqc = b * r - q * c;
  const double x0 = ((p * c00 - b * qfer) + c * qedr) / det;
  const double x1 = ((a * qfer - p * c01) + c * brqc) / det;
  const double x2 = ((a * (d * r - q * e) - b * brqc) + p * c02) / det;
  offset[0] = static_cast<float>(x0);
  offset[1] = static_cast<float>(x1);
  offset[2] = static_cast<float>(x2);
  return (offset[0] != 0.f || offset[1] != 0.f || offset[2] != 0.f) && std::fabs(offset[0]) <= 1.f && std::fabs(offset[1]) <= 1.f &&
         std::fabs(offset[2]) <= 1.f;
}

std::vector<KeyPoint> detect(const Integral& I, float threshold, int n_octaves, int n_layers) {
  std::vector<KeyPoint> kps;
  for (int o = 0; o < n_octaves; ++o) {
    std::vector<Layer> layers;
    for (int l = 0; l < n_layers + 2; ++l) layers.push_back(make_layer(I, o, l));
    for (int l = 1; l <= n_layers; ++l) {
      const Layer& L = layers[l];
      const int margin = (layers[l + 1].size / 2) / L.step + 1;
      for (int i = margin; i < L.rows - margin; ++i)
        for (int j = margin; j < L.cols - margin; ++j) {
          const float v = L.det[static_cast<size_t>(i) * L.cols + j];
          if (!(v > threshold)) continue;
          bool greatest = true;
          for (int s = -1; s <= 1 && greatest; ++s)
            for (int r = -1; r <= 1 && greatest; ++r)
              for (int c = -1; c <= 1; ++c) {
                if (s == 0 && r == 0 && c == 0) continue;
                if (!(v > layers[l + s].det[static_cast<size_t>(i + r) * L.cols + (j + c)])) {
                  greatest = false;
                  break;
                }
              }
          if (!greatest) continue;
          float off[3];
          if (!refine(layers[l - 1], L, layers[l + 1], i, j, off)) continue;
          const int sum_i = L.step * (i - (L.size / 2) / L.step), sum_j = L.step * (j - (L.size / 2) / L.step);
          const float centre = static_cast<float>(L.size - 1) * 0.5f;
          KeyPoint k;
          k.x = (static_cast<float>(sum_j) + centre) + off[0] * static_cast<float>(L.step);
          k.y = (static_cast<float>(sum_i) + centre) + off[1] * static_cast<float>(L.step);
          k.size = static_cast<float>(round_even(static_cast<float>(L.size) + off[2] * static_cast<float>(L.size - layers[l - 1].size)));
          k.angle = -1.f;
          k.response = v;
          k.octave = static_cast<float>(o);
          const float t = L.trace[static_cast<size_t>(i) * L.cols + j];
          k.sign = static_cast<float>((t > 0.f) - (t < 0.f));
          uint32_t bits;
          std::memcpy(&bits, &v, 4);
          const uint32_t generation = (static_cast<uint32_t>(o) << 25) | (static_cast<uint32_t>(l) << 23) |
                                      static_cast<uint32_t>(i * L.cols + j);
          k.order = (static_cast<uint64_t>(~bits) << 32) | generation;
          kps.push_back(k);
        }
    }
  }
  std::sort(kps.begin(), kps.end(), [](const KeyPoint& a, const KeyPoint& b) { return a.order < b.order; });
  return kps;
}

// ---- step 6 --------------------------------------------------------------------------------------------------------
float fast_atan2(float y, float x) {
  const float scale = static_cast<float>(180.0 / 3.14159265358979323846);
  const float p1 = 0.9997878412794807f * scale, p3 = -0.3258083974640975f * scale, p5 = 0.1555786518463281f * scale,
              p7 = -0.04432655554792128f * scale;
  const float ax = std::fabs(x), ay = std::fabs(y);
  const float c = std::min(ax, ay) / (std::max(ax, ay) + static_cast<float>(DBL_EPSILON));
  const float c2 = c * c;
  float a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  if (ax < ay) a = 90.f - a;
  if (x < 0.f) a = 180.f - a;
  if (y < 0.f) a = 360.f - a;
  return a;
}

// t_i = exp(-x_i^2 / (2 sigma^2)), x_i = i - (n - 1) / 2, in double with libm; g_i = (float)(t_i / sum t)
std::vector<float> gaussian_table(int n, double sigma) {
  std::vector<double> t(n);
  double sum = 0.0;
  for (int i = 0; i < n; ++i) {
    const double x = i - (n - 1) * 0.5;
    t[i] = std::exp(-(x * x) / (2.0 * sigma * sigma));
    sum += t[i];
  }
  std::vector<float> g(n);
  for (int i = 0; i < n; ++i) g[i] = static_cast<float>(t[i] / sum);
  return g;
}

// false: the key point is dropped
bool orient(const Integral& I, KeyPoint* k) {
  static const std::vector<float> g = gaussian_table(2 * DLIOM_SURF_ORI_RADIUS + 1, DLIOM_SURF_ORI_SIGMA);
  const float s = k->size * 1.2f / 9.0f;
  const int side = 2 * round_even(2.f * s);
  if (I.H + 1 < side || I.W + 1 < side) return false;
  Box wx[2], wy[2];
  resize_template(kWaveX, 2, 4, side, wx);
  resize_template(kWaveY, 2, 4, side, wy);
  const float half = static_cast<float>(side - 1) / 2.f;
  float X[DLIOM_SURF_ORI_SAMPLES], Y[DLIOM_SURF_ORI_SAMPLES];
  int A[DLIOM_SURF_ORI_SAMPLES];
  int n = 0;
  const int R = DLIOM_SURF_ORI_RADIUS;
  for (int i = -R; i <= R; ++i)
    for (int j = -R; j <= R; ++j) {
      if (i * i + j * j > R * R) continue;
      const float weight = g[i + R] * g[j + R];
      const int x = round_even((k->x + static_cast<float>(i) * s) - half);
      const int y = round_even((k->y + static_cast<float>(j) * s) - half);
      if (y < 0 || y >= I.H + 1 - side || x < 0 || x >= I.W + 1 - side) continue;
      X[n] = response(I, x, y, wx, 2) * weight;
      Y[n] = response(I, x, y, wy, 2) * weight;
      A[n] = round_even(fast_atan2(Y[n], X[n]));
      ++n;
    }
  if (n == 0) return false;
  float bestx = 0.f, besty = 0.f, best = 0.f;
  for (int w = 0; w < 360; w += 5) {
    float sumx = 0.f, sumy = 0.f;
    for (int m = 0; m < n; ++m) {
      const int d = std::abs(A[m] - w);
      if (d < 30 || d > 330) {
        sumx = sumx + X[m];
        sumy = sumy + Y[m];
      }
    }
    const float mod = sumx * sumx + sumy * sumy;
    if (mod > best) {
      best = mod;
      bestx = sumx;
      besty = sumy;
    }
  }
  const float norm = sqrtf(bestx * bestx + besty * besty);
  if (norm == 0.f) return false;
  k->angle = fast_atan2(-besty, bestx);
  k->cos_dir = bestx / norm;
  k->sin_dir = besty / norm;
  return true;
}

// ---- step 7 --------------------------------------------------------------------------------------------------------
void describe(const Image& img, int W, int H, const KeyPoint& k, float* out) {
  static const std::vector<float> g = gaussian_table(DLIOM_SURF_PATCH, DLIOM_SURF_DESCRIPTOR_SIGMA);
  const int P = DLIOM_SURF_PATCH + 1;  // 21
  const float s = k.size * 1.2f / 9.0f;
  const int w = static_cast<int>(static_cast<float>(P) * s);
  const float win_offset = -(static_cast<float>(w - 1) / 2.f);
  const float c = k.cos_dir, sn = k.sin_dir;
  const float start_x = (k.x + win_offset * c) + win_offset * sn;
  const float start_y = (k.y - win_offset * sn) + win_offset * c;
  auto window = [&](int i, int j) -> int {
    const float px = (start_x + static_cast<float>(i) * sn) + static_cast<float>(j) * c;
    const float py = (start_y + static_cast<float>(i) * c) - static_cast<float>(j) * sn;
    const int x = std::min(std::max(round_even(px), 0), W - 1), y = std::min(std::max(round_even(py), 0), H - 1);
    return img[static_cast<size_t>(y) * W + x];
  };
  int patch[DLIOM_SURF_PATCH + 1][DLIOM_SURF_PATCH + 1];
  for (int pi = 0; pi < P; ++pi)
    for (int pj = 0; pj < P; ++pj) {
      int64_t sum = 0;
      for (int ki = (w * pi) / P; ki * P < w * (pi + 1); ++ki) {
        const int oi = std::min(P * ki + P, w * (pi + 1)) - std::max(P * ki, w * pi);
        for (int kj = (w * pj) / P; kj * P < w * (pj + 1); ++kj) {
          const int oj = std::min(P * kj + P, w * (pj + 1)) - std::max(P * kj, w * pj);
          sum += static_cast<int64_t>(oi) * oj * window(ki, kj);
        }
      }
      patch[pi][pj] = static_cast<int>((2 * sum + static_cast<int64_t>(w) * w) / (2 * static_cast<int64_t>(w) * w));
    }
  const int Q = DLIOM_SURF_PATCH;  // 20
  float DX[DLIOM_SURF_PATCH][DLIOM_SURF_PATCH], DY[DLIOM_SURF_PATCH][DLIOM_SURF_PATCH];
  for (int i = 0; i < Q; ++i)
    for (int j = 0; j < Q; ++j) {
      const float dw = g[i] * g[j];
      DX[i][j] = static_cast<float>(patch[i][j + 1] - patch[i][j] + patch[i + 1][j + 1] - patch[i + 1][j]) * dw;
      DY[i][j] = static_cast<float>(patch[i + 1][j] - patch[i][j] + patch[i + 1][j + 1] - patch[i][j + 1]) * dw;
    }
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      for (int y = i * 5; y < i * 5 + 5; ++y)
        for (int x = j * 5; x < j * 5 + 5; ++x) {
          v[0] = v[0] + DX[y][x];
          v[1] = v[1] + DY[y][x];
          v[2] = v[2] + std::fabs(DX[y][x]);
          v[3] = v[3] + std::fabs(DY[y][x]);
        }
      for (int m = 0; m < 4; ++m) out[(i * 4 + j) * 4 + m] = v[m];
    }
  float sum = 0.f;
  for (int m = 0; m < 64; ++m) sum = sum + out[m] * out[m];
  const float scale = 1.f / (sqrtf(sum) + static_cast<float>(DBL_EPSILON));
  for (int m = 0; m < 64; ++m) out[m] = out[m] * scale;
}

// ---- files ---------------------------------------------------------------------------------------------------------
std::vector<char> read_file(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (f == nullptr) std::exit(2);
  std::vector<char> data;
  char buf[65536];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + n);
  std::fclose(f);
  return data;
}

struct Reader {
  const std::vector<char>& d;
  size_t at = 0;
  template <class T>
  T get() {
    if (at + sizeof(T) > d.size()) std::exit(3);
    T v;
    std::memcpy(&v, d.data() + at, sizeof(T));
    at += sizeof(T);
    return v;
  }
  Image image(int W, int H) {
    const size_t n = static_cast<size_t>(W) * H;
    if (W < 0 || H < 0 || at + n > d.size()) std::exit(3);
    Image img(d.begin() + at, d.begin() + at + n);
    at += n;
    return img;
  }
};

template <class T>
void put(std::FILE* f, const T* v, size_t n) {
  if (n > 0 && std::fwrite(v, sizeof(T), n, f) != n) std::exit(4);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: surf_model <input> <output>\n");
    return 1;
  }
  const std::vector<char> data = read_file(argv[1]);
  Reader in{data};
  std::FILE* out = std::fopen(argv[2], "wb");
  if (out == nullptr) return 2;
  const int mode = in.get<int32_t>();
  if (mode == 0) {
    const int W = in.get<int32_t>(), H = in.get<int32_t>(), threshold = in.get<int32_t>(), k = in.get<int32_t>();
    const Image r = binarize_erode(in.image(W, H), W, H, threshold, k);
    put(out, r.data(), r.size());
  } else if (mode == 1) {
    const int W = in.get<int32_t>(), H = in.get<int32_t>(), octave = in.get<int32_t>(), layer = in.get<int32_t>();
    const Layer L = make_layer(integral_of(in.image(W, H), W, H), octave, layer);
    const int32_t dims[2] = {L.rows, L.cols};
    put(out, dims, 2);
    put(out, L.det.data(), L.det.size());
    put(out, L.trace.data(), L.trace.size());
  } else if (mode == 2) {
    const int W = in.get<int32_t>(), H = in.get<int32_t>(), threshold = in.get<int32_t>(), k = in.get<int32_t>();
    const int n_octaves = in.get<int32_t>(), n_layers = in.get<int32_t>();
    const double hessian = in.get<double>();
    const Image img = binarize_erode(in.image(W, H), W, H, threshold, k);
    const Integral I = integral_of(img, W, H);
    std::vector<KeyPoint> kps = detect(I, static_cast<float>(hessian), n_octaves, n_layers);
    int32_t head[2] = {0, DLIOM_OK};
    std::vector<float> records, descriptors;
    if (kps.size() > DLIOM_SURF_MAX_KEYPOINTS) {
      head[0] = static_cast<int32_t>(kps.size());
      head[1] = DLIOM_ERR_CAPACITY;
    } else {
      for (KeyPoint& k : kps) {
        if (!orient(I, &k)) continue;
        const float rec[7] = {k.x, k.y, k.size, k.angle, k.response, k.octave, k.sign};
        records.insert(records.end(), rec, rec + 7);
        descriptors.resize(descriptors.size() + 64);
        describe(img, W, H, k, descriptors.data() + descriptors.size() - 64);
        ++head[0];
      }
    }
    put(out, head, 2);
    put(out, records.data(), records.size());
    put(out, descriptors.data(), descriptors.size());
  } else if (mode == 3) {
    const int W = in.get<int32_t>(), H = in.get<int32_t>();
    const Integral I = integral_of(in.image(W, H), W, H);
    put(out, I.s.data(), I.s.size());
  } else if (mode == 4) {
    const int n = in.get<int32_t>();
    std::vector<float> r(n);
    for (int i = 0; i < n; ++i) {
      const float y = in.get<float>(), x = in.get<float>();
      r[i] = fast_atan2(y, x);
    }
    put(out, r.data(), r.size());
  } else {
    return 5;
  }
  return std::fclose(out) == 0 ? 0 : 4;
}
