// One-thread restatement of Compress (include/dliom.h "compressed point clouds"), written from that statement: the
// bound check, one rounding a coordinate, a stable sort by the nine-field block key, a walk over the sorted points.
// tools/compressed_cloud_bench.py checks the device batch equal to it before timing either.
//
//   compressed_cloud_model in.bin out.bin [repeats]
//     in.bin:  int32 clouds | per cloud: int32 n | float xyz[3 n]
//     out.bin: per cloud: int32 num_points (-1: refused) | int64 words | int32 point_data[words]
//     repeats > 0: compresses everything `repeats` more times and prints the median milliseconds of a pass
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

namespace {

struct Cloud {
  std::vector<float> xyz;
};

bool in_bound(float p) { return std::fabs(p) / 0.001f < 8388608.f; }

// the nine fields of a block, most significant first
std::array<int, 9> block_fields(const std::array<int, 3>& block) {
  const int X = block[0] + 8192, Y = block[1] + 8192, Z = block[2] + 8192;
  return {{Z >> 6, Y >> 6, X >> 6, (Z >> 3) & 7, (Y >> 3) & 7, (X >> 3) & 7, Z & 7, Y & 7, X & 7}};
}

// false: refused
bool compress(const Cloud& cloud, std::vector<int32_t>* point_data) {
  const size_t n = cloud.xyz.size() / 3;
  point_data->clear();
  std::vector<std::array<int, 3>> block(n);
  std::vector<int32_t> word(n);
  for (size_t i = 0; i < n; ++i) {
    int off[3];
    for (int a = 0; a < 3; ++a) {
      const float p = cloud.xyz[3 * i + a];
      if (!in_bound(p)) return false;
      const long q = std::lround(p / 0.001f);
      block[i][a] = static_cast<int>(q >> 10);
      off[a] = static_cast<int>(q & 1023);
    }
    word[i] = (((off[2] << 10) + off[1]) << 10) + off[0];
  }
  std::vector<size_t> order(n);
  std::iota(order.begin(), order.end(), size_t{0});
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return block_fields(block[a]) < block_fields(block[b]); });
  for (size_t s = 0; s < n;) {
    size_t e = s;
    while (e < n && block[order[e]] == block[order[s]]) ++e;
    point_data->push_back(static_cast<int32_t>(e - s));
    for (int a = 0; a < 3; ++a) point_data->push_back(block[order[s]][a]);
    for (size_t i = s; i < e; ++i) point_data->push_back(word[order[i]]);
    s = e;
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  if (in == nullptr) return 2;
  int32_t k = 0;
  if (std::fread(&k, 4, 1, in) != 1 || k < 0) return 2;
  std::vector<Cloud> clouds(static_cast<size_t>(k));
  for (Cloud& c : clouds) {
    int32_t n = 0;
    if (std::fread(&n, 4, 1, in) != 1 || n < 0) return 2;
    c.xyz.resize(3 * static_cast<size_t>(n));
    if (n > 0 && std::fread(c.xyz.data(), 12, static_cast<size_t>(n), in) != static_cast<size_t>(n)) return 2;
  }
  std::fclose(in);
  std::FILE* out = std::fopen(argv[2], "wb");
  if (out == nullptr) return 2;
  std::vector<int32_t> data;
  for (const Cloud& c : clouds) {
    const bool ok = compress(c, &data);
    const int32_t num_points = ok ? static_cast<int32_t>(c.xyz.size() / 3) : -1;
    const int64_t words = ok ? static_cast<int64_t>(data.size()) : 0;
    std::fwrite(&num_points, 4, 1, out);
    std::fwrite(&words, 8, 1, out);
    if (words > 0) std::fwrite(data.data(), 4, static_cast<size_t>(words), out);
  }
  std::fclose(out);
  const int repeats = argc > 3 ? std::atoi(argv[3]) : 0;
  if (repeats > 0) {
    std::vector<double> ms;
    size_t sink = 0;
    for (int r = 0; r < repeats; ++r) {
      const auto t0 = std::chrono::steady_clock::now();
      for (const Cloud& c : clouds) {
        compress(c, &data);
        sink += data.size();
      }
      ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    std::printf("%.4f %zu\n", ms[ms.size() / 2], sink);
  }
  return 0;
}
