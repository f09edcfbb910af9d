// One host thread over dliom_float_text: the XYZ writer's loop with the library's formatter in place of the
// std::ostringstream (built and run by tools/xyz_bench.py; links libdliom.so).
//   xyz_host_loop <in> <out>     <in>: raw floats, three a point; <out>: the text; prints the loop's milliseconds
#include <chrono>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "dliom.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  const std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  if (raw.size() % 12 != 0) return 2;
  const float* points = reinterpret_cast<const float*>(raw.data());
  const size_t n = raw.size() / 12;
  std::string text(n * DLIOM_XYZ_MAX_RECORD, '\0');
  size_t at = 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      char buffer[16];
      int32_t length = 0;
      if (dliom_float_text(points[3 * i + k], buffer, &length) != DLIOM_OK) return 1;
      text.replace(at, static_cast<size_t>(length), buffer, static_cast<size_t>(length));
      at += static_cast<size_t>(length);
      text[at++] = k == 2 ? '\n' : ' ';
    }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  std::ofstream out(argv[2], std::ios::binary);
  out.write(text.data(), static_cast<std::streamsize>(at));
  if (!out.good()) return 2;
  std::printf("%.6f\n", ms);
  return 0;
}
