// CPU model of the XYZ writer's per-point loop (io/xyz_writing_points_processor.cc:13-20): one std::ostringstream a point,
// std::setprecision(6), x y z separated by spaces, a newline.  The reference's own arithmetic through the C++ library; it
// shares nothing with d-liom_amd/csrc/float_text.h.
//
//   xyz_writer_model <in> <out> [--time]
// <in>: raw little-endian floats, three a point.  <out>: the text.  --time prints the loop's milliseconds (one thread).
#include <chrono>
#include <cstdio>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  const std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  if (!in.good() && !in.eof()) return 2;
  if (raw.size() % 12 != 0) return 2;
  const float* points = reinterpret_cast<const float*>(raw.data());
  const size_t n = raw.size() / 12;
  std::string text;
  const auto t0 = std::chrono::steady_clock::now();
  for (size_t i = 0; i < n; ++i) {
    std::ostringstream stream;
    stream << std::setprecision(6);
    stream << points[3 * i] << " " << points[3 * i + 1] << " " << points[3 * i + 2] << "\n";
    text += stream.str();
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  std::ofstream out(argv[2], std::ios::binary);
  out.write(text.data(), static_cast<std::streamsize>(text.size()));
  if (!out.good()) return 2;
  if (argc > 3 && std::string(argv[3]) == "--time") std::printf("%.6f\n", ms);
  return 0;
}
