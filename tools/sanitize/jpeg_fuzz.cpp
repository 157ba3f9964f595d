// Stand-alone sanitizer harness of the JPEG entropy decoder (csrc/data/jpeg.cpp). Host only:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Icsrc/data \
//       tools/sanitize/jpeg_fuzz.cpp csrc/data/jpeg.cpp -o build/jpeg_fuzz
//   build/jpeg_fuzz <directory of files>
//
// Every file of the directory is decoded as it is, at every prefix length, and with seeded single-byte
// corruptions, each for the whole image and for a few windows, into an exactly sized heap buffer (so a
// write past the capacity is a heap overflow the sanitizer reports). The input is copied into an exactly
// sized heap buffer too, so a read past its end is reported as well. Exit status 0: no finding.
#include <dirent.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "jpeg.h"

static long g_decoded = 0, g_declined = 0;

static void run(const std::vector<uint8_t>& bytes, size_t n, int wy, int wx, int wh, int ww, size_t cap) {
  uint8_t* in = static_cast<uint8_t*>(std::malloc(n ? n : 1));
  std::memcpy(in, bytes.data(), n);
  void* mem = nullptr;
  if (posix_memalign(&mem, 16, cap ? cap : 16) != 0) std::abort();
  const char* why = nullptr;
  const long r = hcbjpeg::jpeg_entropy_decode(in, n, wy, wx, wh, ww, static_cast<uint8_t*>(mem), cap, &why);
  if (r < 0) {
    if (!why || !*why) {
      std::fprintf(stderr, "declined without a reason\n");
      std::exit(2);
    }
    ++g_declined;
  } else {
    if ((size_t)r > cap) {
      std::fprintf(stderr, "record of %ld bytes in a buffer of %zu\n", r, cap);
      std::exit(2);
    }
    ++g_decoded;
  }
  std::free(mem);
  std::free(in);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s <directory>\n", argv[0]);
    return 2;
  }
  DIR* d = opendir(argv[1]);
  if (!d) {
    std::perror(argv[1]);
    return 2;
  }
  std::vector<std::string> files;
  while (dirent* e = readdir(d))
    if (e->d_name[0] != '.') files.push_back(std::string(argv[1]) + "/" + e->d_name);
  closedir(d);
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&rng]() {
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return rng;
  };
  const int wins[][4] = {{0, 0, 0, 0}, {0, 0, 1, 1}, {5, 5, 9, 9}, {3, 1, 4, 7}, {16, 16, 8, 8}};
  for (const std::string& f : files) {
    std::ifstream is(f, std::ios::binary);
    std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());
    for (const auto& w : wins) {
      run(bytes, bytes.size(), w[0], w[1], w[2], w[3], 1 << 20);
      run(bytes, bytes.size(), w[0], w[1], w[2], w[3], 640 + 128 * 3);  // a capacity most windows exceed
    }
    for (size_t n = 0; n < bytes.size(); ++n) run(bytes, n, 0, 0, 0, 0, 1 << 16);
    for (int i = 0; i < 2000 && bytes.size() > 2; ++i) {
      std::vector<uint8_t> bad = bytes;
      bad[next() % bad.size()] ^= (uint8_t)(1 + next() % 255);
      const auto& w = wins[next() % 5];
      run(bad, bad.size(), w[0], w[1], w[2], w[3], 1 << 16);
    }
  }
  std::printf("%zu files: %ld decoded, %ld declined, no sanitizer finding\n", files.size(), g_decoded, g_declined);
  return 0;
}
