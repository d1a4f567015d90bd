// holes_check.cpp — the patch arithmetic of holes_exact.hpp as a stand-alone host program (csrc/Makefile:
// holes_check, under AddressSanitizer and UndefinedBehaviorSanitizer; host code only, run on the CPU).
//
// Reads loops from the file named on the command line: a line with L, then L lines of three
// coordinates (C99 hexadecimal floats, so nothing is rounded on the way in). For every loop it prints
//   loop <L> <W(0, L-1) as 16 hex digits> <the split table by diagonals, two hex digits per entry> <rows i.j.k ...>
// which tests/test_holes_host.py compares with the NumPy restatement of the contract.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "holes_exact.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: holes_check LOOPS_FILE\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::fprintf(stderr, "holes_check: cannot open %s\n", argv[1]);
    return 2;
  }
  int L = 0, n_loops = 0;
  while (std::fscanf(f, "%d", &L) == 1) {
    if (L < 3 || L > 255) {
      std::fprintf(stderr, "holes_check: loop length %d\n", L);
      return 2;
    }
    std::vector<double> pts(size_t(3) * L);
    for (int m = 0; m < 3 * L; ++m) {
      char word[64];
      if (std::fscanf(f, "%63s", word) != 1) {
        std::fprintf(stderr, "holes_check: short file\n");
        return 2;
      }
      pts[m] = std::strtod(word, nullptr);
    }
    const int n = pyqsm::fill_table_size(L);
    std::vector<double> W(n);
    std::vector<uint8_t> S(n);
    pyqsm::fill_table(L, pts.data(), W.data(), S.data());
    uint64_t bits;
    std::memcpy(&bits, &W[pyqsm::fill_at(L, 0, L - 1)], 8);
    std::printf("loop %d %016" PRIx64 " ", L, bits);
    for (int e = 0; e < n; ++e) std::printf("%02x", unsigned(S[e]));
    for (int q = 0; q < L - 2; ++q) {
      int i, j, k;
      pyqsm::fill_row(L, S.data(), q, &i, &j, &k);
      std::printf(" %d.%d.%d", i, j, k);
    }
    std::printf("\n");
    ++n_loops;
  }
  std::fclose(f);
  std::printf("holes_check: ok %d loops\n", n_loops);
  return 0;
}
