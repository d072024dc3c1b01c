// log(w!) as predict_score_kernel forms it (gdrf_amd/csrc/score_lfact.h) as a table, without a GPU.
// Build: c++ -std=c++17 -o score_lfact tests/host/score_lfact.cpp
//   score_lfact          reads one count per line from stdin and prints score_lfact(w) with 17 significant digits
//   score_lfact table    prints the number of counts served from the table
#include "../../gdrf_amd/csrc/score_lfact.h"

#include <cstdio>
#include <cstring>

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "table")) {
    std::printf("%d\n", gdrf::SCORE_LFACT_TABLE);
    return 0;
  }
  double w;
  while (std::scanf("%lf", &w) == 1) std::printf("%.17g\n", gdrf::score_lfact(w));
  return 0;
}
