// The planning rule of gdrf_predict_quant's quantile mode (gdrf_amd/csrc/forms.h::quant_plan) as a table, without a GPU.
// Build: c++ -std=c++17 -o quant_plan tests/host/quant_plan.cpp
//   quant_plan           reads one shape per line from stdin:  K C S esz LG   and prints, per shape,  RP CP P lds
//   quant_plan budget    prints the LDS budget of the rule in bytes
#include "../../gdrf_amd/csrc/forms.h"

#include <cstdio>
#include <cstring>

using namespace gdrf::forms;

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "budget")) {
    std::printf("%zu\n", QUANT_LDS);
    return 0;
  }
  int K, C, S, esz, LG;
  while (std::scanf("%d %d %d %d %d", &K, &C, &S, &esz, &LG) == 5) {
    const QuantPlan p = quant_plan(K, C, S, esz, LG);
    std::printf("%d %d %d %zu\n", p.RP, p.CP, p.P, p.lds);
  }
  return 0;
}
