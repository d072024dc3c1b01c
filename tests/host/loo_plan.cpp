// The planning rule of gdrf_predict_loo and gdrf_psis_rows (gdrf_amd/csrc/forms.h::loo_plan) as a table, without a GPU.
// Build: c++ -std=c++17 -o loo_plan tests/host/loo_plan.cpp
//   loo_plan           reads one shape per line from stdin:  K V S esz LG csr   and prints, per shape,  RP P M stride lds
//   loo_plan budget    prints the LDS a workgroup may take, the LDS of a compute unit and the workgroups counted on one (fused, stage)
#include "../../gdrf_amd/csrc/forms.h"

#include <cstdio>
#include <cstring>

using namespace gdrf::forms;

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "budget")) {
    std::printf("%zu %zu %d %d\n", LDS_ROWS, LDS_MAX, LOO_WG_CU, LOO_STAGE_WG_CU);
    return 0;
  }
  int K, V, S, esz, LG, csr;
  while (std::scanf("%d %d %d %d %d %d", &K, &V, &S, &esz, &LG, &csr) == 6) {
    const LooPlan p = loo_plan(K, V, S, esz, LG, csr != 0);
    std::printf("%d %d %d %d %zu\n", p.RP, p.P, p.M, p.stride, p.lds);
  }
  return 0;
}
