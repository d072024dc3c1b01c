// Timing-only harness: the two f16x3 tt kernels (gemm_split.h: one wave per SIMD / q4) alone at the headline shape on pseudo-random operands,
// on the grids and LDS bytes of csrc/forms.h's plan, as api.hip launches them.  Results are not checked.  Build and run from the repository root:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Wno-unused-function -o /tmp/fwd_t_time tools/fwd_t_kernel_time.hip && /tmp/fwd_t_time [KGP]
// KGP: topic pairs per L2 group of the one-wave kernel's pair form (default: forms.h's FWD_T_W1_KGP).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include "../gdrf_amd/csrc/gemm_split.h"
#include "../gdrf_amd/csrc/forms.h"
using namespace gdrf;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)
__global__ void fill_h(_Float16* p, size_t n, float amp) { for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) { unsigned h = (unsigned)(i * 2654435761u); h ^= h >> 15; p[i] = (_Float16)(amp * ((int)(h & 0xffff) - 32768) / 32768.0f); } }
__global__ void fill_f(float* p, size_t n, float amp) { for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) { unsigned h = (unsigned)(i * 2246822519u); h ^= h >> 13; p[i] = amp * ((int)(h & 0xffff) - 32768) / 32768.0f; } }
int main(int argc, char** argv) {
  const int64_t n = 1000000; const int Mp = 512, K = 10, reps = 5;
  const int KGP = argc > 1 ? std::max(1, atoi(argv[1])) : forms::FWD_T_W1_KGP;
  _Float16 *Wh, *STh; float *tt, *sc;
  const int64_t nb = (int64_t)K * Mp * Mp;
  CK(hipMalloc(&Wh, 2 * n * Mp * 2)); CK(hipMalloc(&STh, 2 * nb * 2)); CK(hipMalloc(&tt, K * n * 4)); CK(hipMalloc(&sc, 1024));
  fill_h<<<4096, 256>>>(Wh, 2 * n * Mp, 8000.f); fill_h<<<1024, 256>>>(STh, 2 * nb, 8000.f); fill_f<<<1, 256>>>(sc, 256, 1e-6f);
  // the plan of the shape (one wave per SIMD), and the q4 form's of the same shape
  forms::FormShape f; f.n = f.n_cap = n; f.M = f.Mp = Mp; f.K = K; f.split = 2;
  const forms::FwdTPlan pw = forms::fwd_t_plan(f), p4 = forms::fwd_t_tiled_plan(f);
  if (pw.form != forms::FWD_T_W1) { printf("the shape does not take the one-wave form\n"); return 1; }
  const int KG = p4.KG, rt8 = pw.rt8;
  FwdTSplitArgs<SplitF16> a{Wh, n * Mp, n, Mp, K, KG, rt8, STh, nb, tt, n, sc};
  // as api.hip: K / 4 * 4 topics on the quad form, the rest on the pair form
  const int KQ = pw.KQ, KPr = pw.KP;
  FwdTSplitArgs<SplitF16> aq = a; aq.k_lo = 0; aq.k_n = KQ; aq.KG = 1; aq.rt8 = pw.rt8_q;
  FwdTSplitArgs<SplitF16> a1 = a; a1.k_lo = KQ; a1.k_n = K - KQ; a1.KG = std::min(KPr, KGP);
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const int lds_w1 = pw.lds_p, lds_q = pw.lds_q, lds4 = p4.lds;
  CK(hipFuncSetAttribute((const void*)fwd_t_f16_w1_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_w1));
  CK(hipFuncSetAttribute((const void*)fwd_t_f16_w1_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_q));
  CK(hipFuncSetAttribute((const void*)fwd_t_split_q4_kernel<SplitF16>, hipFuncAttributeMaxDynamicSharedMemorySize, lds4));
  for (int which = 0; which < 2; ++which) {
    float best = 1e9f, sum = 0;
    for (int r = 0; r < reps + 1; ++r) {
      CK(hipEventRecord(e0));
      if (which == 0) {
        if (KQ) hipLaunchKernelGGL(fwd_t_f16_w1_kernel<true>, dim3(pw.grid_q), dim3(256), lds_q, 0, aq);
        if (KPr) hipLaunchKernelGGL(fwd_t_f16_w1_kernel<false>, dim3(pw.grid_p), dim3(256), lds_w1, 0, a1);
      }
      else hipLaunchKernelGGL(fwd_t_split_q4_kernel<SplitF16>, dim3(p4.grid), dim3(p4.threads), lds4, 0, a);
      CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      if (r) { sum += ms; best = ms < best ? ms : best; }
    }
    if (which == 0) printf("%s w1 (KGP %d): mean %.3f ms, best %.3f ms\n", argv[0], KGP, sum / reps, best);
    else printf("%s q4 (KG %d): mean %.3f ms, best %.3f ms\n", argv[0], KG, sum / reps, best);
  }
  return 0;
}
