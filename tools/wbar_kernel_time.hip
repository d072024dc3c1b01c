// Timing-only harness: the two f16x3 W-bar kernels (gemm_split.h: one wave per SIMD / k64) alone at the headline shape on pseudo-random operands,
// on the grid and LDS bytes of csrc/forms.h's plan, as api.hip launches them.  Results are not checked.  Build and run from the repository root:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Wno-unused-function -o /tmp/wbar_time tools/wbar_kernel_time.hip && /tmp/wbar_time
#include <hip/hip_runtime.h>
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
  _Float16 *Wh, *Bh; float *W, *Wbar, *vbar, *locbar, *asum, *U, *sc; unsigned* mx;
  CK(hipMalloc(&Wh, 2 * n * Mp * 2)); CK(hipMalloc(&Bh, 2 * (size_t)K * Mp * Mp * 2)); CK(hipMalloc(&W, n * Mp * 4)); CK(hipMalloc(&Wbar, n * Mp * 4));
  CK(hipMalloc(&vbar, K * n * 4)); CK(hipMalloc(&locbar, K * n * 4)); CK(hipMalloc(&asum, n * 4)); CK(hipMalloc(&U, K * Mp * 4)); CK(hipMalloc(&sc, 1024)); CK(hipMalloc(&mx, 1024));
  fill_h<<<4096, 256>>>(Wh, 2 * n * Mp, 8000.f); fill_h<<<1024, 256>>>(Bh, 2 * (size_t)K * Mp * Mp, 8000.f); fill_f<<<4096, 256>>>(W, n * Mp, 1.f);
  fill_f<<<1024, 256>>>(vbar, K * n, 1.f); fill_f<<<1024, 256>>>(locbar, K * n, 1.f); fill_f<<<256, 256>>>(asum, n, 1.f); fill_f<<<16, 256>>>(U, K * Mp, 1.f); fill_f<<<1, 256>>>(sc, 256, 1e-6f);
  CK(hipMemset(mx, 0, 1024));
  BwdWbarSplitArgs<SplitF16> a{W, Wh, n * Mp, n, Mp, Mp, K, Bh, (int64_t)K * Mp * Mp, vbar, locbar, n, asum, U, Wbar, sc, mx};
  // the plan of the shape (one wave per SIMD), and the k64 form's of the same shape: what the host took before, K past the w1 gate aside
  forms::FormShape f; f.n = f.n_cap = n; f.M = f.Mp = Mp; f.K = K; f.split = 2; f.nsplit_cap = forms::nsplit_cap_rule(K, Mp, n, 4);
  const forms::WbarPlan pw = forms::wbar_plan(f);
  if (pw.form != forms::WBAR_W1 || pw.R != 2) { printf("the shape does not take the one-wave form with two requests per phase\n"); return 1; }
  const unsigned grid = pw.grid;
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const size_t lds_w1 = pw.lds, lds64 = forms::wbar_k64_lds(K);
  CK(hipFuncSetAttribute((const void*)bwd_wbar_f16_w1_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_w1));
  CK(hipFuncSetAttribute((const void*)bwd_wbar_f16_k64_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds64));
  for (int which = 0; which < 2; ++which) {
    float best = 1e9f, sum = 0;
    for (int r = 0; r < reps + 1; ++r) {
      CK(hipEventRecord(e0));
      if (which == 0) hipLaunchKernelGGL(bwd_wbar_f16_w1_kernel<2>, dim3(grid), dim3(256), lds_w1, 0, a);
      else hipLaunchKernelGGL(bwd_wbar_f16_k64_kernel, dim3(grid, 1), dim3(512), lds64, 0, a);
      CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      if (r) { sum += ms; best = ms < best ? ms : best; }
    }
    printf("%s %s: mean %.3f ms, best %.3f ms\n", argv[0], which == 0 ? "w1 " : "k64", sum / reps, best);
  }
  return 0;
}
