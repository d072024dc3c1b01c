// log(w!) = lgamma(w + 1) at a count w (a whole number >= 0), in double - what predict_score_kernel forms its Multinomial coefficient
// from.  The log of the exact factorial from a table below 24, Stirling's series in 1 / (w + 1) from there (its first omitted term,
// 1 / (1188 (w + 1)^9), is below 3e-16 at w = 24, where the value is 54.8).  The library's lgamma is exact to the same few ulps, but
// inlined it takes the kernel from 160 - 180 registers to 256 and past them: one log and a polynomial keep the occupancy of the sibling
// kernels.  A negative w is not a count (no caller passes one): it reads as an absent entry, 0, and never indexes the table.
// No HIP in this file but the two qualifiers: the host compiler builds it alone for tests/host/score_lfact.cpp.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define GDRF_LFACT_HD __host__ __device__ __forceinline__
#else
#define GDRF_LFACT_HD inline
#endif

namespace gdrf {

constexpr int SCORE_LFACT_TABLE = 24;      // counts below this come from the table

GDRF_LFACT_HD double score_lfact(double w) {
  constexpr double table[SCORE_LFACT_TABLE] = {
      0.0, 0.0, 0.6931471805599453, 1.791759469228055, 3.1780538303479458, 4.787491742782046, 6.579251212010101, 8.525161361065415,
      10.60460290274525, 12.801827480081469, 15.104412573075516, 17.502307845873887, 19.987214495661885, 22.552163853123425,
      25.19122118273868, 27.89927138384089, 30.671860106080672, 33.50507345013689, 36.39544520803305, 39.339884187199495,
      42.335616460753485, 45.38013889847691, 48.47118135183523, 51.60667556776438};
  if (w < (double)SCORE_LFACT_TABLE) return w > 1.0 ? table[(int)w] : 0.0;
  const double x = w + 1.0, r = 1.0 / x, r2 = r * r;
  return (x - 0.5) * log(x) - x + 0.9189385332046727 + r * (1.0 / 12.0 - r2 * (1.0 / 360.0 - r2 * (1.0 / 1260.0 - r2 * (1.0 / 1680.0))));
}

}  // namespace gdrf
