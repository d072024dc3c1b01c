// Pareto-smoothed importance-sampling leave-one-out (gdrf_predict_loo, gdrf_psis_rows): for a row with the S log likelihoods a_s of
// predict_score.h (the Multinomial coefficient left out), in double throughout,
//   1  x_s = min_t(a_t) - a_s, the log importance ratios with their maximum at 0, ordered ascending x_(0) <= .. <= x_(S-1);
//      a_(r) = min(a) - x_(r): no index travels with a value
//   2  M = ceil(min(S / 5, 3 sqrt(S))) (the host's, passed in), u = x_(S-M-1), y_i = exp(x_(S-M+i)) - exp(u), i = 0 .. M-1, ascending
//   3  q = y_(floor(M/4 + 0.5) - 1); q not > 0: no fit, pareto_k = NaN, the tail stays.  A non-finite k from the fit is returned and
//      the tail stays
//   4  Zhang & Stephens 2009 without the pruning of negligible weights: m = 30 + floor(sqrt(M)), for j = 1 .. m
//        b_j = (1 - sqrt(m / (j - 0.5))) / (3 q) + 1 / y_(M-1),  k_j = mean_i log1p(-b_j y_i),  L_j = M (log(-b_j / k_j) - k_j - 1)
//        w_j = 1 / sum_t exp(L_t - L_j), normalised to sum to 1
//      b = sum_j w_j b_j,  k' = mean_i log1p(-b y_i),  sigma = -k' / b,  pareto_k = (M k' + 5) / (M + 10)
//   5  p_i = (i + 0.5) / M: the tail value x_(S-M+i) becomes log(sigma expm1(-k log1p(-p_i)) / k + exp(u)), k = pareto_k
//      (k == 0: the limit -sigma log1p(-p_i))
//   6  x = min(x, 0),  lw_(r) = x_(r) - logsumexp(x)
//   7  elpd_loo = logsumexp_r(a_(r) + lw_(r)),  ess = 1 / sum_r exp(2 lw_(r))
// A row whose a_s are all equal gives elpd_loo = a, ess = S, pareto_k = NaN; an empty row elpd_loo = 0.
//
// group_psis is run by the LG lanes of the group that owns the row, on the row's LDS: x[P] holds a_s (P = S rounded up to a power of
// two), scr[M + 3 m] is the fit's.  The values are ordered in place by predict_quant.h's bitonic network (the tail up to P is +inf and
// sorts last); the exceedances go to scr[0 .. M), the grid's b_j, L_j and w_j behind them, lane l on j = l + 1, l + 1 + LG, ..: a lane
// sums a grid point's M terms alone, in i order, and every lane sums the m weights in j order, so the fit's own sums do not depend on
// LG; the sums over a row's M or S terms (k', the two logsumexps, ess) are a lane's strided share, then a butterfly.  The smoothed tail
// replaces the exceedances in scr - a_(r) needs the ordered x as they were.  Every exchange is private to the group, hence to a wave:
// wave_lds_fence and no barrier.
//
// Two kernels call it:
//   predict_loo_kernel<T, LG, KJ, CSR>  follows predict_score_kernel step for step - the row prior, the draws, the softmax, theta_phi,
//       the per-chunk group_sum, GDRF_SCORE_V_CHUNK, the order of every sum - so a row's a_s are bit for bit the ones
//       gdrf_predict_score folds, and folds them through ScoreStats in sample order too: lpd, total and log_coef are its, bit for bit.
//       It keeps all S of a row in LDS instead of a tile of GDRF_SCORE_S_TILE, which removes the sample tiles: a chunk of Phi is
//       visited once.  A workgroup pass takes RP rows (forms.h::loo_plan), the groups g < RP; the others idle and, in the dense form,
//       still join the staging barriers.  a_out (S, nrows), optional, receives the a_s.
//   psis_rows_kernel<LG>  a caller's (S, nrows) double matrix from global memory, no model quantity.
// out is (6, nrows) double: elpd_loo, pareto_k, ess, lpd, total, log_coef; the stage kernel writes the first three.
// Nothing about a row depends on another row, on the grid or on how the rows are cut into calls; no atomics: every output is
// bit-identical under any batching.
#pragma once
#include "common.h"
#include "kernels_n.h"
#include "lane_group.h"
#include "predict_quant.h"     // group_bitonic_sort
#include "predict_score.h"     // ScoreStats, score_theta, score_chunk_stride

#ifndef GDRF_LOO_MAX_SAMPLES   // include/gdrf_hip.h declares both too
#define GDRF_LOO_MAX_SAMPLES 1024
#define GDRF_LOO_MIN_SAMPLES 25
#endif

namespace gdrf {

constexpr int PSIS_LG = 16;    // the lanes of a row's group in psis_rows_kernel

// The row's result in every lane of the group.  On return x[0 .. S) holds the ordered x_(r); the caller fences before x or scr is rewritten.
template <int LG>
__device__ void group_psis(double* x, double* scr, int S, int P, int M, int l, double& elpd, double& pareto_k, double& ess) {
  const double qnan = __builtin_nan("");
  // 1: the shift, the padding, the order
  double amin = INFINITY;
  for (int s = l; s < S; s += LG) amin = fmin(amin, x[s]);
  amin = -group_max<LG>(-amin);
  for (int s = l; s < P; s += LG) x[s] = s < S ? amin - x[s] : (double)INFINITY;
  wave_lds_fence();
  group_bitonic_sort<double, LG>(x, P, l);
  // 2: the exceedances over the cutoff
  const int t0 = S - M, m = 30 + (int)floor(sqrt((double)M));
  double* y = scr;
  double* bj = scr + M;
  double* Lj = bj + m;
  double* wj = Lj + m;
  const double dM = (double)M, eu = exp(x[t0 - 1]);
  for (int i = l; i < M; i += LG) y[i] = exp(x[t0 + i]) - eu;
  wave_lds_fence();
  // 3, 4: the fit
  const double q = y[(int)floor(dM / 4.0 + 0.5) - 1], ymax = y[M - 1];
  double k = qnan, sigma = 0;
  if (q > 0) {                                                     // the lanes of a group agree
    for (int j = l; j < m; j += LG) {
      const double b = (1.0 - sqrt((double)m / ((double)(j + 1) - 0.5))) / (3.0 * q) + 1.0 / ymax;
      double kk = 0;
      for (int i = 0; i < M; ++i) kk += log1p(-b * y[i]);
      kk /= dM;
      bj[j] = b;
      Lj[j] = dM * (log(-b / kk) - kk - 1.0);
    }
    wave_lds_fence();
    for (int j = l; j < m; j += LG) {
      const double Lme = Lj[j];
      double sw = 0;
      for (int t = 0; t < m; ++t) sw += exp(Lj[t] - Lme);
      wj[j] = 1.0 / sw;
    }
    wave_lds_fence();
    double wsum = 0, b = 0;
    for (int j = 0; j < m; ++j) wsum += wj[j];
    for (int j = 0; j < m; ++j) b += wj[j] / wsum * bj[j];
    double kp = 0;
    for (int i = l; i < M; i += LG) kp += log1p(-b * y[i]);
    kp = group_sum<LG>(kp) / dM;
    sigma = -kp / b;
    k = (dM * kp + 5.0) / (dM + 10.0);
  }
  wave_lds_fence();                                                // y was read by every lane and is rewritten now
  // 5, 6: the tail, smoothed where the fit stands, and the truncation at 0, into scr
  const bool smooth = q > 0 && isfinite(k);
  for (int i = l; i < M; i += LG) {
    double v = x[t0 + i];
    if (smooth) {
      const double lp = log1p(-((double)i + 0.5) / dM);
      const double qt = k == 0.0 ? -sigma * lp : sigma * expm1(-k * lp) / k;
      v = log(qt + eu);
    }
    y[i] = fmin(v, 0.0);
  }
  wave_lds_fence();
  auto xs = [&](int r) { return r < t0 ? fmin(x[r], 0.0) : y[r - t0]; };
  double mx = -INFINITY;
  for (int r = l; r < S; r += LG) mx = fmax(mx, xs(r));
  mx = group_max<LG>(mx);
  double se = 0;
  for (int r = l; r < S; r += LG) se += exp(xs(r) - mx);
  const double lse = mx + log(group_sum<LG>(se));
  // 7: the outputs
  double tm = -INFINITY;
  for (int r = l; r < S; r += LG) tm = fmax(tm, (amin - x[r]) + (xs(r) - lse));
  tm = group_max<LG>(tm);
  double st = 0, s2 = 0;
  for (int r = l; r < S; r += LG) {
    const double lw = xs(r) - lse;
    st += exp((amin - x[r]) + lw - tm);
    s2 += exp(2.0 * lw);
  }
  elpd = tm + log(group_sum<LG>(st));
  ess = 1.0 / group_sum<LG>(s2);
  pareto_k = k;
}

// dynamic LDS (forms.h::loo_plan has the same sum): rows [RP][stride] double | Phi chunk [K][W] (dense) | theta [RP][LG KJ] | counts [RP][W] (dense)
template <typename T, int LG, int KJ, bool CSR>
__global__ __launch_bounds__(256) void predict_loo_kernel(
    int64_t nrows, int K, int V, int S, int RP, int P, int M, int stride, const Hyper* __restrict__ h, const T* __restrict__ qpart, int nqpart,
    const T* __restrict__ loc, const T* __restrict__ tt, int64_t ldk, const T* __restrict__ mean, int64_t mean_sk, int64_t mean_sn,
    const T* __restrict__ eps, uint64_t seed, int64_t row_offset, const T* __restrict__ phi, const int32_t* __restrict__ ws,
    const int64_t* __restrict__ crow, const int32_t* __restrict__ col, const int32_t* __restrict__ val, double* __restrict__ out,
    double* __restrict__ a_out) {
  constexpr int Kp = LG * KJ, VC = GDRF_SCORE_V_CHUNK;
  extern __shared__ __attribute__((aligned(16))) char loo_smem[];
  const int tid = threadIdx.x, l = tid % LG, g = tid / LG;
  const int W = min(V, VC);
  double* aS = reinterpret_cast<double*>(loo_smem);
  T* phiS = reinterpret_cast<T*>(aS + (size_t)RP * stride);              // dense only, as is wS
  T* thS = CSR ? phiS : phiS + (size_t)K * W;
  int32_t* wS = reinterpret_cast<int32_t*>(thS + RP * Kp);
  const int gr = g < RP ? g : 0;                                         // a group without a row of the pass touches no LDS of its own
  T* th_row = thS + gr * Kp;
  double* a_row = aS + (size_t)gr * stride;
  int32_t* w_row = wS + (size_t)gr * W;
  const int nchunk = (V + VC - 1) / VC;
  // chunk c of Phi into LDS, as predict_score_kernel stages it
  auto stage = [&](int c) -> int {
    const int cw = min(VC, V - c * VC);
    if (nchunk > 1) __syncthreads();
    for (int e = tid; e < K * W; e += 256) {
      const int k = e / W, v = e - k * W;
      phiS[e] = v < cw ? phi[(int64_t)k * V + c * VC + v] : T(0);
    }
    if (nchunk > 1) __syncthreads();
    return cw;
  };
  if constexpr (!CSR) { if (nchunk == 1) { stage(0); __syncthreads(); } }
  const T var0 = (T)h->var;
  const int64_t nblk = (nrows + RP - 1) / RP;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {         // dense: uniform over the workgroup, every group joins the barriers
    const int64_t n = blk * RP + g;
    const bool active = g < RP && n < nrows;                             // the lanes of a group agree
    if (CSR && !active) continue;
    T m[KJ], sd[KJ];
#pragma unroll
    for (int j = 0; j < KJ; ++j) m[j] = sd[j] = 0;
    if (active) {
      const T v0 = row_prior_v0(qpart, nqpart, ldk, n, var0);
#pragma unroll
      for (int j = 0; j < KJ; ++j) {
        const int k = l + LG * j;
        if (k < K) row_prior_topic(v0, loc, tt, ldk, mean, mean_sk, mean_sn, k, n, m[j], sd[j]);
      }
    }
    ScoreStats st;
    double tot = 0, lg = 0;                                              // this lane's shares of sum w and sum lgamma(w + 1)
    if constexpr (CSR) {
      const int64_t e0 = crow[n], e1 = crow[n + 1];
      for (int64_t e = e0 + l; e < e1; e += LG) {
        const int32_t w = val[e];
        if (w == 0) continue;
        tot += (double)w; lg += score_lfact((double)w);
      }
      for (int s = 0; s < S; ++s) {
        score_theta<T, LG, KJ>(th_row, m, sd, eps, seed, row_offset, nrows, n, K, l, s);
        wave_lds_fence();
        double a = 0;
        for (int64_t e = e0 + l; e < e1; e += LG) {
          const int32_t w = val[e];
          if (w == 0) continue;                                          // a stored zero is an absent entry
          a += (double)w * (double)t_log<T>(theta_phi(th_row, phi + col[e], (int64_t)V, K));
        }
        wave_lds_fence();                                                // theta is rewritten by the next sample
        a = group_sum<LG>(a);
        st.take(s, a);
        if (l == 0) a_row[s] = a;
      }
    } else {
      for (int c = 0; c < nchunk; ++c) {
        const int cw = nchunk > 1 ? stage(c) : V;
        if (!active) continue;
        for (int v = l; v < cw; v += LG) {
          const int32_t w = ws[n * V + c * VC + v];
          w_row[v] = w;
          if (w != 0) { tot += (double)w; lg += score_lfact((double)w); }
        }
        wave_lds_fence();
        for (int s = 0; s < S; ++s) {
          score_theta<T, LG, KJ>(th_row, m, sd, eps, seed, row_offset, nrows, n, K, l, s);
          wave_lds_fence();
          double a = 0;
          for (int v = l; v < cw; v += LG) {
            const int32_t w = w_row[v];
            if (w == 0) continue;
            a += (double)w * (double)t_log<T>(theta_phi(th_row, phiS + v, W, K));
          }
          wave_lds_fence();                                              // theta is rewritten by the next sample
          a = group_sum<LG>(a);
          if (l == 0) a_row[s] = c == 0 ? a : a_row[s] + a;              // lane 0 alone touches the samples until they are folded
        }
        wave_lds_fence();                                                // the counts are rewritten by the next chunk
      }
      if (!active) continue;
      wave_lds_fence();
      for (int s = 0; s < S; ++s) st.take(s, a_row[s]);
    }
    wave_lds_fence();
    tot = group_sum<LG>(tot);
    lg = group_sum<LG>(lg);
    if (a_out) for (int s = l; s < S; s += LG) a_out[(int64_t)s * nrows + n] = a_row[s];
    double elpd, pk, ess;
    group_psis<LG>(a_row, a_row + P, S, P, M, l, elpd, pk, ess);
    if (l == 0) {
      out[n] = elpd;
      out[nrows + n] = pk;
      out[2 * nrows + n] = ess;
      out[3 * nrows + n] = st.lm + log(st.la) - log((double)S);         // ScoreStats::store's lpd
      out[4 * nrows + n] = tot;
      out[5 * nrows + n] = score_lfact(tot) - lg;
    }
    wave_lds_fence();                                                    // the samples are rewritten by the next pass
  }
}

// the stage alone: log_lik (S, nrows) double -> out rows 0 .. 2 of (3, nrows); LDS rows [RP][stride] double
template <int LG>
__global__ __launch_bounds__(256) void psis_rows_kernel(int64_t nrows, int S, int RP, int P, int M, int stride, const double* __restrict__ log_lik,
                                                        double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char loo_smem[];
  const int tid = threadIdx.x, l = tid % LG, g = tid / LG;
  if (g >= RP) return;                                                   // no barrier anywhere: the group may leave
  double* a_row = reinterpret_cast<double*>(loo_smem) + (size_t)g * stride;
  const int64_t nblk = (nrows + RP - 1) / RP;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t n = blk * RP + g;
    if (n >= nrows) continue;
    for (int s = l; s < S; s += LG) a_row[s] = log_lik[(int64_t)s * nrows + n];
    wave_lds_fence();
    double elpd, pk, ess;
    group_psis<LG>(a_row, a_row + P, S, P, M, l, elpd, pk, ess);
    if (l == 0) { out[n] = elpd; out[nrows + n] = pk; out[2 * nrows + n] = ess; }
    wave_lds_fence();
  }
}

}  // namespace gdrf
