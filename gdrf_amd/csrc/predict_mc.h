// Monte-Carlo integration over the guide's q(mu) at new inputs (gdrf_predict_mc): for row n, topic k, sample s
//   mu[s][k][n] = f_loc[k][n] + mean[k][n] + f_var[k][n] eps[s][k][n]     (f_var as the SCALE, as the guide is written: sparse_gdrf.py:403-405)
//   theta[s][n][:] = softmax_k(mu[s][:][n]),  p[s][n][:] = theta[s][n][:] Phi
// with (f_loc, f_var) what gdrf_predict mode 4 returns.  The plug-in quantities of predict.h are softmax(f_loc); these integrate over the
// posterior of the latent field instead, which matters wherever f_var is not small (away from the data).
//
// The kernel consumes the step's forward by-products (loc, the partial row norms qpart, tt), as predict_var_kernel does, and assembles
// f_var with the same arithmetic.  eps is either an injected (S, K, n) array or generated inline: philox_normal (kernels_n.h) keyed by
// the seed with counter (global row, topic, s) - sample s of row n is bit for bit what fill_eps_kernel writes for step = s, so the draws
// do not depend on how the rows are cut into calls.
//
// A group of LG lanes owns a row, lane l holds the topics l, l + LG, ... (KJ of them: LG x KJ >= K, two per lane above 64 topics); the
// group's reductions, its softmax and the row prior are those of lane_group.h.  Nothing about a row depends on another row or on the
// grid, so every output but the score's sum over rows is bit-identical however the rows are batched.
//   mode 0  theta samples (S, n, K)
//   mode 1  mean and variance (divisor S) of theta over the samples, (2, n, K): sums of theta_s - theta_0 and of its square in double
//           registers (the shift removes the cancellation of E[x^2] - E[x]^2); no sample is stored
//   mode 2  sum_n l_n and sum w, l_n = logsumexp_s(sum_v w[n][v] log p[s][n][v]) - log S: Phi (K, V) in LDS for the workgroup, the
//           counts and the current theta of each of its rows in LDS, lanes over the words; p_v = sum_k theta_k phi_kv and its log in the
//           array precision, weighted with the count and summed in double as mode 3 of gdrf_predict does (a zero count is skipped: it
//           adds nothing); a running logsumexp in double per row; per-workgroup partials dpart[grid][2], no atomics.  p is never stored.
//   mode 3  mu samples (S, K, n), for a caller-evaluated link
#pragma once
#include "common.h"
#include "kernels_n.h"
#include "lane_group.h"

namespace gdrf {

enum { MC_THETA = 0, MC_MOMENTS = 1, MC_SCORE = 2, MC_MU = 3 };

// dynamic LDS of mode 2: Phi [K][V] | theta [rows][LG KJ] | counts [rows][V], rows = 256 / LG
template <typename T> inline size_t mc_score_lds(int K, int V, int LG, int KJ) {
  const size_t rows = 256 / LG;
  return ((size_t)K * V + rows * LG * KJ) * sizeof(T) + rows * V * sizeof(int32_t);
}

template <typename T, int LG, int KJ>
__global__ __launch_bounds__(256) void predict_mc_kernel(
    int mode, int64_t nrows, int K, int V, int S, const Hyper* __restrict__ h, const T* __restrict__ qpart, int nqpart,
    const T* __restrict__ loc, const T* __restrict__ tt, int64_t ldk, const T* __restrict__ mean, int64_t mean_sk, int64_t mean_sn,
    const T* __restrict__ eps, uint64_t seed, int64_t row_offset, const T* __restrict__ phi, const int32_t* __restrict__ ws,
    T* __restrict__ out, double* __restrict__ dpart) {
  constexpr int RPB = 256 / LG, Kp = LG * KJ;
  __shared__ double scratch[16];
  extern __shared__ __attribute__((aligned(16))) char mc_smem[];
  T* phiS = reinterpret_cast<T*>(mc_smem);                   // mode 2 only: the launch gives the other modes no dynamic LDS
  T* thS = phiS + (size_t)K * V;
  int32_t* wS = reinterpret_cast<int32_t*>(thS + RPB * Kp);
  const int tid = threadIdx.x, l = tid % LG, g = tid / LG;
  T* th_row = thS + g * Kp;
  int32_t* w_row = wS + (size_t)g * V;
  if (mode == MC_SCORE) {
    for (int e = tid; e < K * V; e += 256) phiS[e] = phi[e];
    __syncthreads();
  }
  const T var0 = (T)h->var;
  const double log_s = log((double)S);
  double s_l = 0, s_w = 0;
  const int64_t nblk = (nrows + RPB - 1) / RPB;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t n = blk * RPB + g;
    if (n >= nrows) continue;                                // the lanes of a group leave together
    const T v0 = row_prior_v0(qpart, nqpart, ldk, n, var0);
    T m[KJ], sd[KJ];
#pragma unroll
    for (int j = 0; j < KJ; ++j) {
      const int k = l + LG * j;
      m[j] = sd[j] = 0;
      if (k < K) row_prior_topic(v0, loc, tt, ldk, mean, mean_sk, mean_sn, k, n, m[j], sd[j]);
    }
    double wsum = 0;
    if (mode == MC_SCORE) {
      for (int v = l; v < V; v += LG) { const int32_t w = ws[n * V + v]; w_row[v] = w; wsum += (double)w; }
      wsum = group_sum<LG>(wsum);
    }
    T t0[KJ];
    double d1[KJ], d2[KJ];
#pragma unroll
    for (int j = 0; j < KJ; ++j) { t0[j] = 0; d1[j] = d2[j] = 0; }
    double lse_m = 0, lse_a = 0;
    for (int s = 0; s < S; ++s) {
      T th[KJ];
#pragma unroll
      for (int j = 0; j < KJ; ++j) {
        const int k = l + LG * j;
        th[j] = T(GROUP_PAD);
        if (k < K) {
          const T e = eps ? eps[((int64_t)s * K + k) * nrows + n] : philox_normal<T>(seed, (uint64_t)(n + row_offset), k, (uint32_t)s);
          th[j] = m[j] + sd[j] * e;
        }
      }
      if (mode == MC_MU) {
#pragma unroll
        for (int j = 0; j < KJ; ++j) { const int k = l + LG * j; if (k < K) out[((int64_t)s * K + k) * nrows + n] = th[j]; }
        continue;
      }
      group_softmax<LG>(th, l, K);
      if (mode == MC_THETA) {
#pragma unroll
        for (int j = 0; j < KJ; ++j) { const int k = l + LG * j; if (k < K) out[((int64_t)s * nrows + n) * K + k] = th[j]; }
      } else if (mode == MC_MOMENTS) {
#pragma unroll
        for (int j = 0; j < KJ; ++j) {
          if (s == 0) t0[j] = th[j];
          const double d = (double)th[j] - (double)t0[j];
          d1[j] += d; d2[j] += d * d;
        }
      } else {
        // this row's theta through the group's LDS slots, lanes over words
#pragma unroll
        for (int j = 0; j < KJ; ++j) { const int k = l + LG * j; if (k < K) th_row[k] = th[j]; }
        wave_lds_fence();
        double a = 0;
        for (int v = l; v < V; v += LG) {
          const int32_t w = w_row[v];
          if (w == 0) continue;
          a += (double)w * (double)t_log<T>(theta_phi(th_row, phiS + v, V, K));
        }
        wave_lds_fence();                                    // theta is rewritten by the next sample
        a = group_sum<LG>(a);
        if (s == 0) { lse_m = a; lse_a = 1.0; }
        else if (a > lse_m) { lse_a = lse_a * exp(lse_m - a) + 1.0; lse_m = a; }
        else lse_a += exp(a - lse_m);
      }
    }
    if (mode == MC_MOMENTS) {
      const double is = 1.0 / (double)S;
#pragma unroll
      for (int j = 0; j < KJ; ++j) {
        const int k = l + LG * j;
        if (k < K) {
          const double md = d1[j] * is, vr = d2[j] * is - md * md;
          out[n * K + k] = (T)((double)t0[j] + md);
          out[(nrows + n) * K + k] = (T)(vr > 0 ? vr : 0.0);
        }
      }
    } else if (mode == MC_SCORE && l == 0) {
      s_l += lse_m + log(lse_a) - log_s;
      s_w += wsum;
    }
  }
  if (mode == MC_SCORE) dpart_store2(dpart, scratch, s_l, s_w);
}

}  // namespace gdrf
