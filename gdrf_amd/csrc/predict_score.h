// Per-row Monte-Carlo log predictive densities (gdrf_predict_score): for row n, its counts w (V of them) and the S draws of the guide that
// gdrf_predict_mc makes,
//   mu[s][k] = f_loc[k][n] + mean[k][n] + f_var[k][n] eps[s][k][n]   (f_var as the SCALE),  theta_s = softmax_k(mu[s]),  p_s = theta_s Phi
//   a_s  = sum_{v: w_v != 0} w_v log p_sv
//   out[0]  lpd           logsumexp_s(a_s) - log S      (what MC_SCORE of predict_mc.h sums over the rows and throws away)
//   out[1]  mean_log_lik  (1/S) sum_s a_s
//   out[2]  var_log_lik   sum_s (a_s - out[1])^2 / (S - 1)      (0 for S = 1)
//   out[3]  total         sum_v w_v
//   out[4]  log_coef      lgamma(total + 1) - sum_v lgamma(w_v + 1)
// out is (5, n) double.  lpd and mean_log_lik leave the Multinomial coefficient out, as gdrf_predict mode 3 and MC_SCORE do; log_coef is
// returned beside them so that a caller can add it.  WAIC is lpd - var_log_lik, summed over the rows.
//
// A group of LG lanes owns a row as in predict_mc_kernel: the row prior, the draws (the same counter (global row, topic, s), hence the same
// bits) and the softmax are those of lane_group.h and philox_normal.  The row's current theta goes through the group's LDS slots, the
// group's lanes stride over the words: p_v = sum_k theta_k Phi[k][v] (k ascending) and its log in the array precision, weighted with the
// count and summed in double; a zero count (a stored zero) is skipped.  The statistics over the samples are ScoreStats below: a running
// logsumexp in double, and the sums of a_s - a_0 and of its square in double (the shift MC_MOMENTS uses: draws that are all equal give a
// variance of exactly 0).  log_coef is formed once per row in double.
//
// Two forms of one template:
//   dense  V and S are not limited by LDS.  Phi is staged in chunks of GDRF_SCORE_V_CHUNK words, [K][W] with W = min(V, chunk), as
//          predict_info_kernel stages its chunks, and the row's counts of the chunk go into the group's LDS slots.  a_s needs every
//          chunk before the logsumexp can take it, so the samples are taken in tiles of GDRF_SCORE_S_TILE: for a tile, over the chunks,
//          theta_s is REGENERATED for every s of the tile (the draws are counter-based; an injected eps is read again) and the chunk's
//          share of a_s - summed over the group - is added to the group's [S_TILE] doubles in LDS in chunk order; after the last chunk
//          the tile's a_s are folded into the statistics in sample order.  One chunk (V <= chunk) is staged once per workgroup, not once
//          per tile.  The staging is the only thing the workgroup does together: the row loop is uniform over the workgroup and a
//          group without a row (past the end) only joins the barriers.
//   CSR    a row's stored entries only, LG at a time, Phi read from global memory as foldin_kernel<.., true> reads it: no chunks, no
//          barrier, the sample loop outermost.  A row without stored entries gives 0 in all five outputs.
// Nothing about a row depends on another row, on the grid or on how the rows are cut into calls; no atomics, no cross-row reduction, no
// sample stored: every output is bit-identical under any batching.  (The two forms add a row's words in different orders: they agree
// to rounding, not bit for bit.)
#pragma once
#include "common.h"
#include "kernels_n.h"
#include "lane_group.h"
#include "score_lfact.h"       // log(w!) for log_coef: the library's lgamma, inlined, would cost the kernel its occupancy

#ifndef GDRF_SCORE_V_CHUNK     // include/gdrf_hip.h declares both too: the words of Phi staged in LDS at a time (K = 128 in double: 128 KB)
#define GDRF_SCORE_V_CHUNK 128
#endif
#ifndef GDRF_SCORE_S_TILE      // the samples whose a_s a group keeps in LDS while the chunks of Phi pass
#define GDRF_SCORE_S_TILE 64
#endif

namespace gdrf {

// the row stride of the staged Phi chunk
inline int score_chunk_stride(int V) { return std::min(V, (int)GDRF_SCORE_V_CHUNK); }
// dynamic LDS of the dense form: a tile [rows][S_TILE] double | Phi chunk [K][W] | theta [rows][LG KJ] | counts [rows][W], rows = 256 / LG.
// The worst case, K = 128 in double (rows = 4): 2 KB + 128 KB + 4 KB + 2 KB = 136 KB.
template <typename T> inline size_t score_dense_lds(int K, int V, int LG, int KJ) {
  const size_t rows = 256 / LG, W = score_chunk_stride(V);
  return rows * GDRF_SCORE_S_TILE * sizeof(double) + ((size_t)K * W + rows * LG * KJ) * sizeof(T) + rows * W * sizeof(int32_t);
}
// the CSR form keeps theta only
template <typename T> inline size_t score_csr_lds(int LG, int KJ) { return (size_t)(256 / LG) * LG * KJ * sizeof(T); }

// The statistics of a row over its samples, taken in sample order; every lane of the group holds the same bits.
struct ScoreStats {
  double a0 = 0, d1 = 0, d2 = 0, lm = 0, la = 0;
  __device__ __forceinline__ void take(int s, double a) {
    if (s == 0) { a0 = a; lm = a; la = 1.0; return; }
    const double d = a - a0;
    d1 += d; d2 += d * d;
    if (a > lm) { la = la * exp(lm - a) + 1.0; lm = a; }
    else la += exp(a - lm);
  }
  __device__ __forceinline__ void store(double* out, int64_t nrows, int64_t n, int S, double tot, double coef) const {
    const double md = d1 / (double)S;
    const double vr = S > 1 ? (d2 - d1 * md) / (double)(S - 1) : 0.0;
    out[n] = lm + log(la) - log((double)S);
    out[nrows + n] = a0 + md;
    out[2 * nrows + n] = vr > 0 ? vr : 0.0;
    out[3 * nrows + n] = tot;
    out[4 * nrows + n] = coef;
  }
};

// sample s of the group's row -> its LDS slots (the caller fences)
template <typename T, int LG, int KJ>
__device__ __forceinline__ void score_theta(T* th_row, const T (&m)[KJ], const T (&sd)[KJ], const T* eps, uint64_t seed, int64_t row_offset,
                                            int64_t nrows, int64_t n, int K, int l, int s) {
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
  group_softmax<LG>(th, l, K);
#pragma unroll
  for (int j = 0; j < KJ; ++j) { const int k = l + LG * j; if (k < K) th_row[k] = th[j]; }
}

template <typename T, int LG, int KJ, bool CSR>
__global__ __launch_bounds__(256) void predict_score_kernel(
    int64_t nrows, int K, int V, int S, const Hyper* __restrict__ h, const T* __restrict__ qpart, int nqpart, const T* __restrict__ loc,
    const T* __restrict__ tt, int64_t ldk, const T* __restrict__ mean, int64_t mean_sk, int64_t mean_sn, const T* __restrict__ eps,
    uint64_t seed, int64_t row_offset, const T* __restrict__ phi, const int32_t* __restrict__ ws, const int64_t* __restrict__ crow,
    const int32_t* __restrict__ col, const int32_t* __restrict__ val, double* __restrict__ out) {
  constexpr int RPB = 256 / LG, Kp = LG * KJ, VC = GDRF_SCORE_V_CHUNK, ST = GDRF_SCORE_S_TILE;
  extern __shared__ __attribute__((aligned(16))) char score_smem[];
  const int tid = threadIdx.x, l = tid % LG, g = tid / LG;
  const int W = min(V, VC);
  double* aS = reinterpret_cast<double*>(score_smem);                    // dense only, as are phiS and wS
  T* phiS = CSR ? reinterpret_cast<T*>(score_smem) : reinterpret_cast<T*>(aS + RPB * ST);
  T* thS = CSR ? phiS : phiS + (size_t)K * W;
  int32_t* wS = reinterpret_cast<int32_t*>(thS + RPB * Kp);
  T* th_row = thS + g * Kp;
  double* a_row = aS + g * ST;
  int32_t* w_row = wS + (size_t)g * W;
  const int nchunk = (V + VC - 1) / VC;
  // chunk c of Phi into LDS; more than one chunk: behind a barrier (the previous one may still be read) and before one.  Returns the
  // chunk's words.
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
  const int64_t nblk = (nrows + RPB - 1) / RPB;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {         // dense: uniform over the workgroup, every group joins the barriers
    const int64_t n = blk * RPB + g;
    const bool active = n < nrows;                                       // the lanes of a group agree
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
        st.take(s, group_sum<LG>(a));
      }
    } else {
      for (int t0 = 0; t0 < S; t0 += ST) {
        const int ts = min(ST, S - t0);
        for (int c = 0; c < nchunk; ++c) {
          const int cw = nchunk > 1 ? stage(c) : V;
          if (!active) continue;
          for (int v = l; v < cw; v += LG) {
            const int32_t w = ws[n * V + c * VC + v];
            w_row[v] = w;
            if (t0 == 0 && w != 0) { tot += (double)w; lg += score_lfact((double)w); }
          }
          wave_lds_fence();
          for (int s = 0; s < ts; ++s) {
            score_theta<T, LG, KJ>(th_row, m, sd, eps, seed, row_offset, nrows, n, K, l, t0 + s);
            wave_lds_fence();
            double a = 0;
            for (int v = l; v < cw; v += LG) {
              const int32_t w = w_row[v];
              if (w == 0) continue;
              a += (double)w * (double)t_log<T>(theta_phi(th_row, phiS + v, W, K));
            }
            wave_lds_fence();                                            // theta is rewritten by the next sample
            a = group_sum<LG>(a);
            if (l == 0) a_row[s] = c == 0 ? a : a_row[s] + a;            // lane 0 alone touches the tile until it is folded
          }
          wave_lds_fence();                                              // the counts are rewritten by the next chunk
        }
        if (!active) continue;
        wave_lds_fence();
        for (int s = 0; s < ts; ++s) st.take(t0 + s, a_row[s]);
        wave_lds_fence();                                                // the tile is rewritten by the next one
      }
      if (!active) continue;
    }
    tot = group_sum<LG>(tot);
    lg = group_sum<LG>(lg);
    if (l == 0) st.store(out, nrows, n, S, tot, score_lfact(tot) - lg);
  }
}

}  // namespace gdrf
