// Per-location entropy and information-gain maps (gdrf_predict_info): for row n and the S draws of the guide that gdrf_predict_mc makes,
//   mu[s][k] = f_loc[k][n] + mean[k][n] + f_var[k][n] eps[s][k][n]   (f_var as the SCALE),  theta_s = softmax_k(mu[s]),  p_s = theta_s Phi
// and with h(q) = -sum_i q_i log q_i (0 log 0 = 0), theta_bar = (1/S) sum_s theta_s, p_bar = theta_bar Phi (the map is linear):
//   out[0]  topic_entropy           h(theta_bar)
//   out[1]  topic_expected_entropy  (1/S) sum_s h(theta_s)
//   out[2]  topic_information       out[0] - out[1]
//   out[3]  word_entropy            h(p_bar)
//   out[4]  word_expected_entropy   (1/S) sum_s h(p_s)
//   out[5]  word_information        out[3] - out[4]
// out is (6, n) double.  The two information values are the Jensen-Shannon divergences of the S sampled distributions - the Monte-Carlo
// estimate of the mutual information between one token's topic (word) at x and the latent field there - and are returned as computed,
// not clamped: 0 <= out[5] <= out[2] <= log min(K, S) up to rounding.
//
// A group of LG lanes owns a row as in predict_mc_kernel: the row prior, the draws (the same counter (global row, topic, s), hence the same
// bits) and the softmax are those of lane_group.h and philox_normal.  theta_bar is accumulated as MC_MOMENTS accumulates its mean (in
// double, shifted by the first sample, rounded to T): it is bit for bit that mean.  The word part: the row's current theta goes through
// the group's LDS slots and the group's lanes stride over QUADS of consecutive words - one 4-wide LDS read of Phi per topic and quad -,
// p_v = sum_k theta_k Phi[k][v] (k ascending) and p_v log p_v in T, a p_v <= 0 adds nothing, the sums in double per lane and one
// butterfly over the group per row at the end.
//
// V is not limited by LDS: Phi is staged in chunks of GDRF_INFO_V_CHUNK words, [K][W] with W = min(V, chunk) rounded up to a quad and
// the padding zero (so it adds nothing).  One chunk (V <= GDRF_INFO_V_CHUNK) is staged once per workgroup.  More: for every pass of the
// workgroup over its rows the chunks are staged in turn and theta_s is REGENERATED for every chunk (the draws are counter-based; an
// injected eps is read again), the topic sums are taken on the first chunk only; word_entropy is a last pass over the chunks from
// theta_bar.  The staging is the only thing the workgroup does together: the row loop is uniform over the workgroup and a group
// without a row (past the end) only joins the barriers.  Nothing about a row depends on another row, on the grid or on how the rows
// are cut into calls; no atomics, no cross-row reduction, no sample stored.
#pragma once
#include "common.h"
#include "kernels_n.h"
#include "lane_group.h"

#ifndef GDRF_INFO_V_CHUNK      // include/gdrf_hip.h declares it too: the words of Phi staged in LDS at a time (K = 128 in double: 128 KB)
#define GDRF_INFO_V_CHUNK 128
#endif

namespace gdrf {

template <typename T> using InfoQuad = T __attribute__((ext_vector_type(4)));

// the row stride of the staged Phi chunk: min(V, chunk) rounded up to a quad
inline int info_chunk_stride(int V) { return (std::min(V, (int)GDRF_INFO_V_CHUNK) + 3) / 4 * 4; }
// dynamic LDS: Phi chunk [K][W] | theta [rows][LG KJ], rows = 256 / LG
template <typename T> inline size_t info_lds(int K, int V, int LG, int KJ) {
  return ((size_t)K * info_chunk_stride(V) + (size_t)(256 / LG) * LG * KJ) * sizeof(T);
}

// x log x in T, widened; 0 for x <= 0
template <typename T> __device__ __forceinline__ double info_xlogx(T x) { return x > T(0) ? (double)(x * t_log<T>(x)) : 0.0; }

// this lane's share of sum_v p_v log p_v over the cw words of the staged chunk, p = th_row Phi
template <typename T, int LG> __device__ __forceinline__ double info_chunk_plogp(const T* th_row, const T* phiS, int W4, int cw, int K, int l) {
  const InfoQuad<T>* ph = reinterpret_cast<const InfoQuad<T>*>(phiS);
  double a = 0;
  for (int q = l; 4 * q < cw; q += LG) {
    InfoQuad<T> p = T(0);
    for (int k = 0; k < K; ++k) p += th_row[k] * ph[k * W4 + q];
    a += info_xlogx<T>(p.x) + info_xlogx<T>(p.y) + info_xlogx<T>(p.z) + info_xlogx<T>(p.w);
  }
  return a;
}

template <typename T, int LG, int KJ>
__global__ __launch_bounds__(256) void predict_info_kernel(
    int64_t nrows, int K, int V, int S, const Hyper* __restrict__ h, const T* __restrict__ qpart, int nqpart, const T* __restrict__ loc,
    const T* __restrict__ tt, int64_t ldk, const T* __restrict__ mean, int64_t mean_sk, int64_t mean_sn, const T* __restrict__ eps,
    uint64_t seed, int64_t row_offset, const T* __restrict__ phi, double* __restrict__ out) {
  constexpr int RPB = 256 / LG, Kp = LG * KJ, VC = GDRF_INFO_V_CHUNK;
  extern __shared__ __attribute__((aligned(32))) char info_smem[];
  const int W = (min(V, VC) + 3) / 4 * 4, W4 = W / 4;
  T* phiS = reinterpret_cast<T*>(info_smem);
  T* thS = phiS + (size_t)K * W;
  const int tid = threadIdx.x, l = tid % LG, g = tid / LG;
  T* th_row = thS + g * Kp;
  const int nchunk = (V + VC - 1) / VC;
  // chunk c of Phi into LDS, zero past its last word; more than one chunk: behind a barrier (the previous one may still be read) and
  // before one.  Returns the chunk's words.
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
  if (nchunk == 1) { stage(0); __syncthreads(); }
  const T var0 = (T)h->var;
  const double is = 1.0 / (double)S;
  const int64_t nblk = (nrows + RPB - 1) / RPB;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {         // uniform over the workgroup: every group joins the barriers
    const int64_t n = blk * RPB + g;
    const bool active = n < nrows;                                       // the lanes of a group agree
    T m[KJ], sd[KJ], t0[KJ];
    double d1[KJ];
#pragma unroll
    for (int j = 0; j < KJ; ++j) { m[j] = sd[j] = t0[j] = 0; d1[j] = 0; }
    if (active) {
      const T v0 = row_prior_v0(qpart, nqpart, ldk, n, var0);
#pragma unroll
      for (int j = 0; j < KJ; ++j) {
        const int k = l + LG * j;
        if (k < K) row_prior_topic(v0, loc, tt, ldk, mean, mean_sk, mean_sn, k, n, m[j], sd[j]);
      }
    }
    double ht = 0, hw = 0;                                               // this lane's sums over s of sum theta log theta, sum p log p
    for (int c = 0; c < nchunk; ++c) {
      const int cw = nchunk > 1 ? stage(c) : V;
      if (!active) continue;
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
        group_softmax<LG>(th, l, K);
        if (c == 0) {
#pragma unroll
          for (int j = 0; j < KJ; ++j) {
            if (s == 0) t0[j] = th[j];
            d1[j] += (double)th[j] - (double)t0[j];
            ht += info_xlogx<T>(th[j]);
          }
        }
#pragma unroll
        for (int j = 0; j < KJ; ++j) { const int k = l + LG * j; if (k < K) th_row[k] = th[j]; }
        wave_lds_fence();
        hw += info_chunk_plogp<T, LG>(th_row, phiS, W4, cw, K, l);
        wave_lds_fence();                                                // theta is rewritten by the next sample
      }
    }
    // theta_bar as MC_MOMENTS rounds its mean, its entropy, and the last pass over the chunks for h(theta_bar Phi)
    double hbt = 0, hbw = 0;
    if (active) {
#pragma unroll
      for (int j = 0; j < KJ; ++j) {
        const int k = l + LG * j;
        if (k < K) {
          const T tb = (T)((double)t0[j] + d1[j] * is);
          hbt += info_xlogx<T>(tb);
          th_row[k] = tb;
        }
      }
    }
    for (int c = 0; c < nchunk; ++c) {
      const int cw = nchunk > 1 ? stage(c) : V;                         // its barriers also order theta_bar's writes; one chunk: the fence below
      if (!active) continue;
      wave_lds_fence();
      hbw += info_chunk_plogp<T, LG>(th_row, phiS, W4, cw, K, l);
    }
    if (!active) continue;
    wave_lds_fence();                                                    // theta_bar is rewritten by the next row's first sample
    ht = group_sum<LG>(ht); hw = group_sum<LG>(hw); hbt = group_sum<LG>(hbt); hbw = group_sum<LG>(hbw);
    if (l == 0) {
      const double te = -hbt, tx = -ht * is, we = -hbw, wx = -hw * is;
      out[n] = te; out[nrows + n] = tx; out[2 * nrows + n] = te - tx;
      out[3 * nrows + n] = we; out[4 * nrows + n] = wx; out[5 * nrows + n] = we - wx;
    }
  }
}

}  // namespace gdrf
