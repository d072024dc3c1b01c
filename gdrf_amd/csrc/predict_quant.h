// Credible-interval, exceedance and dominant-topic maps (gdrf_predict_quant): for row n and the S draws of the guide that gdrf_predict_mc
// makes,
//   mu[s][k] = f_loc[k][n] + mean[k][n] + f_var[k][n] eps[s][k][n]   (f_var as the SCALE),  theta_s = softmax_k(mu[s])
// a component c of the row is a topic, x_s = theta_s[c], or a chosen word v = words[c] (no list: v = c), x_s = sum_k theta_s[k] Phi[k][v]
// in T with k ascending (theta_phi of lane_group.h, Phi read from global memory: the chosen columns stay in the caches).
//   QUANT_Q         out (Q, n, C): the type-7 sample quantile of x_0 .. x_{S-1} per level.  The host hands (lo, frac) per level
//                   (lo = floor(q (S - 1)), frac = q (S - 1) - lo, in double), the kernel returns x_(lo) + frac (x_(hi) - x_(lo)) in double,
//                   hi = min(lo + 1, S - 1), x_(r) the r-th order statistic: no rank is decided on the device
//   QUANT_EXCEED    out (Tn, n, C): #{s : x_s > tau} / S per threshold, strict, the integer count divided once in double
//   QUANT_DOMINANT  out (n, K): #{s : argmax_k theta_s = k} / S, ties to the lower topic (group_argmax), topics only
//
// A group of LG lanes owns a row as in predict_mc_kernel and predict_info_kernel: the row prior, the draws (the same counter (global row,
// topic, s), hence the same bits) and the softmax are those of lane_group.h and philox_normal, so x_s of a topic is bit for bit what
// MC_THETA stores.  A word's x_s: theta goes through the group's LDS slots and the group's lanes stride over the chosen words.
//
// EXCEED and DOMINANT keep integer counters in registers (two 16-bit counts to a register: S <= 65535) and store nothing: a lane counts
// for the topics it holds, or for QUANT_WJ words per pass over the draws (more chosen words: the draws are regenerated per pass, as
// predict_info regenerates them per chunk of Phi).
//
// QUANT needs a component's S samples side by side.  A pass of the workgroup handles RP rows (the groups g < RP; RP <= 256 / LG, the
// others idle through the pass) and CP components per row (forms.h::quant_plan): the samples go to LDS as
//   [row][comp][P + 1]  T,  P = S rounded up to a power of two, the tail up to P +inf,  row stride CP (P + 1) + LG
// (the odd component stride spreads the lanes of a group, which store sample s of neighbouring topics at once, over neighbouring banks
// instead of one; the LG elements between rows stagger the groups of a wave, which walk their rows in step, when CP (P + 1) is a
// multiple of the bank count) and are ordered in place by a bitonic network that the owning group runs, lane l on the compare-exchange
// pairs l, l + LG, ...; every exchange is private to the group, hence to a wave: the stages are separated by wave_lds_fence and the
// kernel has no barrier at all.  The ranks lo / hi of every level are then read back.
// More components than CP: further passes, each regenerating the draws.
//
// Nothing about a row depends on another row, on the grid or on how the rows are cut into calls; no atomics, no cross-row reduction.
#pragma once
#include "common.h"
#include "kernels_n.h"
#include "lane_group.h"

#ifndef GDRF_QUANT_MAX_SAMPLES     // include/gdrf_hip.h declares them too
#define GDRF_QUANT_MAX_SAMPLES 1024
#define GDRF_QUANT_MAX_LEVELS 16
#endif

namespace gdrf {

enum { QUANT_Q = 0, QUANT_EXCEED = 1, QUANT_DOMINANT = 2 };
constexpr int QUANT_NL = GDRF_QUANT_MAX_LEVELS;
constexpr int QUANT_WJ = 4;        // words a lane counts for in one pass of EXCEED

// the levels of a call, by value: v = frac (QUANT_Q) or tau (QUANT_EXCEED), lo = the lower rank (QUANT_Q)
struct QuantLevels { double v[QUANT_NL]; int lo[QUANT_NL]; };

// The exceedance counters of one component: a count is at most S <= 65535, so the thresholds 2 i and 2 i + 1 share a register
__device__ __forceinline__ void quant_count_clear(uint32_t (&cnt)[QUANT_NL / 2]) {
#pragma unroll
  for (int i = 0; i < QUANT_NL / 2; ++i) cnt[i] = 0;
}
__device__ __forceinline__ void quant_count(uint32_t (&cnt)[QUANT_NL / 2], double x, const QuantLevels& lev, int nlev) {
#pragma unroll
  for (int i = 0; i < QUANT_NL / 2; ++i)
    cnt[i] += (uint32_t)(2 * i < nlev && x > lev.v[2 * i]) | ((uint32_t)(2 * i + 1 < nlev && x > lev.v[2 * i + 1]) << 16);
}
__device__ __forceinline__ uint32_t quant_count_of(const uint32_t (&cnt)[QUANT_NL / 2], int t) { return (cnt[t / 2] >> (16 * (t & 1))) & 0xffffu; }

// dynamic LDS: theta [256 / LG][LG KJ] | samples [RP][CP (P + 1) + LG] (QUANT_Q only)
template <typename T> inline size_t quant_theta_lds(int LG, int KJ) { return (size_t)(256 / LG) * LG * KJ * sizeof(T); }

// the lower index of pair p of a stage with partner distance j (a power of two): p with a zero bit inserted at j
__device__ __forceinline__ int quant_pair_low(int p, int j) { return ((p & ~(j - 1)) << 1) | (p & (j - 1)); }

// ascending bitonic network over x[0 .. P), P a power of two, run by the LG lanes of the owning group
template <typename T, int LG> __device__ __forceinline__ void group_bitonic_sort(T* x, int P, int l) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = l; p < P / 2; p += LG) {
        const int i = quant_pair_low(p, j), ip = i | j;
        const T a = x[i], b = x[ip];
        if ((a > b) == ((i & k) == 0)) { x[i] = b; x[ip] = a; }
      }
      wave_lds_fence();
    }
  }
}

template <typename T, int LG, int KJ>
__global__ __launch_bounds__(256) void predict_quant_kernel(
    int mode, int64_t nrows, int K, int V, int S, const Hyper* __restrict__ h, const T* __restrict__ qpart, int nqpart, const T* __restrict__ loc,
    const T* __restrict__ tt, int64_t ldk, const T* __restrict__ mean, int64_t mean_sk, int64_t mean_sn, const T* __restrict__ eps,
    uint64_t seed, int64_t row_offset, const T* __restrict__ phi, const int32_t* __restrict__ words, int C, bool use_words, int nlev,
    QuantLevels lev, int RP, int CP, int P, double* __restrict__ out) {
  constexpr int RPB = 256 / LG, Kp = LG * KJ;
  extern __shared__ __attribute__((aligned(16))) char quant_smem[];
  T* thS = reinterpret_cast<T*>(quant_smem);
  T* xS = thS + RPB * Kp;
  const int tid = threadIdx.x, l = tid % LG, g = tid / LG;
  T* th_row = thS + g * Kp;
  const int rows = mode == QUANT_Q ? RP : RPB;                 // rows of a workgroup pass
  const int PS = P + 1;                                        // the component stride
  T* x_row = xS + (size_t)g * ((size_t)CP * PS + LG);          // QUANT_Q, g < RP only
  const T var0 = (T)h->var;
  const double dS = (double)S;
  const int64_t nblk = (nrows + rows - 1) / rows;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t n = blk * rows + g;
    if (g >= rows || n >= nrows) continue;                     // the lanes of a group leave together; nothing below is shared between groups
    const T v0 = row_prior_v0(qpart, nqpart, ldk, n, var0);
    T m[KJ], sd[KJ];
#pragma unroll
    for (int j = 0; j < KJ; ++j) {
      const int k = l + LG * j;
      m[j] = sd[j] = 0;
      if (k < K) row_prior_topic(v0, loc, tt, ldk, mean, mean_sk, mean_sn, k, n, m[j], sd[j]);
    }
    // theta of sample s, as predict_mc_kernel forms it
    auto draw = [&](int s, T (&th)[KJ]) {
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
    };
    // theta into the group's LDS slots, for the lanes that stride over words; the caller fences again before the next sample
    auto share = [&](const T (&th)[KJ]) {
#pragma unroll
      for (int j = 0; j < KJ; ++j) { const int k = l + LG * j; if (k < K) th_row[k] = th[j]; }
      wave_lds_fence();
    };
    auto word_of = [&](int c) -> int64_t { return words ? (int64_t)words[c] : (int64_t)c; };

    if (mode == QUANT_DOMINANT) {
      int cnt[KJ];
#pragma unroll
      for (int j = 0; j < KJ; ++j) cnt[j] = 0;
      for (int s = 0; s < S; ++s) {
        T th[KJ];
        draw(s, th);
        T val = T(-1); int idx = INT32_MAX;                    // a lane without a topic never wins: theta >= 0
#pragma unroll
        for (int j = 0; j < KJ; ++j) { const int k = l + LG * j; if (k < K && th[j] > val) { val = th[j]; idx = k; } }
        group_argmax<LG>(val, idx);
#pragma unroll
        for (int j = 0; j < KJ; ++j) cnt[j] += (idx == l + LG * j);
      }
#pragma unroll
      for (int j = 0; j < KJ; ++j) { const int k = l + LG * j; if (k < K) out[n * K + k] = (double)cnt[j] / dS; }
    } else if (mode == QUANT_EXCEED && !use_words) {
      uint32_t cnt[KJ][QUANT_NL / 2];
#pragma unroll
      for (int j = 0; j < KJ; ++j) quant_count_clear(cnt[j]);
      for (int s = 0; s < S; ++s) {
        T th[KJ];
        draw(s, th);
#pragma unroll
        for (int j = 0; j < KJ; ++j) quant_count(cnt[j], (double)th[j], lev, nlev);
      }
#pragma unroll
      for (int j = 0; j < KJ; ++j) {
        const int k = l + LG * j;
#pragma unroll
        for (int t = 0; t < QUANT_NL; ++t)
          if (k < K && t < nlev) out[((int64_t)t * nrows + n) * C + k] = (double)quant_count_of(cnt[j], t) / dS;
      }
    } else if (mode == QUANT_EXCEED) {
      for (int c0 = 0; c0 < C; c0 += LG * QUANT_WJ) {          // a pass: QUANT_WJ words per lane, the draws regenerated
        uint32_t cnt[QUANT_WJ][QUANT_NL / 2];
        const T* col[QUANT_WJ];
#pragma unroll
        for (int w = 0; w < QUANT_WJ; ++w) {
          const int c = c0 + l + LG * w;
          col[w] = c < C ? phi + word_of(c) : nullptr;
          quant_count_clear(cnt[w]);
        }
        for (int s = 0; s < S; ++s) {
          T th[KJ];
          draw(s, th);
          share(th);
#pragma unroll
          for (int w = 0; w < QUANT_WJ; ++w) {
            if (!col[w]) continue;
            quant_count(cnt[w], (double)theta_phi(th_row, col[w], (int64_t)V, K), lev, nlev);
          }
          wave_lds_fence();                                    // theta is rewritten by the next sample
        }
#pragma unroll
        for (int w = 0; w < QUANT_WJ; ++w) {
          const int c = c0 + l + LG * w;
#pragma unroll
          for (int t = 0; t < QUANT_NL; ++t)
            if (c < C && t < nlev) out[((int64_t)t * nrows + n) * C + c] = (double)quant_count_of(cnt[w], t) / dS;
        }
      }
    } else {
      for (int c0 = 0; c0 < C; c0 += CP) {                     // a pass: the samples of cp components into LDS, the draws regenerated
        const int cp = min(CP, C - c0);
        for (int s = 0; s < S; ++s) {
          T th[KJ];
          draw(s, th);
          if (use_words) {
            share(th);
            for (int cc = l; cc < cp; cc += LG) x_row[(size_t)cc * PS + s] = theta_phi(th_row, phi + word_of(c0 + cc), (int64_t)V, K);
            wave_lds_fence();                                  // theta is rewritten by the next sample
          } else {
#pragma unroll
            for (int j = 0; j < KJ; ++j) {
              const int k = l + LG * j;
              if (k >= c0 && k < c0 + cp) x_row[(size_t)(k - c0) * PS + s] = th[j];
            }
          }
        }
        for (int e = l; e < cp * (P - S); e += LG) {           // the tail of every component: +inf
          const int cc = e / (P - S);
          x_row[(size_t)cc * PS + S + (e - cc * (P - S))] = T(INFINITY);
        }
        wave_lds_fence();
        for (int cc = 0; cc < cp; ++cc) group_bitonic_sort<T, LG>(x_row + (size_t)cc * PS, P, l);
        for (int e = l; e < cp * nlev; e += LG) {
          const int cc = e / nlev, t = e - cc * nlev;
          const int lo = lev.lo[t], hi = min(lo + 1, S - 1);
          const double a = (double)x_row[(size_t)cc * PS + lo], b = (double)x_row[(size_t)cc * PS + hi];
          out[((int64_t)t * nrows + n) * C + c0 + cc] = a + lev.v[t] * (b - a);
        }
        wave_lds_fence();                                      // the samples are rewritten by the next pass
      }
    }
  }
}

}  // namespace gdrf
