// Posterior-predictive count samples (gdrf_sample_counts): for sample s, row n, with theta[s][n][:] a draw of the topic proportions
//   p[s][n][v] = sum_k theta[s][n][k] Phi[k][v]                          (array precision, as MC_SCORE of predict_mc.h forms it)
//   c[s][n][v] = p[s][n][0] + ... + p[s][n][v]                            (inclusive prefix sum, accumulated in double)
//   word(s,n,t) = the smallest v with u[s][n][t] * c[s][n][V-1] < c[s][n][v]   (compared in double),  t = 0 .. T_n - 1
//   w_rep[s][n][v] = #{ t : word(s,n,t) = v }
// Scaling by c[V-1] means theta and Phi need not sum to one to the last bit; the strict inequality means a word with p = 0 is never
// drawn; a row with T_n = 0 gives zeros.  (A product u c[V-1] that rounds up to c[V-1] - an injected u within 2^-53 of one - is taken
// as the largest double below c[V-1]: the last word with p > 0.)
//
// u is either an injected (S, n, Tmax) double array or generated inline: Philox4x32-10 (philox_round, kernels_n.h) keyed by the seed with
// counter (global row = row_offset + n, 2^31 | token block t / 4, sample s); word t % 4 of the block gives u = (word + 0.5) / 2^32 in
// double.  philox_normal's counter is (global row, topic k, step) with k <= 128: the top bit of the third word keeps the token draws of
// a seed apart from the normals that drew theta under the same seed.  sc_fill_uniforms_kernel writes exactly these numbers.
//
// A WAVE owns a (row, sample) pair (V <= GDRF_SC_WAVE_V; above it the whole workgroup does, see the forms below); blockIdx.y is the
// sample, the owners of one sample stride over the rows.  Per owner in LDS: the CDF (V doubles), the counts (V int32), theta; SC_STATS
// also keeps p.  Lanes over the words form p from Phi (in LDS while four workgroups still fit a CU, else from global memory, where it
// stays in L2) and store it as a double; the prefix sum runs over 64 contiguous chunks, one per lane of ONE wave: chunk sums from zero,
// the chunk offsets by a serial sum over the 64 lanes (every lane the same bits), c[v] = offset + the chunk's running sum.  That order
// makes c non-decreasing to the bit (x -> fl(a + x) is monotone and a chunk's last value IS the next offset), which the binary search
// needs to be well defined.  Lanes over blocks of four tokens then draw, search the CDF and add into the counts with integer LDS
// atomics (order-independent, so deterministic); lanes over the words store.  Between the phases of a wave-owned pair stands
// wave_lds_fence (lane_group.h), not a barrier.
//   SC_COUNTS    out (S, n, V) int32: w_rep
//   SC_STATS     the check statistics of the same draws, no replicate stored: with q = p / c[V-1] in double,
//                dev_rep[s] = 2 sum_n sum_{v: w_rep > 0} w_rep log(w_rep / (T_n q_v)), dev_obs[s] the same for the observed counts ws[n]
//                with T_n = sum_v ws[n][v]; zeros[s][v] = #{ n : w_rep[s][n][v] = 0 } as int64.  The two sums: lane partials in double,
//                per-workgroup partials dpart[s][grid][2], summed in a fixed order by sc_reduce_kernel - no float atomics.  zeros: per
//                workgroup in LDS, one 64-bit integer atomic per word and workgroup - exact, whatever the order.
// Nothing about a (row, sample) pair depends on another pair or on the grid.
#pragma once
#include "common.h"
#include "kernels_n.h"
#include "lane_group.h"

namespace gdrf {

enum { SC_COUNTS = 0, SC_STATS = 1, SC_UNIFORMS = 2 };
#ifndef GDRF_SC_MAX_V          // include/gdrf_hip.h declares it too: the words a call serves (one wave's CDF, counts and p in double, 80 KB, fit a CU's LDS)
#define GDRF_SC_MAX_V 4096
#endif
#define GDRF_SC_KP 128         // theta's LDS slots per wave (K <= 128)

// the four uniforms of token block `blk` (tokens 4 blk .. 4 blk + 3) of (global row gn, sample s)
__device__ __forceinline__ void sc_token_uniforms(uint64_t seed, uint64_t gn, uint32_t blk, uint32_t s, double (&u)[4]) {
  uint32_t c[4] = {(uint32_t)gn, (uint32_t)(gn >> 32), 0x80000000u | blk, s};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) { philox_round(c, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
#pragma unroll
  for (int j = 0; j < 4; ++j) u[j] = ((double)c[j] + 0.5) * (1.0 / 4294967296.0);
}

// u (S, n, tmax) as the kernel below would draw them inline: one thread per (token block, row), blockIdx.y = sample
__global__ void sc_fill_uniforms_kernel(uint64_t seed, int64_t row_offset, int64_t nrows, int tmax, double* __restrict__ u) {
  const int nb = (tmax + 3) / 4;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nrows * nb) return;
  const int64_t n = i / nb;
  const int b = (int)(i - n * nb), s = blockIdx.y;
  double r[4];
  sc_token_uniforms(seed, (uint64_t)(n + row_offset), (uint32_t)b, (uint32_t)s, r);
  double* dst = u + ((int64_t)s * nrows + n) * tmax;
#pragma unroll
  for (int j = 0; j < 4; ++j) if (4 * b + j < tmax) dst[4 * b + j] = r[j];
}

// dynamic LDS: Phi [K][V] (PHI_LDS) | zeros [Vp] int32 (SC_STATS) | per wave: cdf [Vp] double | counts [Vp] int32 | p [Vp] T (SC_STATS) |
// theta [GDRF_SC_KP] T;  Vp = V rounded up to 4, so that every array starts on 16 bytes
template <typename T> inline size_t sc_wave_lds(int V, int mode) {
  const size_t Vp = (size_t)round_up(V, 4);
  return Vp * (sizeof(double) + sizeof(int32_t) + (mode == SC_STATS ? sizeof(T) : 0)) + GDRF_SC_KP * sizeof(T);
}
template <typename T> inline size_t sc_phi_lds(int K, int V) { return (size_t)round_up((int64_t)K * V * sizeof(T), 16); }
template <typename T> inline size_t sc_lds(int K, int V, int mode, int waves, bool phi_lds) {
  return (phi_lds ? sc_phi_lds<T>(K, V) : 0) + (mode == SC_STATS ? (size_t)round_up(V, 4) * sizeof(int32_t) : 0) + waves * sc_wave_lds<T>(V, mode);
}

// who owns a (row, sample) pair and where Phi is read from: a wave with Phi in LDS, a wave with Phi from global memory, or - for
// V > GDRF_SC_WAVE_V, where a wave's own arrays would leave a CU only a few waves - the whole workgroup (one set of arrays, barriers
// where the wave forms wait, the prefix sum still by the first wave alone: the CDF's bits do not depend on the form)
enum { SC_WAVE_PHI = 0, SC_WAVE = 1, SC_BLOCK = 2 };
#define GDRF_SC_WAVE_V 256

template <typename T, int FORM>
__global__ __launch_bounds__(256) void sample_counts_kernel(
    int mode, int64_t nrows, int K, int V, const T* __restrict__ theta, const T* __restrict__ phi, const int32_t* __restrict__ totals, int tmax,
    const int32_t* __restrict__ ws, uint64_t seed, int64_t row_offset, const double* __restrict__ u, int32_t* __restrict__ out,
    double* __restrict__ dpart, unsigned long long* __restrict__ zeros) {
  constexpr bool BLK = FORM == SC_BLOCK, PHI_LDS = FORM == SC_WAVE_PHI;
  __shared__ double scratch[16];                              // block_sum's; [15]: c[V-1] from the first wave to the others (SC_BLOCK)
  extern __shared__ __attribute__((aligned(16))) char sc_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = blockIdx.y;
  const int gl = BLK ? tid : lane, gsz = BLK ? (int)blockDim.x : 64;           // this thread within the group that owns a pair
  const int units = BLK ? 1 : (int)(blockDim.x >> 6), unit = BLK ? 0 : wave;  // such groups in the workgroup
  const int Vp = (V + 3) & ~3;
  const bool stats = mode == SC_STATS;
  char* base = sc_smem;
  const T* phiS = phi;
  if (PHI_LDS) {
    T* dst = reinterpret_cast<T*>(base);
    for (int e = tid; e < K * V; e += blockDim.x) dst[e] = phi[e];
    phiS = dst;
    base += ((size_t)K * V * sizeof(T) + 15) & ~(size_t)15;
  }
  int32_t* zS = reinterpret_cast<int32_t*>(base);             // SC_STATS: this workgroup's zero counts per word
  if (stats) {
    for (int v = tid; v < V; v += blockDim.x) zS[v] = 0;
    base += (size_t)Vp * sizeof(int32_t);
  }
  base += (size_t)unit * ((size_t)Vp * (sizeof(double) + sizeof(int32_t) + (stats ? sizeof(T) : 0)) + GDRF_SC_KP * sizeof(T));
  double* cdf = reinterpret_cast<double*>(base);
  int32_t* cnt = reinterpret_cast<int32_t*>(cdf + Vp);
  T* pS = reinterpret_cast<T*>(cnt + Vp);
  T* thS = pS + (stats ? Vp : 0);
  if (PHI_LDS || stats) __syncthreads();
  auto phase = [&]() { if (BLK) __syncthreads(); else wave_lds_fence(); };      // a wave-owned pair: the fence; a workgroup-owned one: a barrier

  const int chunk = (V + 63) >> 6, v0 = min(V, lane * chunk), v1 = min(V, v0 + chunk);
  double a_rep = 0, a_obs = 0;
  for (int64_t n = (int64_t)blockIdx.x * units + unit; n < nrows; n += (int64_t)gridDim.x * units) {      // SC_BLOCK: the same trips for every thread
    const int64_t pair = (int64_t)s * nrows + n;
    const int Tn = min(max(totals[n], 0), tmax);
    for (int k = gl; k < K; k += gsz) thS[k] = theta[pair * K + k];
    phase();
    // p in the array precision, held as a double where the prefix sum will stand; the counts start at zero
    for (int v = gl; v < V; v += gsz) {
      T p = 0;
#pragma unroll 4                                                // four Phi loads in flight; the order of the sum stays k = 0, 1, ...
      for (int k = 0; k < K; ++k) p += thS[k] * phiS[(int64_t)k * V + v];
      cdf[v] = (double)p;
      cnt[v] = 0;
      if (stats) pS[v] = p;
    }
    phase();
    double ctot = 0;
    if (!BLK || wave == 0) {
      double tot = 0, off = 0;
      for (int v = v0; v < v1; ++v) tot += cdf[v];
      for (int l = 0; l < 64; ++l) {                            // serial over the lanes: every lane forms the same 64 sums
        if (l == lane) off = ctot;
        ctot += __shfl(tot, l, 64);
      }
      double run = 0;
      for (int v = v0; v < v1; ++v) { run += cdf[v]; cdf[v] = off + run; }
      if (BLK && lane == 0) scratch[15] = ctot;
    }
    phase();
    if (BLK) ctot = scratch[15];
    const double cmax = __longlong_as_double(__double_as_longlong(ctot) - 1);      // the largest double below c[V-1] (c[V-1] > 0)
    const double* urow = u ? u + pair * tmax : nullptr;
    for (int b = gl; 4 * b < Tn; b += gsz) {
      double r[4];
      if (urow) {
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = 4 * b + j < Tn ? urow[4 * b + j] : 0.0;
      } else {
        sc_token_uniforms(seed, (uint64_t)(n + row_offset), (uint32_t)b, (uint32_t)s, r);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (4 * b + j >= Tn) continue;
        double x = r[j] * ctot;
        if (!(x < ctot)) x = cmax;
        int lo = 0, hi = V - 1;                                 // the answer lies in [lo, hi]: c[V-1] = ctot > x
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (x < cdf[mid]) hi = mid; else lo = mid + 1;
        }
        atomicAdd(&cnt[lo], 1);
      }
    }
    phase();
    if (!stats) {
      for (int v = gl; v < V; v += gsz) out[pair * V + v] = cnt[v];
    } else {
      long long tobs = 0;                                       // every wave for itself: the same integer in each
      for (int v = lane; v < V; v += 64) tobs += ws[n * V + v];
      tobs = wave_sum(tobs);
      for (int v = gl; v < V; v += gsz) {
        const int32_t c = cnt[v], w = ws[n * V + v];
        if (c == 0) atomicAdd(&zS[v], 1);
        if (c > 0 || w > 0) {
          const double q = (double)pS[v] / ctot;
          if (c > 0) a_rep += (double)c * log((double)c / ((double)Tn * q));
          if (w > 0) a_obs += (double)w * log((double)w / ((double)tobs * q));
        }
      }
    }
    phase();                                                    // the next pair rewrites theta, the CDF and the counts
  }
  if (stats) {
    const double a = block_sum(2.0 * a_rep, scratch), b = block_sum(2.0 * a_obs, scratch);     // its barriers also end the zero counts
    const int64_t slot = (int64_t)s * gridDim.x + blockIdx.x;
    if (tid == 0) { dpart[2 * slot] = a; dpart[2 * slot + 1] = b; }
    for (int v = tid; v < V; v += blockDim.x)
      if (zS[v]) atomicAdd(&zeros[(int64_t)s * V + v], (unsigned long long)zS[v]);
  }
}

// dev[0][s], dev[1][s] = the sums of the `nparts` per-workgroup partials of sample s = blockIdx.x, in one fixed order
__global__ __launch_bounds__(256) void sc_reduce_kernel(const double* __restrict__ dpart, int nparts, int S, double* __restrict__ dev) {
  __shared__ double scratch[16];
  const int s = blockIdx.x;
  double a = 0, b = 0;
  for (int g = threadIdx.x; g < nparts; g += blockDim.x) {
    a += dpart[2 * ((int64_t)s * nparts + g)];
    b += dpart[2 * ((int64_t)s * nparts + g) + 1];
  }
  a = block_sum(a, scratch);
  b = block_sum(b, scratch);
  if (threadIdx.x == 0) { dev[s] = a; dev[(int64_t)S + s] = b; }
}

}  // namespace gdrf
