// The vocabulary-streamed row form (gdrf_set_rows_form(ctx, 1)): the per-row terms that touch the vocabulary, for any V.
//
// Per row n the likelihood needs (rows_lds.h: elbo_rows_kernel for the arithmetic)
//   p_v = sum_k theta_k phi_kv ;  ph_v = p_v / sum_v p_v clamped to [eps, 1 - eps] ;  sum_v w_v log ph_v ;
//   pbar_v = w_v / p_v (0 where the clamp is active) ;  thetabar_k = sum_v phi_kv pbar_v ;  Phi-bar_kv += theta_k pbar_v.
// The LDS forms keep all of Phi (K x V) and its gradient in LDS.  Here a workgroup owns 64 rows at a time and keeps only their theta
// (K x 64) resident; Phi streams through LDS in tiles of VT words (64 for float, 32 for double) and each count is read once.  The
// normaliser is sum_k theta_k rowsum_k with rowsum_k = sum_v phi_kv formed once per call (vs_rowsum_kernel), so the clamp test needs no
// second sweep.  thetabar accumulates across the tiles in registers (lane = row, topics wave + 4 j); Phi-bar accumulates in the
// workgroup's own K x V slot of a partial buffer (read-modify-write, no atomics) over a capped grid, and reduce_parts_kernel adds the
// slots in a fixed order: bit-identical from run to run.
//
// One kernel, four uses (MODE):
//   VS_SOFTMAX  src = mu (K, n): theta = softmax(mu); after the sweep the softmax pull-back around the dominant topic (the same
//               cancellation-free form as elbo_rows_kernel) -> dst = mubar (K, n).  The V-free remainder (Normal sites, row-local
//               backward) is rows_sites_kernel (single point) or elbo_rows2_sites_kernel (two points), rows_lds.h.
//   VS_LINK     src = theta (K, n) returned by a caller's link, which need not sum to one -> dst = thetabar_k - cn rowsum_k =
//               sum_v phi_kv w_v / p_v - sum_v w_v / sum_v p_v (sums over the words inside the clamp range), call 1 of gdrf_step_local_link;
//               the constant part of its Phi-bar (- sum_rows theta_k cn) is known only after the sweep: its per-workgroup sums go to cpart
//               and are subtracted after the reduction (vs_sub_rows_kernel).
//   VS_WORDP    src = topic_probs (n, K): dst = p (n, V), gdrf_predict mode 2.
//   VS_PERP     src = topic_probs: sum w log p and sum w per workgroup (dpart[grid][2], accumulated when dacc), gdrf_predict mode 3.
// Offsets into the counts, the outputs and every (K, n) array are 64-bit.
#pragma once
#include "common.h"

namespace gdrf {

enum { VS_SOFTMAX = 0, VS_LINK = 1, VS_WORDP = 2, VS_PERP = 3 };

template <typename T> struct VsCfg {
  static constexpr int RB = 64;                          // rows of a block: one per lane in the thetabar pass
  static constexpr int VT = sizeof(T) == 8 ? 32 : 64;    // words of a Phi tile (double: K = 128 then fits in 120 KB)
  static constexpr int NG = 256 / VT;                    // thread groups of the p and Phi-bar passes (one word column per thread)
  static constexpr int RPT = RB / NG;                    // consecutive rows per thread in the p pass
};

// LDS bytes: scratch 128 | theta K x RB | Phi tile K x VT | pbar RB x (VT + 1) | row state 8 x RB | dominant topic RB ints
template <typename T> static inline size_t vs_lds(int K) {
  using C = VsCfg<T>;
  return 128 + ((size_t)K * C::RB + (size_t)K * C::VT + (size_t)C::RB * (C::VT + 1) + 8 * C::RB) * sizeof(T) + C::RB * sizeof(int);
}

// rowsum[k] = sum_v phi[k][v] (in double, one workgroup per topic)
template <typename T>
__global__ __launch_bounds__(256) void vs_rowsum_kernel(const T* __restrict__ phi, int K, int V, T* __restrict__ rowsum) {
  __shared__ double scratch[16];
  const int k = blockIdx.x;
  double s = 0;
  for (int v = threadIdx.x; v < V; v += blockDim.x) s += (double)phi[(int64_t)k * V + v];
  s = block_sum(s, scratch);
  if (threadIdx.x == 0) rowsum[k] = (T)s;
}

// x[k][v] -= c[k]
template <typename T>
__global__ void vs_sub_rows_kernel(int K, int V, const T* __restrict__ c, T* __restrict__ x) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)K * V) return;
  x[e] -= c[e / V];
}

// KJ: topics per thread in the thetabar pass (4 waves: KJ = 8 for K <= 32, 32 for K <= 128).  src and dst may alias (mu -> mubar in place).
template <typename T, int MODE, int KJ>
__global__ __launch_bounds__(256) void rows_vstream_kernel(
    int64_t nrows, int K, int V, const T* src, int64_t src_sk, int64_t src_sn,
    const int32_t* __restrict__ ws, const T* __restrict__ phi, const T* __restrict__ rowsum,
    T* dst, int64_t dst_ld, double* __restrict__ dpart, int dacc, T* __restrict__ part /*[grid][K*V]*/, T* __restrict__ cpart /*[grid][K]*/) {
  using C = VsCfg<T>;
  constexpr int RB = C::RB, VT = C::VT, NG = C::NG, RPT = C::RPT;
  constexpr bool ELBO = MODE == VS_SOFTMAX || MODE == VS_LINK;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* scratch = reinterpret_cast<double*>(smem);     // [16]
  T* thS = reinterpret_cast<T*>(smem + 128);              // [K][RB]  theta, topic-major
  T* phS = thS + (size_t)K * RB;                          // [K][VT]  Phi tile
  T* pbS = phS + (size_t)K * VT;                          // [RB][VT + 1] pbar of the tile
  T* rwS = pbS + RB * (VT + 1);                           // [8][RB]: 1 / sum p | sum of unclamped w (link) | cref or cn | 4 partial dots
  int* kdS = reinterpret_cast<int*>(rwS + 8 * RB);        // [RB] dominant topic
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int vl = tid % VT, grp = tid / VT;
  const T feps = t_eps<T>();
  double s_a = 0, s_b = 0;                                // ELBO: sum w log ph ; perplexity: sum w log p, sum w
  T cacc = 0;                                             // link: sum_rows theta_k cn of topic k = tid
  const int64_t KV = (int64_t)K * V;
  T* mypart = ELBO ? part + (int64_t)blockIdx.x * KV : nullptr;
  const int64_t nblk = (nrows + RB - 1) / RB;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const bool first = blk == blockIdx.x;
    const int64_t n0 = blk * RB;
    // theta of the block's rows, one thread per row (coalesced over the rows for the (K, n) layouts)
    if (tid < RB) {
      const int64_t n = n0 + tid;
      if (n < nrows) {
        if constexpr (MODE == VS_SOFTMAX) {
          T mx = -3.0e38f;
          for (int k = 0; k < K; ++k) { const T m = src[(int64_t)k * src_sk + n * src_sn]; thS[k * RB + tid] = m; mx = fmax(mx, m); }
          T se = 0;
          for (int k = 0; k < K; ++k) { const T e = t_exp<T>(thS[k * RB + tid] - mx); thS[k * RB + tid] = e; se += e; }
          const T ise = T(1) / se;
          T ps = 0, tmax = -1;
          int kd = 0;
          for (int k = 0; k < K; ++k) {
            const T th = thS[k * RB + tid] * ise;
            thS[k * RB + tid] = th;
            ps += th * rowsum[k];
            if (th > tmax) { tmax = th; kd = k; }
          }
          rwS[tid] = T(1) / ps; kdS[tid] = kd;
        } else {
          T ps = 0;
          for (int k = 0; k < K; ++k) {
            const T th = src[(int64_t)k * src_sk + n * src_sn];
            thS[k * RB + tid] = th;
            if constexpr (ELBO) ps += th * rowsum[k];
          }
          if constexpr (ELBO) rwS[tid] = T(1) / ps;
        }
      } else {
        for (int k = 0; k < K; ++k) thS[k * RB + tid] = 0;
        rwS[tid] = 0; kdS[tid] = 0;
      }
      rwS[RB + tid] = 0;
    }
    T tb[ELBO ? KJ : 1];
#pragma unroll
    for (int j = 0; j < (ELBO ? KJ : 1); ++j) tb[j] = 0;
    __syncthreads();
    for (int64_t v0 = 0; v0 < V; v0 += VT) {
      for (int e = tid; e < K * VT; e += 256) {
        const int k = e / VT;
        const int64_t v = v0 + (e - k * VT);
        phS[e] = v < V ? phi[(int64_t)k * V + v] : T(0);
      }
      __syncthreads();
      // p of rows grp * RPT + i, word v0 + vl
      const int64_t v = v0 + vl;
      const int r0 = grp * RPT;
      T p[RPT];
#pragma unroll
      for (int i = 0; i < RPT; ++i) p[i] = 0;
      for (int k = 0; k < K; ++k) {
        const T f = phS[k * VT + vl];
#pragma unroll
        for (int i = 0; i < RPT; ++i) p[i] += thS[k * RB + r0 + i] * f;
      }
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        const int r = r0 + i;
        const int64_t n = n0 + r;
        const bool ok = n < nrows && v < V;
        if constexpr (MODE == VS_WORDP) {
          if (ok) dst[n * dst_ld + v] = p[i];
        } else if constexpr (MODE == VS_PERP) {
          if (ok) { const double w = (double)ws[n * V + v]; s_a += w * (double)t_log<T>(p[i]); s_b += w; }
        } else {
          T pb = 0, wi = 0;
          if (ok) {
            const T ph = p[i] * rwS[r];
            const T wt = (T)ws[n * V + v];
            const bool inr = (ph > feps) && (ph < T(1) - feps);
            const T phc = fmin(fmax(ph, feps), T(1) - feps);
            s_a += (double)(wt * t_log<T>(phc));
            pb = inr ? wt / p[i] : T(0);
            wi = inr ? wt : T(0);
          }
          pbS[r * (VT + 1) + vl] = pb;
          if constexpr (MODE == VS_LINK) {          // sum of the unclamped counts of row r: the VT lanes of its group, one writer
#pragma unroll
            for (int o = VT / 2; o >= 1; o >>= 1) wi += __shfl_xor(wi, o, 64);
            if (vl == 0) rwS[RB + r] += wi;
          }
        }
      }
      if constexpr (ELBO) {
        __syncthreads();
        // thetabar of row `lane`, topics wv + 4 j
        for (int jv = 0; jv < VT; ++jv) {
          const T pbv = pbS[lane * (VT + 1) + jv];
#pragma unroll
          for (int j = 0; j < KJ; ++j) { const int k = wv + 4 * j; if (k < K) tb[j] += phS[k * VT + jv] * pbv; }
        }
        // Phi-bar of word v, topics grp + NG j, summed over the block's rows into the workgroup's slot
        if (v < V)
          for (int k = grp; k < K; k += NG) {
            T s = 0;
            for (int r = 0; r < RB; ++r) s += thS[k * RB + r] * pbS[r * (VT + 1) + vl];
            T* d = mypart + (int64_t)k * V + v;
            *d = first ? s : *d + s;
          }
      }
      __syncthreads();
    }
    if constexpr (MODE == VS_SOFTMAX) {
      // mubar_k = theta_k ((thetabar_k - cref) + sum_j theta_j (cref - thetabar_j)), cref = thetabar of the dominant topic
      const int kd = kdS[lane];
#pragma unroll
      for (int j = 0; j < KJ; ++j) if (wv + 4 * j == kd) rwS[2 * RB + lane] = tb[j];
      __syncthreads();
      const T cref = rwS[2 * RB + lane];
      T d = 0;
#pragma unroll
      for (int j = 0; j < KJ; ++j) { const int k = wv + 4 * j; if (k < K) d += thS[k * RB + lane] * (cref - tb[j]); }
      rwS[(4 + wv) * RB + lane] = d;
      __syncthreads();
      const T dot = ((rwS[4 * RB + lane] + rwS[5 * RB + lane]) + rwS[6 * RB + lane]) + rwS[7 * RB + lane];
      const int64_t n = n0 + lane;
      if (n < nrows) {
#pragma unroll
        for (int j = 0; j < KJ; ++j) {
          const int k = wv + 4 * j;
          if (k < K) dst[(int64_t)k * dst_ld + n] = thS[k * RB + lane] * ((tb[j] - cref) + dot);
        }
      }
      __syncthreads();
    } else if constexpr (MODE == VS_LINK) {
      const int64_t n = n0 + lane;
      const T cn = rwS[RB + lane] * rwS[lane];           // d/dp_v' of -sum_v w_v log(sum p), the same for every v'
      if (n < nrows) {
#pragma unroll
        for (int j = 0; j < KJ; ++j) {
          const int k = wv + 4 * j;
          if (k < K) dst[(int64_t)k * dst_ld + n] = tb[j] - cn * rowsum[k];
        }
      }
      if (wv == 0) rwS[2 * RB + lane] = cn;
      __syncthreads();
      if (tid < K) for (int r = 0; r < RB; ++r) cacc += thS[tid * RB + r] * rwS[2 * RB + r];
      __syncthreads();
    }
  }
  if constexpr (ELBO) {
    dpart_store<DP_LOGLIK>(dpart, scratch, 0, s_a, 0, 0);
    if constexpr (MODE == VS_LINK) { if (tid < K) cpart[(int64_t)blockIdx.x * K + tid] = cacc; }
  } else if constexpr (MODE == VS_PERP) {
    dpart_store2(dpart, scratch, s_a, s_b, dacc);
  }
}

}  // namespace gdrf
