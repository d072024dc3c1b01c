// The device helpers of the lane-group row kernels (predict_mc.h, foldin.h, rows_csr.h; predict.h takes the fence and the row prior,
// sample_counts.h the fence).  In these kernels a group of LG lanes owns a row (LG a power of two <= 64, groups aligned, so a group never straddles a
// wave) and lane l holds the topics l, l + LG, ... (KJ of them, LG x KJ >= K).  A workgroup of 256 threads passes over 256 / LG rows at
// a time, tid -> (l, g) = (tid % LG, tid / LG).  Every reduction over a group is a butterfly of shuffles: the same bits in every lane.
#pragma once
#include "common.h"

namespace gdrf {

template <int LG, typename T> __device__ __forceinline__ T group_sum(T v) {
#pragma unroll
  for (int o = LG / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int LG, typename T> __device__ __forceinline__ T group_max(T v) {
#pragma unroll
  for (int o = LG / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
// the largest val of the group and its idx, the lowest idx among equals
template <int LG, typename T> __device__ __forceinline__ void group_argmax(T& val, int& idx) {
#pragma unroll
  for (int o = LG / 2; o > 0; o >>= 1) {
    const T ov = __shfl_xor(val, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > val || (ov == val && oi < idx)) { val = ov; idx = oi; }
  }
}

// What stands between LDS writes of some lanes and LDS reads (or rewrites) of the same words by OTHER lanes of the same wave.  A wave's LDS
// operations complete in the order they were issued, so once the wave has waited for its own outstanding ones every lane sees what every
// other lane of the wave wrote before the wait; the memory clobber keeps the compiler from moving an access across it.  A lane group
// never straddles a wave, hence a group-private (or wave-private) exchange needs this wait and no barrier.  It does NOT order anything
// between waves: an exchange that the whole workgroup takes part in needs __syncthreads() (sample_counts_kernel's SC_BLOCK form takes
// that where its wave forms take this).
__device__ __forceinline__ void wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// x[j] (topic l + LG j) -> softmax over the K topics of the group's row.  The slots past K (l + LG j >= K) take part in the maximum: the
// caller pads them with GROUP_PAD; they come back as 0.  (foldin_kernel's softmax, in double inside its iteration, keeps the mask it has
// in registers instead: it stays written out there.)
constexpr float GROUP_PAD = -3.0e38f;
template <int LG, int KJ, typename T> __device__ __forceinline__ void group_softmax(T (&x)[KJ], int l, int K) {
  T mx = x[0];
#pragma unroll
  for (int j = 1; j < KJ; ++j) mx = fmax(mx, x[j]);
  mx = group_max<LG>(mx);
  T se = 0;
#pragma unroll
  for (int j = 0; j < KJ; ++j) { x[j] = l + LG * j < K ? t_exp<T>(x[j] - mx) : T(0); se += x[j]; }
  se = group_sum<LG>(se);
  const T ise = T(1) / se;
#pragma unroll
  for (int j = 0; j < KJ; ++j) x[j] *= ise;
}

// The prior of row n from the step's forward by-products, the one place that forms it (predict_var_kernel returns it, predict_mc_kernel
// and foldin_kernel start from it): f_var[k][n] = clamp(variance - q_n, 0) + tt[k][n] with q_n the sum of the partial row norms of W
// (row_prior_v0 is the topic-free part), and the location f_loc[k][n] (+ mean[k][n] where a mean is bound).
template <typename T> __device__ __forceinline__ T row_prior_v0(const T* qpart, int nqpart, int64_t ldk, int64_t n, T var) {
  T qn = 0;
  for (int c = 0; c < nqpart; ++c) qn += qpart[(int64_t)c * ldk + n];
  return (var - qn > T(0)) ? var - qn : T(0);
}
// topic k of row n: m = f_loc (+ mean), fv = f_var
template <typename T> __device__ __forceinline__ void row_prior_topic(T v0, const T* loc, const T* tt, int64_t ldk, const T* mean, int64_t mean_sk, int64_t mean_sn,
                                                                   int k, int64_t n, T& m, T& fv) {
  m = loc[(int64_t)k * ldk + n];
  if (mean) m += mean[(int64_t)k * mean_sk + n * mean_sn];
  fv = v0 + tt[(int64_t)k * ldk + n];
}

// p = sum_k theta_k phi_k of one word, in T, summed in the order k = 0, 1, ...: phi_col points at the word's entry of topic 0, consecutive
// topics lie `stride` elements apart (an int for Phi in LDS, an int64_t for Phi in global memory)
template <typename T, typename I> __device__ __forceinline__ T theta_phi(const T* th_row, const T* phi_col, I stride, int K) {
  T p = 0;
  for (int k = 0; k < K; ++k) p += th_row[k] * phi_col[k * stride];
  return p;
}

}  // namespace gdrf
