// The sparse row form: the per-row terms that touch the vocabulary, on a CSR count matrix bound with gdrf_bind_counts_csr.
//
// A zero count adds exactly nothing to any per-row term (rows_vstream.h: 0 * log ph to the log-likelihood, pbar_v = 0 to thetabar and to
// Phi-bar; the normaliser sum_v p_v = sum_k theta_k rowsum_k needs no sweep over the words), so visiting the stored entries alone gives the
// sums of rows_vstream_kernel with nnz x K work instead of n x V x K, and no dense (n, V) array exists anywhere.  The kernels below stand
// in for rows_vstream_kernel in its three modes that read counts (VS_SOFTMAX, VS_LINK, VS_PERP), on the same buffers with the same
// meaning; the V-free kernels around it are those of the streamed form (rows_lds.h).  The arithmetic per stored entry is that of rows_vstream_kernel
// (ph = p / sum p, the clamp to [eps, 1 - eps], pbar = w / p inside the clamp range only, the unclamped count sum of the link mode): the
// two forms differ by summation order only.
//
// Two passes, because the two outputs reduce along different axes:
//   row pass (CSR order), rows_csr_kernel: a group of LG lanes owns a row, lane l holds topics l, l + LG, ... (KJ of them) of theta, of the
//     entry's Phi column and of thetabar.  The group reads LG entries (column, count) at once, one per lane, and walks them with lane
//     broadcasts; per entry p = sum_k theta_k phi_kv is a butterfly sum over the group (the same bits in every lane), thetabar_k += phi_kv
//     pbar stays in registers.  Phi is read from a (V, Kp) transposed copy made once per call (csr_transpose_phi_kernel, Kp = K rounded up
//     to LG, zero-padded), so that an entry's column is one contiguous run used for both products.  pbar of every stored entry goes to an
//     nnz-long array, theta to an (n, K) row-major one.
//   column pass (CSC order), csr_phibar_seg_kernel + csr_phibar_combine_kernel: Phi-bar_kv = sum_n theta_kn pbar_nv.  The caller supplies
//     the column grouping: ccol (V + 1) column pointers and cperm (nnz) listing CSR positions sorted by (column, row).  A column is cut
//     into segments of CSR_SEG entries (a word present in every sample is the normal case); a lane group owns a segment, lanes over
//     topics, adds its entries in list order reading theta[n][0..K) as one run, and writes its partial sum; the combine kernel adds a
//     column's segments in order (in double) into one (K, V) slot, zeros for a column without entries.  The segment table (csr_segscan_kernel)
//     and the row of every entry (csr_entry_rows_kernel) are built once per binding.
// No atomics; every sum has a fixed order: bit-identical from run to run.  Every offset into the entry arrays is 64-bit.  A stored entry
// whose value is 0 behaves as an absent one; column indices need not be sorted inside a row; an index outside [0, V) is skipped.
// Duplicate (row, column) entries are NOT supported: each is treated as a word of its own, which is not the likelihood of their sum.
#pragma once
#include "common.h"
#include "rows_vstream.h"
#include "lane_group.h"

namespace gdrf {

enum { CSR_SEG = 256 };          // entries of a column segment

// phiT[v][k] = phi[k][v] for k < K, 0 for K <= k < Kp
template <typename T>
__global__ void csr_transpose_phi_kernel(const T* __restrict__ phi, int K, int Kp, int V, T* __restrict__ phiT) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)V * Kp) return;
  const int64_t v = e / Kp;
  const int k = (int)(e - v * Kp);
  phiT[e] = k < K ? phi[(int64_t)k * V + v] : T(0);
}

// erow[e] = the row of stored entry e; a 16-lane group per row
__global__ __launch_bounds__(256) void csr_entry_rows_kernel(const int64_t* __restrict__ crow, int64_t nrows, int64_t nnz, int32_t* __restrict__ erow) {
  const int l = threadIdx.x & 15;
  for (int64_t n = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4; n < nrows; n += ((int64_t)gridDim.x * blockDim.x) >> 4) {
    const int64_t a = max((int64_t)0, crow[n]), b = min(nnz, crow[n + 1]);
    for (int64_t e = a + l; e < b; e += 16) erow[e] = (int32_t)n;
  }
}

// The segment table of the column pass, one workgroup of 1024 threads: column v has max(1, ceil(len_v / CSR_SEG)) segments; segoff (V + 1)
// is their exclusive scan, segcol[w] the column of segment w.  At most V + nnz / CSR_SEG segments.
__global__ __launch_bounds__(1024) void csr_segscan_kernel(const int64_t* __restrict__ ccol, int V, int64_t* __restrict__ segoff, int32_t* __restrict__ segcol) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int per = (V + 1023) / 1024;
  const int v0 = min(V, t * per), v1 = min(V, v0 + per);
  int64_t s = 0;
  for (int v = v0; v < v1; ++v) { const int64_t len = ccol[v + 1] - ccol[v]; s += len > CSR_SEG ? (len + CSR_SEG - 1) / CSR_SEG : 1; }
  part[t] = s;
  __syncthreads();
  if (t == 0) { int64_t a = 0; for (int i = 0; i < 1024; ++i) { const int64_t x = part[i]; part[i] = a; a += x; } segoff[V] = a; }
  __syncthreads();
  int64_t o = part[t];
  for (int v = v0; v < v1; ++v) {
    const int64_t len = ccol[v + 1] - ccol[v];
    const int64_t ns = len > CSR_SEG ? (len + CSR_SEG - 1) / CSR_SEG : 1;
    segoff[v] = o;
    for (int64_t j = 0; j < ns; ++j) segcol[o + j] = v;
    o += ns;
  }
}

// The row pass.  src: mu (VS_SOFTMAX) or theta (VS_LINK) as (K, n) through (src_sk, src_sn), topic_probs (n, K) for VS_PERP.  crow points at
// the first of the call's nrows rows (entries are absolute positions).  dst as in rows_vstream_kernel; thN (n, K) and pb (nnz) for the
// column pass, cn (n) for the link mode's constant part; dpart[grid][4] slot 1 (ELBO modes) or dpart[grid][2] (VS_PERP, added when dacc).
template <typename T, int MODE, int LG, int KJ>
__global__ __launch_bounds__(256) void rows_csr_kernel(
    int64_t nrows, int K, int Kp, int V, int64_t nnz, const T* src, int64_t src_sk, int64_t src_sn,
    const int64_t* __restrict__ crow, const int32_t* __restrict__ col, const int32_t* __restrict__ val,
    const T* __restrict__ phiT, const T* __restrict__ rowsum, T* dst, int64_t dst_ld, double* __restrict__ dpart, int dacc,
    T* __restrict__ thN, T* __restrict__ pb, T* __restrict__ cn_out) {
  constexpr bool ELBO = MODE == VS_SOFTMAX || MODE == VS_LINK;
  constexpr int RPB = 256 / LG;
  __shared__ double scratch[16];
  const int tid = threadIdx.x, l = tid % LG, g = tid / LG;
  const T feps = t_eps<T>();
  double s_a = 0, s_b = 0;
  const int64_t nblk = (nrows + RPB - 1) / RPB;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t n = blk * RPB + g;
    if (n >= nrows) continue;                              // the lanes of a group leave together
    T th[KJ], tb[KJ];
    T ips = 0;
    int kd = 0;
    if constexpr (MODE == VS_SOFTMAX) {
#pragma unroll
      for (int j = 0; j < KJ; ++j) { const int k = l + LG * j; th[j] = k < K ? src[(int64_t)k * src_sk + n * src_sn] : T(GROUP_PAD); }
      group_softmax<LG>(th, l, K);
      T ps = 0, tmax = -1;
#pragma unroll
      for (int j = 0; j < KJ; ++j) {
        const int k = l + LG * j;
        if (k < K) { ps += th[j] * rowsum[k]; if (th[j] > tmax) { tmax = th[j]; kd = k; } }
      }
      ps = group_sum<LG>(ps);
      ips = T(1) / ps;
      group_argmax<LG>(tmax, kd);                          // the dominant topic: the largest theta, the lowest index among equals
    } else {
      T ps = 0;
#pragma unroll
      for (int j = 0; j < KJ; ++j) {
        const int k = l + LG * j;
        th[j] = k < K ? src[(int64_t)k * src_sk + n * src_sn] : T(0);
        if constexpr (ELBO) { if (k < K) ps += th[j] * rowsum[k]; }
      }
      if constexpr (ELBO) { ps = group_sum<LG>(ps); ips = T(1) / ps; }
    }
    if constexpr (ELBO) {
#pragma unroll
      for (int j = 0; j < KJ; ++j) { tb[j] = 0; const int k = l + LG * j; if (k < K) thN[n * K + k] = th[j]; }
    }
    T wsum = 0;                                            // link: the sum of the unclamped counts
    const int64_t ea = max((int64_t)0, crow[n]), eb = min(nnz, crow[n + 1]);
    for (int64_t e0 = ea; e0 < eb; e0 += LG) {
      const int64_t my = e0 + l;
      const bool has = my < eb;
      const int vc = has ? col[my] : -1;
      const int wc = has ? val[my] : 0;
      const int cnt = (int)min((int64_t)LG, eb - e0);
      T mypb = 0;
      for (int t = 0; t < cnt; ++t) {
        const int v = __shfl(vc, t, LG);
        const int w = __shfl(wc, t, LG);
        if ((unsigned)v >= (unsigned)V) continue;          // outside the vocabulary: skipped (the same in every lane of the group)
        const T* pc = phiT + (int64_t)v * Kp + l;
        T f[KJ];
        T p = 0;
#pragma unroll
        for (int j = 0; j < KJ; ++j) {
          f[j] = LG * j < Kp ? pc[LG * j] : T(0);
          p += th[j] * f[j];
        }
        p = group_sum<LG>(p);
        if constexpr (MODE == VS_PERP) {
          if (l == 0 && w != 0) { s_a += (double)w * (double)t_log<T>(p); s_b += (double)w; }
        } else {
          const T ph = p * ips;
          const T wt = (T)w;
          const bool inr = (ph > feps) && (ph < T(1) - feps);
          const T phc = fmin(fmax(ph, feps), T(1) - feps);
          if (l == 0) s_a += (double)(wt * t_log<T>(phc));
          const T pbv = inr ? wt / p : T(0);
          wsum += inr ? wt : T(0);
#pragma unroll
          for (int j = 0; j < KJ; ++j) tb[j] += f[j] * pbv;
          if (l == t) mypb = pbv;
        }
      }
      if constexpr (ELBO) { if (has) pb[my] = mypb; }
    }
    if constexpr (MODE == VS_SOFTMAX) {
      // mubar_k = theta_k ((thetabar_k - cref) + sum_j theta_j (cref - thetabar_j)), cref = thetabar of the dominant topic
      T cref = 0;
#pragma unroll
      for (int j = 0; j < KJ; ++j) if (l + LG * j == kd) cref = tb[j];
      cref = group_sum<LG>(cref);                      // one lane holds it, the others add zeros
      T d = 0;
#pragma unroll
      for (int j = 0; j < KJ; ++j) if (l + LG * j < K) d += th[j] * (cref - tb[j]);
      d = group_sum<LG>(d);
#pragma unroll
      for (int j = 0; j < KJ; ++j) { const int k = l + LG * j; if (k < K) dst[(int64_t)k * dst_ld + n] = th[j] * ((tb[j] - cref) + d); }
    } else if constexpr (MODE == VS_LINK) {
      const T cn = wsum * ips;                             // d/dp_v' of -sum_v w_v log(sum p), the same for every v'
#pragma unroll
      for (int j = 0; j < KJ; ++j) { const int k = l + LG * j; if (k < K) dst[(int64_t)k * dst_ld + n] = tb[j] - cn * rowsum[k]; }
      if (l == 0) cn_out[n] = cn;
    }
  }
  if constexpr (ELBO) {
    dpart_store<DP_LOGLIK>(dpart, scratch, 0, s_a, 0, 0);
  } else {
    dpart_store2(dpart, scratch, s_a, s_b, dacc);
  }
}

// link mode: cpart[block][k] = sum over the block's rows of theta_k cn, the constant part of its Phi-bar (vs_sub_rows_kernel subtracts its
// reduction).  Thread k of a workgroup, rows blockIdx.x, blockIdx.x + gridDim.x, ... in blocks of 64.
template <typename T>
__global__ __launch_bounds__(128) void csr_link_const_kernel(int64_t nrows, int K, const T* __restrict__ thN, const T* __restrict__ cn, T* __restrict__ cpart) {
  const int k = threadIdx.x;
  if (k >= K) return;
  T acc = 0;
  const int64_t nblk = (nrows + 63) / 64;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t n1 = min(nrows, blk * 64 + 64);
    for (int64_t n = blk * 64; n < n1; ++n) acc += thN[n * K + k] * cn[n];
  }
  cpart[(int64_t)blockIdx.x * K + k] = acc;
}

// The column pass: segment w of the table (column segcol[w], entries ccol[v] + j CSR_SEG ... of cperm) -> parts[w][0..K)
template <typename T, int LG, int KJ>
__global__ __launch_bounds__(256) void csr_phibar_seg_kernel(
    int K, int V, int64_t nnz, int64_t nrows, const int64_t* __restrict__ ccol, const int64_t* __restrict__ cperm, const int64_t* __restrict__ segoff,
    const int32_t* __restrict__ segcol, const int32_t* __restrict__ erow, const T* __restrict__ pb, const T* __restrict__ thN,
    T* __restrict__ parts) {
  const int l = threadIdx.x % LG;
  const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LG;
  if (w >= segoff[V]) return;
  const int v = segcol[w];
  const int64_t i0 = ccol[v] + (w - segoff[v]) * CSR_SEG;
  const int64_t i1 = min(min(ccol[v + 1], i0 + CSR_SEG), nnz);
  T acc[KJ];
#pragma unroll
  for (int j = 0; j < KJ; ++j) acc[j] = 0;
  for (int64_t c0 = max((int64_t)0, i0); c0 < i1; c0 += LG) {
    const int64_t my = c0 + l;
    int r = -1;
    T pv = 0;
    if (my < i1) {
      const int64_t e = cperm[my];
      if (e >= 0 && e < nnz) { r = erow[e]; pv = pb[e]; }
    }
    const int cnt = (int)min((int64_t)LG, i1 - c0);
    for (int t = 0; t < cnt; ++t) {
      const int rr = __shfl(r, t, LG);
      const T pbv = __shfl(pv, t, LG);
      if ((unsigned)rr >= (uint64_t)nrows) continue;
      const T* tr = thN + (int64_t)rr * K + l;
#pragma unroll
      for (int j = 0; j < KJ; ++j) if (l + LG * j < K) acc[j] += tr[LG * j] * pbv;
    }
  }
#pragma unroll
  for (int j = 0; j < KJ; ++j) { const int k = l + LG * j; if (k < K) parts[w * K + k] = acc[j]; }
}

// out[k][v] = the sum of column v's segments in order (in double); zero for a column without entries
template <typename T>
__global__ void csr_phibar_combine_kernel(int K, int V, const int64_t* __restrict__ segoff, const T* __restrict__ parts, T* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)K * V) return;
  const int k = (int)(e / V);
  const int64_t v = e - (int64_t)k * V;
  double s = 0;
  for (int64_t w = segoff[v]; w < segoff[v + 1]; ++w) s += (double)parts[w * K + k];
  out[e] = (T)s;
}

// data-only Multinomial constant on CSR rows: sum_n [lgamma(total_n + 1) - sum_e lgamma(w_e + 1)] in double (kernels_n.h: ll_const_kernel);
// a 16-lane group per row, its lanes' sums added in a fixed order
__global__ __launch_bounds__(256) void ll_const_csr_kernel(const int64_t* __restrict__ crow, const int32_t* __restrict__ val, int64_t nrows, int64_t nnz,
                                                           double* __restrict__ dpart) {
  __shared__ double scratch[16];
  const int l = threadIdx.x & 15;
  double s = 0;
  for (int64_t n = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4; n < nrows; n += ((int64_t)gridDim.x * blockDim.x) >> 4) {
    const int64_t a = max((int64_t)0, crow[n]), b = min(nnz, crow[n + 1]);
    double tot = 0, sl = 0;
    for (int64_t e = a + l; e < b; e += 16) { const double w = (double)val[e]; tot += w; sl += lgamma(w + 1.0); }
    tot = group_sum<16>(tot);
    if (l == 0) s += lgamma(tot + 1.0);
    s -= sl;
  }
  s = block_sum(s, scratch);
  if (threadIdx.x == 0) dpart[blockIdx.x] = s;
}

}  // namespace gdrf
