// Joint posterior at new inputs (gdrf_predict_cov, gdrf_sample_joint): with W = K_*m L^-T (n x M, the step's forward),
//   R   = K_** - W W^T                     (n x n, the same for every topic; no jitter, no clamp)
//   C_k = R + T_k T_k^T,  T_k = W S_k      (the covariance of q(f_k(X*)); its diagonal is mode 4's f_var without the clamp)
//   f[s][k][:] = W (u_k + S_k xi[s][k][:]) + G zeta[s][k][:] + mean[k][:],  G G^T = R + j I      (pathwise joint samples)
// (whiten = False: u_k, S_k are L^-1 u_k, L^-1 S_k, as everywhere else).  DESIGN.md section 19 has the derivation and the numbers.
//
// Everything n x n is formed in the solve precision: K_** - W W^T cancels almost completely near the inducing points, so W is
// recomputed here in the solve precision from the step's solve-precision K_nm and L^-1 (the step's own W is stored in the array
// precision) and K_** is evaluated in the solve precision in the epilogue of the product that subtracts W W^T from it.
//
// One product form serves every contraction: out[i][j] = sum_q A[i][q] B[j][q] (both operands row-major along the reduction index) on
// the solve-precision 16x16x4 matrix instruction.  A workgroup owns a 64 x 64 output tile, each of its four waves a 32 x 32 quarter (2 x 2
// instruction tiles); the operands come straight from L2 as 16-byte vectors, lane group g of a wave owning the reduction indices
// q0 + VE g .. + VE - 1 of a step of 4 VE - the same permutation on both operands, so the instruction's own k order does not matter.
// The symmetric forms compute the tiles on and below the diagonal only and write every value to both (i, j) and (j, i): the result equals
// its transpose to the bit.  A sum runs over q in one fixed order inside one wave: no atomics, bit-identical from call to call.
#pragma once
#include "common.h"
#include "kernels_mm.h"
#include "kernels_n.h"
#include <type_traits>

namespace gdrf {

enum { COV_FULL = 0, COV_RESID = 1 };
#define GDRF_JT 64             // output tile edge of the joint kernels' workgroups

// Philox streams of gdrf_sample_joint: the "global row" word of philox_normal's counter is XI + m for xi[s][k][m] and ZETA + i for
// zeta[s][k][i] (i: the row's position within the call); the other counter words are (topic, sample) as for gdrf_fill_eps.  The two
// ranges are disjoint from each other and from the rows gdrf_predict_mc and the training step draw for (row < 2^61).
#define GDRF_JOINT_XI_STREAM   ((uint64_t)1 << 61)
#define GDRF_JOINT_ZETA_STREAM ((uint64_t)1 << 62)

// VE consecutive elements at p as solve-precision values (zeros for a row outside the operand: p then points at a valid row)
template <typename TS, typename TB>
__device__ __forceinline__ void jt_load(const TB* __restrict__ p, bool ok, TS (&v)[Vec16<TS>::N]) {
  constexpr int VE = Vec16<TS>::N;
  if constexpr (std::is_same<TS, TB>::value) {
    const typename Vec16<TS>::type x = *reinterpret_cast<const typename Vec16<TS>::type*>(p);
#pragma unroll
    for (int e = 0; e < VE; ++e) v[e] = ok ? x[e] : TS(0);
  } else {
#pragma unroll
    for (int e = 0; e < VE; ++e) v[e] = ok ? (TS)p[e] : TS(0);
  }
}

// acc[a][b] += sum_{q in [q0, q1)} A[i0 + 16 a + r][q] B[j0 + 16 b + c][q] for this wave's 32 x 32 quarter; q0, q1 multiples of 4 VE,
// lda, ldb multiples of VE, rows >= ni / nj read as zero
template <typename TS, typename TB>
__device__ __forceinline__ void jt_accum(typename Mfma<TS>::acc_t (&acc)[2][2], const TS* __restrict__ A, int64_t lda, int64_t i0, int64_t ni,
                                         const TB* __restrict__ B, int64_t ldb, int64_t j0, int64_t nj, int q0, int q1, int lane) {
  using MF = Mfma<TS>;
  constexpr int VE = Vec16<TS>::N, KC = 4 * VE;
  const int lr = lane & 15, lg = lane >> 4;
  const TS* ap[2];
  const TB* bp[2];
  bool aok[2], bok[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int64_t ra = i0 + 16 * t + lr, rb = j0 + 16 * t + lr;
    aok[t] = ra < ni; bok[t] = rb < nj;
    ap[t] = A + (aok[t] ? ra : 0) * lda + lg * VE;
    bp[t] = B + (bok[t] ? rb : 0) * ldb + lg * VE;
  }
  for (int q = q0; q < q1; q += KC) {
    TS va[2][VE], vb[2][VE];
#pragma unroll
    for (int t = 0; t < 2; ++t) { jt_load<TS, TS>(ap[t] + q, aok[t], va[t]); jt_load<TS, TB>(bp[t] + q, bok[t], vb[t]); }
#pragma unroll
    for (int e = 0; e < VE; ++e)
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = MF::mma(va[a][e], vb[b][e], acc[a][b]);
  }
}

// the batched product and its three epilogues; grid (column tiles, row tiles, batch)
//   JT_PLAIN  out[b][i][j] = sum_q A[b][i][q] B[b][j][q]                         every tile (W = K_nm L^-T, T_k = W S_k)
//   JT_RESID  out[i][j] = k(x_i, x_j) - sum_q A[i][q] A[j][q]                    lower tiles + mirror (R; B = A, ni = nj)
//   JT_FULL   out[b][i][j] = base[i][j] + sum_q A[b][i][q] A[b][j][q]            lower tiles + mirror (C_k; B = A, ni = nj)
enum { JT_PLAIN = 0, JT_RESID = 1, JT_FULL = 2 };
template <typename TS, typename TB, typename TX, typename TO>
struct JointNT {
  const TS* A; int64_t lda, a_bs, ni;
  const TB* B; int64_t ldb, b_bs, nj;
  int kd;                                     // reduction length, a multiple of 4 VE
  TO* out; int64_t ldo, o_bs;
  const TS* base; int64_t ldbase;             // JT_FULL
  const TX* X; int D, kind; const Hyper* h;   // JT_RESID: the (embedded) rows; ARD instantiation: scaled by h->sc as they are read
};

template <typename TS, typename TB, typename TX, typename TO, int EPI, bool ARD>
__global__ __launch_bounds__(256) void joint_nt_kernel(JointNT<TS, TB, TX, TO> p) {
  using MF = Mfma<TS>;
  using acc_t = typename MF::acc_t;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15;
  if (EPI != JT_PLAIN && blockIdx.x > blockIdx.y) return;                     // above the diagonal: written by its mirror tile
  const int64_t i0 = (int64_t)blockIdx.y * GDRF_JT + 32 * (wave >> 1), j0 = (int64_t)blockIdx.x * GDRF_JT + 32 * (wave & 1);
  if (EPI != JT_PLAIN && j0 > i0) return;                                     // the upper quarter of a diagonal tile likewise
  if (i0 >= p.ni || j0 >= p.nj) return;
  const int64_t bz = blockIdx.z;
  acc_t acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = acc_t{0, 0, 0, 0};
  jt_accum<TS, TB>(acc, p.A + bz * p.a_bs, p.lda, i0, p.ni, p.B + bz * p.b_bs, p.ldb, j0, p.nj, 0, p.kd, lane);
  TO* out = p.out + bz * p.o_bs;
  TS xj[2][GDRF_DMAX];
  TS var = 0, ils2 = 0, al = 0;
  if (EPI == JT_RESID) {
    var = (TS)p.h->var; ils2 = (TS)p.h->inv_ls2; al = (TS)p.h->alpha;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int64_t j = j0 + 16 * b + lr;
#pragma unroll
      for (int d = 0; d < GDRF_DMAX; ++d)
        xj[b][d] = (j < p.nj && d < p.D) ? (ARD ? (TS)p.X[j * p.D + d] * (TS)p.h->sc[d] : (TS)p.X[j * p.D + d]) : TS(0);
    }
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i = i0 + 16 * a + MF::crow(lane, r);
      if (i >= p.ni) continue;
      TS xi[GDRF_DMAX];
      if (EPI == JT_RESID) {
#pragma unroll
        for (int d = 0; d < GDRF_DMAX; ++d) xi[d] = d < p.D ? (ARD ? (TS)p.X[i * p.D + d] * (TS)p.h->sc[d] : (TS)p.X[i * p.D + d]) : TS(0);
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int64_t j = j0 + 16 * b + lr;
        if (j >= p.nj) continue;
        const TS s = acc[a][b][r];
        if (EPI == JT_PLAIN) { out[i * p.ldo + j] = (TO)s; continue; }
        if (j > i) continue;
        TS v;
        if (EPI == JT_RESID) {
          TS r2 = 0;
#pragma unroll
          for (int d = 0; d < GDRF_DMAX; ++d) { const TS t = xi[d] - xj[b][d]; r2 += t * t; }
          v = cov_from_r2<TS>(p.kind, r2 * ils2, var, al) - s;
        } else {
          v = p.base[i * p.ldbase + j] + s;
        }
        out[i * p.ldo + j] = (TO)v;
        if (j < i) out[j * p.ldo + i] = (TO)v;
      }
    }
}

// the Cholesky input: G = tril(R) + jitter I on the n x n block, zero elsewhere in the (np, np) buffer (chol_kernel works in place on the
// lower triangle; the zeros above it are what the sampler's product over q <= i relies on)
template <typename TS>
__global__ void joint_chol_in_kernel(const TS* __restrict__ R, int64_t n, int64_t np, double jitter, TS* __restrict__ G) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j >= np) return;
  TS v = 0;
  if (i < n && j <= i) { v = R[i * np + j]; if (i == j) v += (TS)jitter; }
  G[i * np + j] = v;
}

// out (n, n) in the array precision from the (np, np) solve-precision R
template <typename TS, typename TO>
__global__ void joint_copy_out_kernel(const TS* __restrict__ R, int64_t n, int64_t np, TO* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j < n) out[i * n + j] = (TO)R[i * np + j];
}

// V[s K + k][i] = u_k[i] + sum_{j <= i} S_k[i][j] xi[s][k][j] in the solve precision, zero for i >= M; grid (ceil(Mp / 256), S K).
// xi: the injected (S, K, M) array, or Philox draws (rounded to the array precision, as an injected copy of them would be).
// Dynamic LDS: M array-precision elements.
template <typename TS, typename T>
__global__ __launch_bounds__(256) void joint_v_kernel(const T* __restrict__ U, const T* __restrict__ ST, int M, int Mp, int K, const T* __restrict__ xi,
                                                      uint64_t seed, TS* __restrict__ V) {
  extern __shared__ __attribute__((aligned(16))) char jv_smem[];
  T* xs = reinterpret_cast<T*>(jv_smem);
  const int sk = blockIdx.y, s = sk / K, k = sk - s * K;
  for (int j = threadIdx.x; j < M; j += blockDim.x)
    xs[j] = xi ? xi[(int64_t)sk * M + j] : philox_normal<T>(seed, GDRF_JOINT_XI_STREAM + (uint64_t)j, k, (uint32_t)s);
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Mp) return;
  TS v = 0;
  if (i < M) {
    const T* st = ST + (int64_t)k * Mp * Mp + i;               // S_k[i][j] = ST_k[j][i]: consecutive lanes, consecutive addresses
    for (int j = 0; j <= i; ++j) v += (TS)st[(int64_t)j * Mp] * (TS)xs[j];
    v += (TS)U[(int64_t)k * M + i];
  }
  V[(int64_t)sk * Mp + i] = v;
}

// Zt[s K + k][i] = zeta[s][k][i] in the solve precision, zero for n <= i < np; grid (ceil(np / 256), S K)
template <typename TS, typename T>
__global__ void joint_zeta_kernel(int64_t n, int64_t np, int K, const T* __restrict__ zeta, uint64_t seed, TS* __restrict__ Zt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  const int sk = blockIdx.y, s = sk / K, k = sk - s * K;
  TS v = 0;
  if (i < n) v = (TS)(zeta ? zeta[(int64_t)sk * n + i] : philox_normal<T>(seed, GDRF_JOINT_ZETA_STREAM + (uint64_t)i, k, (uint32_t)s));
  Zt[(int64_t)sk * np + i] = v;
}

// out[s K + k][i] = sum_m V[s K + k][m] W[i][m] + sum_{q <= i} Zt[s K + k][q] G[i][q] + mean[k][i]: both products of the pathwise sample
// into one accumulator; grid (ceil(n / 64), ceil(S K / 64)).  G is lower triangular with zeros above its diagonal, so the second
// product stops at the end of the quarter's last 32-column block.
template <typename TS, typename T>
__global__ __launch_bounds__(256) void joint_sample_kernel(const TS* __restrict__ V, int64_t nsk, int K, const TS* __restrict__ W, int Mp,
                                                           const TS* __restrict__ Zt, const TS* __restrict__ G, int64_t n, int64_t np,
                                                           const T* __restrict__ mean, int64_t mean_sk, int64_t mean_sn, T* __restrict__ out) {
  using MF = Mfma<TS>;
  using acc_t = typename MF::acc_t;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15;
  const int64_t i0 = (int64_t)blockIdx.y * GDRF_JT + 32 * (wave >> 1), j0 = (int64_t)blockIdx.x * GDRF_JT + 32 * (wave & 1);
  if (i0 >= nsk || j0 >= n) return;
  acc_t acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = acc_t{0, 0, 0, 0};
  jt_accum<TS, TS>(acc, V, Mp, i0, nsk, W, Mp, j0, n, 0, Mp, lane);
  const int64_t qe = j0 + 32 < np ? j0 + 32 : np;
  jt_accum<TS, TS>(acc, Zt, np, i0, nsk, G, np, j0, n, 0, (int)qe, lane);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t sk = i0 + 16 * a + MF::crow(lane, r);
      if (sk >= nsk) continue;
      const int64_t k = sk % K;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int64_t i = j0 + 16 * b + lr;
        if (i >= n) continue;
        TS v = acc[a][b][r];
        if (mean) v += (TS)mean[k * mean_sk + i * mean_sn];
        out[sk * n + i] = (T)v;
      }
    }
}

}  // namespace gdrf
