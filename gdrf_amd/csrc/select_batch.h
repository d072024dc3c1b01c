// Greedy choice of a non-redundant batch of rows (gdrf_select_batch).  With C_k = R + T_k T_k^T the joint posterior covariances of
// predict_cov.h and s2 > 0 an observation-noise variance, the information in noisy observations f_k(x_a) + N(0, s2) at the rows A is
//   I(A) = 1/2 sum_k log det(I + C_k[A, A] / s2)
// and the greedy rule picks, `count` times, the row not picked yet with the largest gain g_j = 1/2 sum_k log1p(max(d_k[j], 0) / s2), ties
// to the lower index; d_k[j] is the variance of f_k(x_j) given noisy observations at every pick so far.  Pick t at row p updates, per topic,
//   c_k,t[j] = (C_k[j][p] - sum_{s<t} c_k,s[j] c_k,s[p]) / sqrt(d_k[p] + s2),   d_k[j] -= c_k,t[j]^2
// (the pivoted partial Cholesky of C_k + s2 I); sum_t gain_t = I(picked).  d_k starts as mode 4's variance, clamp included, widened to the
// solve precision.  G `given` rows, appended behind the n candidates, are forced pivots ahead of the free picks.  s2 > 0 keeps every
// pivot positive: no failure flag, no jitter.  DESIGN.md section 23 has the definition and the numbers.
//
// No n x n matrix is formed.  One column per pick comes from the solve-precision W (c->jW, predict_cov.h):
//   C_k[j][p] = (k(x_j, x_p) - w_j . w_p) + w_j . b_k,   b_k = S_k (S_k^T w_p)
// Per pick two launches, the host reads nothing in between:
//   select_prep_kernel  one workgroup per topic: the argmax over the pass's per-workgroup partials (a forced pivot for t < G), w_p, b_k,
//                       the pivot's own history c_k,s[p] and d_k[p]
//   select_pass_kernel  the pass over the rows: K + 1 dot products of length Mp per row against B = (w_p, b_1 .. b_K), the history, the
//                       update of c and d, the new gain and the workgroup's best (gain, index)
// The pass is a skinny product in the solve precision; its traffic is the read of W.  A workgroup owns tiles of 64 rows.  The right-hand sides
// go through LDS in blocks of 16 columns (w_p and 15 topics); lane groups of 16 lanes own a row, each lane 16 bytes of it per step, two
// rows at a time against one read of B.  Up to 15 topics the block is loaded once per workgroup and W is read once; above, the tile's
// further blocks read it again (from L2) and reload B.  The epilogue puts the rows on the lanes, so c and d move in whole lines.  Sums
// run in one fixed order, the best row is compared as (gain, -index): no atomics, the same result for every grid, bit-identical calls.
#pragma once
#include "common.h"
#include "kernels_mm.h"
#include "lane_group.h"

namespace gdrf {

#define GDRF_SEL_ROWS 64       // rows of a workgroup's tile in the pass
#define GDRF_SEL_COLS 16       // right-hand sides per block: w_p and GDRF_SEL_COLS - 1 topics
#define GDRF_SEL_PARTS 1024    // most workgroups of the pass (its per-workgroup partials)

template <typename T> __device__ __forceinline__ T t_log1p(T x);
template <> __device__ __forceinline__ float  t_log1p<float>(float x)   { return log1pf(x); }
template <> __device__ __forceinline__ double t_log1p<double>(double x) { return log1p(x); }

template <typename TS> __device__ __forceinline__ TS sel_gain_term(TS d, TS s2) { return TS(0.5) * t_log1p<TS>((d > TS(0) ? d : TS(0)) / s2); }

__device__ __forceinline__ bool sel_better(double g2, long long i2, double g, long long i) { return g2 > g || (g2 == g && i2 < i); }

// the workgroup's best (gain, index) of its threads' candidates -> part[blockIdx.x]; sg, si: LDS scratch of 4 entries (256 threads)
__device__ __forceinline__ void sel_block_best(double g, long long i, double* sg, long long* si, double* __restrict__ part_g, long long* __restrict__ part_i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double g2 = __shfl_xor(g, o, 64);
    const long long i2 = __shfl_xor(i, o, 64);
    if (sel_better(g2, i2, g, i)) { g = g2; i = i2; }
  }
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sg[w] = g; si[w] = i; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int x = 1; x < (int)(blockDim.x >> 6); ++x)
      if (sel_better(sg[x], si[x], g, i)) { g = sg[x]; i = si[x]; }
    part_g[blockIdx.x] = g; part_i[blockIdx.x] = i;
  }
}

#define GDRF_SEL_NONE 0x7fffffffffffffffLL      // the index of "no candidate" (its gain is -1: every real gain is >= 0)

// d[k][j] = f_var[k][j] of mode 4 (row_prior_v0 + tt) for the nt = n + G rows, taken[j] = 0, and the first gains' partials over the n candidates
template <typename TS, typename T>
__global__ __launch_bounds__(256) void select_init_kernel(int64_t n, int64_t nt, int K, const Hyper* __restrict__ h, const T* __restrict__ qpart, int nqpart,
                                                          const T* __restrict__ tt, int64_t ldk, double s2d, TS* __restrict__ d, int* __restrict__ taken,
                                                          double* __restrict__ part_g, long long* __restrict__ part_i) {
  __shared__ double sg[4];
  __shared__ long long si[4];
  const TS s2 = (TS)s2d;
  double bg = -1.0; long long bi = GDRF_SEL_NONE;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < nt; j += (int64_t)gridDim.x * 256) {
    const T v0 = row_prior_v0(qpart, nqpart, ldk, j, (T)h->var);
    TS g = 0;
    for (int k = 0; k < K; ++k) {
      const TS dv = (TS)(v0 + tt[(int64_t)k * ldk + j]);
      d[(int64_t)k * nt + j] = dv;
      g += sel_gain_term<TS>(dv, s2);
    }
    taken[j] = 0;
    if (j < n && sel_better((double)g, j, bg, bi)) { bg = (double)g; bi = j; }
  }
  sel_block_best(bg, bi, sg, si, part_g, part_i);
}

template <typename TS, typename T>
struct SelPrep {
  int t, G, K, M, Mp, Tm, nparts;             // pick t of Tm = G + count
  int64_t n, nt;
  const double* part_g; const long long* part_i;
  const TS* W; const T* S; const T* ST;       // (nt, Mp); S_k and S_k^T (K, Mp, Mp) in the array precision
  const TS* c; const TS* d;                   // (K, Tm, nt), (K, nt)
  TS* B; TS* hp; TS* dp;                      // (K + 1, Mp); (K, Tm); (K)
  long long* picks; int* taken; long long* idx_out; double* gains_out;
};

// grid K, 256 threads; dynamic LDS 2 Mp solve-precision elements
template <typename TS, typename T>
__global__ __launch_bounds__(256) void select_prep_kernel(SelPrep<TS, T> a) {
  extern __shared__ __attribute__((aligned(16))) char sel_smem[];
  TS* wp = reinterpret_cast<TS*>(sel_smem);
  TS* u = wp + a.Mp;
  __shared__ double sg[4];
  __shared__ long long si[4];
  const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, M = a.M, Mp = a.Mp;
  int64_t p;
  if (a.t < a.G) {
    p = a.n + a.t;                            // a given row: a forced pivot
    if (k == 0 && tid == 0) a.picks[a.t] = p;
  } else {
    // every workgroup reduces the partials itself (the same comparison in the same order: the same row)
    double g = -1.0; long long i = GDRF_SEL_NONE;
    for (int x = tid; x < a.nparts; x += 256)
      if (sel_better(a.part_g[x], a.part_i[x], g, i)) { g = a.part_g[x]; i = a.part_i[x]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double g2 = __shfl_xor(g, o, 64);
      const long long i2 = __shfl_xor(i, o, 64);
      if (sel_better(g2, i2, g, i)) { g = g2; i = i2; }
    }
    if (lane == 0) { sg[wave] = g; si[wave] = i; }
    __syncthreads();
    g = sg[0]; i = si[0];
    for (int x = 1; x < 4; ++x)
      if (sel_better(sg[x], si[x], g, i)) { g = sg[x]; i = si[x]; }
    p = (i >= 0 && i < a.n) ? i : 0;          // no candidate compares as better only when every gain is NaN: stay inside the arrays
    if (k == 0 && tid == 0) {
      a.picks[a.t] = p; a.taken[p] = 1;
      a.idx_out[a.t - a.G] = p; a.gains_out[a.t - a.G] = g;
    }
  }
  for (int i = tid; i < Mp; i += 256) wp[i] = i < M ? a.W[p * Mp + i] : TS(0);
  __syncthreads();
  const T* sk = a.S + (int64_t)k * Mp * Mp;
  const T* st = a.ST + (int64_t)k * Mp * Mp;
  // S_k is lower triangular.  u = S_k^T w_p: u[j] = sum_{q >= j} S_k[q][j] w_p[q]; b_k = S_k u: b[i] = sum_{j <= i} ST_k[j][i] u[j].  A thread
  // per entry, consecutive lanes on consecutive addresses, each sum in the order of its index
  for (int j = tid; j < Mp; j += 256) {
    TS s = 0;
    if (j < M)
#pragma unroll 8
      for (int q = j; q < M; ++q) s += (TS)sk[(int64_t)q * Mp + j] * wp[q];
    u[j] = s;
  }
  __syncthreads();
  for (int i = tid; i < Mp; i += 256) {
    TS b = 0;
    if (i < M)
#pragma unroll 8
      for (int j = 0; j <= i; ++j) b += (TS)st[(int64_t)j * Mp + i] * u[j];
    a.B[(int64_t)(1 + k) * Mp + i] = b;
    if (k == 0) a.B[i] = wp[i];
  }
  for (int s = tid; s < a.t; s += 256) a.hp[(int64_t)k * a.Tm + s] = a.c[((int64_t)k * a.Tm + s) * a.nt + p];
  if (tid == 0) a.dp[k] = a.d[(int64_t)k * a.nt + p];
}

template <typename TS, typename T>
struct SelPass {
  int t, K, Mp, Tm, D, kind;
  int64_t n, nt;
  double s2;
  const Hyper* h; const T* X;                 // the (embedded) rows, (nt, D)
  const TS* W; const TS* B; const TS* hp; const TS* dp;
  TS* c; TS* d;
  const long long* picks; const int* taken;
  double* part_g; long long* part_i;
};

template <typename TS> static inline size_t sel_pass_lds(int Mp) {
  return ((size_t)GDRF_SEL_COLS * Mp + (size_t)GDRF_SEL_COLS * GDRF_SEL_ROWS + 4 * GDRF_SEL_ROWS) * sizeof(TS);
}

// grid <= min(ceil(nt / 64), GDRF_SEL_PARTS) workgroups of 256 threads striding over the tiles; dynamic LDS sel_pass_lds<TS>(Mp)
template <typename TS, typename T, bool ARD>
__global__ __launch_bounds__(256) void select_pass_kernel(SelPass<TS, T> a) {
  constexpr int VE = Vec16<TS>::N, NC = GDRF_SEL_COLS, NR = GDRF_SEL_ROWS;
  using vec_t = typename Vec16<TS>::type;
  extern __shared__ __attribute__((aligned(16))) char sel_smem[];
  TS* Bs = reinterpret_cast<TS*>(sel_smem);          // [NC][Mp]
  TS* sums = Bs + (size_t)NC * a.Mp;                 // [NC][NR]
  TS* gw = sums + NC * NR;                           // [4][NR]
  __shared__ double sg[4];
  __shared__ long long si[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = tid >> 4, gl = tid & 15;
  const int K = a.K, Mp = a.Mp, t = a.t;
  const int64_t nt = a.nt, p = a.picks[t];
  const int nb = (K + NC - 2) / (NC - 1);
  const int64_t ntiles = (nt + NR - 1) / NR;
  const TS s2 = (TS)a.s2, var = (TS)a.h->var, ils2 = (TS)a.h->inv_ls2, al = (TS)a.h->alpha;
  TS xp[GDRF_DMAX];
#pragma unroll
  for (int dd = 0; dd < GDRF_DMAX; ++dd)
    xp[dd] = dd < a.D ? (ARD ? (TS)a.X[p * a.D + dd] * (TS)a.h->sc[dd] : (TS)a.X[p * a.D + dd]) : TS(0);
  double bg = -1.0; long long bi = GDRF_SEL_NONE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t j0 = tile * NR, jr = j0 + lane;    // jr: the row this lane owns in the epilogue
    TS kpp = 0;
    if (jr < nt) {
      TS r2 = 0;
#pragma unroll
      for (int dd = 0; dd < GDRF_DMAX; ++dd) {
        const TS xj = dd < a.D ? (ARD ? (TS)a.X[jr * a.D + dd] * (TS)a.h->sc[dd] : (TS)a.X[jr * a.D + dd]) : TS(0);
        const TS df = xj - xp[dd];
        r2 += df * df;
      }
      kpp = cov_from_r2<TS>(a.kind, r2 * ils2, var, al);
    }
    TS gacc = 0;
    for (int kb = 0; kb < nb; ++kb) {
      if (nb > 1 || tile == (int64_t)blockIdx.x) {
        // column 0: w_p; column i: b of topic (NC - 1) kb + i - 1, zeros past the last topic
        __syncthreads();
        for (int x = tid * VE; x < NC * Mp; x += 256 * VE) {
          const int i = x / Mp, q = x - i * Mp;
          const int kk = (NC - 1) * kb + i - 1;
          vec_t v;
#pragma unroll
          for (int e = 0; e < VE; ++e) v[e] = TS(0);
          if (i == 0) v = *reinterpret_cast<const vec_t*>(a.B + q);
          else if (kk < K) v = *reinterpret_cast<const vec_t*>(a.B + (int64_t)(1 + kk) * Mp + q);
          *reinterpret_cast<vec_t*>(Bs + x) = v;
        }
        __syncthreads();
      }
      // the dot products: this lane group's four rows, two at a time
#pragma unroll 1
      for (int rp = 0; rp < 4; rp += 2) {
        const int r0 = grp * 4 + rp;
        const int64_t ja = j0 + r0 < nt ? j0 + r0 : nt - 1, jb = j0 + r0 + 1 < nt ? j0 + r0 + 1 : nt - 1;
        const TS* wa = a.W + ja * Mp;
        const TS* wb = a.W + jb * Mp;
        TS acc[2][NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) { acc[0][i] = 0; acc[1][i] = 0; }
        for (int q = gl * VE; q < Mp; q += 16 * VE) {
          const vec_t va = *reinterpret_cast<const vec_t*>(wa + q);
          const vec_t vb = *reinterpret_cast<const vec_t*>(wb + q);
#pragma unroll
          for (int i = 0; i < NC; ++i) {
            const vec_t b = *reinterpret_cast<const vec_t*>(Bs + (size_t)i * Mp + q);
#pragma unroll
            for (int e = 0; e < VE; ++e) { acc[0][i] += va[e] * b[e]; acc[1][i] += vb[e] * b[e]; }
          }
        }
        TS m0 = 0, m1 = 0;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
          const TS s0 = group16_sum(acc[0][i]), s1 = group16_sum(acc[1][i]);
          if (gl == i) { m0 = s0; m1 = s1; }
        }
        sums[gl * NR + r0] = m0;
        sums[gl * NR + r0 + 1] = m1;
      }
      __syncthreads();
      // the epilogue: lanes over the tile's rows, waves over the block's topics
      if (jr < nt) {
        const TS br = kpp - sums[lane];
        for (int i = wave == 0 ? 4 : wave; i < NC; i += 4) {
          const int k = (NC - 1) * kb + i - 1;
          if (k >= K) break;
          const TS* ck = a.c + (int64_t)k * a.Tm * nt + jr;
          const TS* hk = a.hp + (int64_t)k * a.Tm;
          // eight entries of the history per round, their loads requested together: one memory latency per round, not per entry
          TS hs = 0;
          int s = 0;
          for (; s + 8 <= t; s += 8) {
            TS cv[8], hv[8];
#pragma unroll
            for (int x = 0; x < 8; ++x) { cv[x] = ck[(int64_t)(s + x) * nt]; hv[x] = hk[s + x]; }
#pragma unroll
            for (int x = 0; x < 8; ++x) hs += cv[x] * hv[x];
          }
          for (; s < t; ++s) hs += ck[(int64_t)s * nt] * hk[s];
          const TS cn = (br + sums[i * NR + lane] - hs) / t_sqrt<TS>(a.dp[k] + s2);
          a.c[((int64_t)k * a.Tm + t) * nt + jr] = cn;
          const TS dn = a.d[(int64_t)k * nt + jr] - cn * cn;
          a.d[(int64_t)k * nt + jr] = dn;
          gacc += sel_gain_term<TS>(dn, s2);
        }
      }
      __syncthreads();
    }
    gw[wave * NR + lane] = gacc;
    __syncthreads();
    if (wave == 0 && jr < a.n && !a.taken[jr]) {
      const double g = (double)(((gw[lane] + gw[NR + lane]) + gw[2 * NR + lane]) + gw[3 * NR + lane]);
      if (sel_better(g, jr, bg, bi)) { bg = g; bi = jr; }
    }
  }
  sel_block_best(bg, bi, sg, si, a.part_g, a.part_i);
}

// out (K, n) float64 from d (K, nt)
template <typename TS>
__global__ void select_var_out_kernel(const TS* __restrict__ d, int64_t n, int64_t nt, double* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
  if (j < n) out[k * n + j] = (double)d[k * nt + j];
}

}  // namespace gdrf
