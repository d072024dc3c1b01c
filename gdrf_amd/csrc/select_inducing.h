// Greedy conditional-variance choice of inducing points from the data (gdrf_select_inducing): the pivoted partial Cholesky of the PRIOR
// kernel matrix K_nn of the n rows X, the rule of select_batch.h without a posterior and without noise (Burt, Rasmussen, van der Wilk 2020,
// Alg. 1).  In the solve precision TS, with k the context's kernel at its current hyper-parameters and G `given` rows appended behind the
// candidates as forced pivots:
//   d[j] = k(x_j, x_j)                                 for the nt = n + G rows
//   pick t:  p = the t-th given row (t < G), else the candidate j < n not picked yet with the largest d[j], ties to the lower index
//            piv_t = d[p]
//            piv_t > floor:  c_t[j] = (k(x_j, x_p) - sum_{s<t} c_s[j] c_s[p]) / sqrt(piv_t),   d[j] -= c_t[j]^2
//            else:           c_t = 0       (nothing left to explain, or a duplicate among the given rows)
//            trace_t = sum_{j<n} d[j]      (double) = tr(K_nn - Q_nn) of the picks so far
// rank = the picks with piv_t > floor.  DESIGN.md section 27 has the definition, the limits and the numbers.
//
// No n x n matrix and no factorisation: the kernel column of a pick is evaluated on the fly from the (embedded) rows.  Per pick two launches,
// the host reads nothing in between:
//   inducing_prep_kernel  one workgroup: the trace of the pass before it, the argmax over the pass's per-workgroup partials (a forced pivot
//                         for t < G), the pivot, whether it is above the floor, and the pivot's own history c_s[p]
//   inducing_pass_kernel  the pass over the rows, a thread per row: the pivot's history broadcast from LDS, the row's history c_s[j] read in
//                         whole lines of the (T, nt) array, eight entries requested together; the kernel column; the update of c and d; the
//                         workgroup's best (d, index) and the tile's part of the trace
// The pass is a streaming kernel; its traffic is the read of the history, T^2 nt / 2 elements over the whole call.  The best row is compared as
// (d, -index), the trace is summed per tile of 256 rows and then over the tiles, both in one fixed order: no atomics, the same result for every
// grid, bit-identical calls.
#pragma once
#include "common.h"
#include "kernels_mm.h"
#include "select_batch.h"

namespace gdrf {

#define GDRF_IND_ROWS 256       // rows of a tile in the pass: a thread per row
#define GDRF_IND_PARTS 2048     // most workgroups of the pass (its per-workgroup best rows)
#define GDRF_IND_NEG (-1.7976931348623157e308)    // the d of "no candidate": below every real one (a rounded-off d may be slightly negative)

// what the preparation leaves for the pass of the same pick
struct IndPick { long long p; double piv; int ok; int pad; };

// the rows' coordinates as the covariance forms see them: scaled in ARD contexts, as they are otherwise (embedded rows carry their scales)
template <typename TS, typename T, bool ARD>
__device__ __forceinline__ void ind_row(const T* __restrict__ X, int64_t j, int D, const Hyper* __restrict__ h, TS (&x)[GDRF_DMAX]) {
#pragma unroll
  for (int dd = 0; dd < GDRF_DMAX; ++dd)
    x[dd] = dd < D ? (ARD ? (TS)X[j * D + dd] * (TS)h->sc[dd] : (TS)X[j * D + dd]) : TS(0);
}

// the workgroup's sum of v over its 256 threads in one fixed order, returned to every thread; sw: LDS scratch of 4 entries
__device__ __forceinline__ double ind_block_sum(double v, double* sw) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sw[0] + sw[1]) + sw[2]) + sw[3];
}

// d[j] = k(x_j, x_j) for the nt rows, taken[j] = 0, the first partials.  grid <= GDRF_IND_PARTS workgroups of 256 threads striding over the tiles
template <typename TS>
__global__ __launch_bounds__(256) void inducing_init_kernel(int64_t n, int64_t nt, int kind, const Hyper* __restrict__ h, TS* __restrict__ d,
                                                            int* __restrict__ taken, double* __restrict__ part_g, long long* __restrict__ part_i,
                                                            double* __restrict__ part_tr) {
  __shared__ double sg[4];
  __shared__ long long si[4];
  __shared__ double sw[4];
  const TS kd = cov_from_r2<TS>(kind, TS(0), (TS)h->var, (TS)h->alpha);
  const int64_t ntiles = (nt + GDRF_IND_ROWS - 1) / GDRF_IND_ROWS;
  double bg = GDRF_IND_NEG; long long bi = GDRF_SEL_NONE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t j = tile * GDRF_IND_ROWS + threadIdx.x;
    if (j < nt) { d[j] = kd; taken[j] = 0; }
    if (j < n && sel_better((double)kd, j, bg, bi)) { bg = (double)kd; bi = j; }
    const double tr = ind_block_sum(j < n ? (double)kd : 0.0, sw);
    if (threadIdx.x == 0) part_tr[tile] = tr;
  }
  sel_block_best(bg, bi, sg, si, part_g, part_i);
}

template <typename TS>
struct IndPrep {
  int t, G, Tm, nparts;                       // pick t of Tm = G + count; t = Tm: the trace of the last pass only
  int64_t n, nt, ntiles;
  double floor;
  const double* part_g; const long long* part_i; const double* part_tr;
  const TS* c; const TS* d;                   // (Tm, nt), (nt)
  TS* hp; IndPick* pick; int* taken;          // the pivot's history (GDRF_INDUCING_MAX_PICKS)
  long long* idx_out; double* pivots_out; double* trace_out; int* rank_out;
};

// one workgroup of 256 threads
template <typename TS>
__global__ __launch_bounds__(256) void inducing_prep_kernel(IndPrep<TS> a) {
  __shared__ double sg[4];
  __shared__ long long si[4];
  __shared__ double sw[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, t = a.t;
  if (t > 0) {
    // trace_{t-1}: the tiles' parts, a thread's in the order of the tiles, then the threads'
    double tr = 0;
    for (int64_t x = tid; x < a.ntiles; x += 256) tr += a.part_tr[x];
    tr = ind_block_sum(tr, sw);
    if (tid == 0) a.trace_out[t - 1] = tr;
  }
  if (t >= a.Tm) return;
  int64_t p;
  if (t < a.G) {
    p = a.n + t;                              // a given row: a forced pivot
  } else {
    double g = GDRF_IND_NEG; long long i = GDRF_SEL_NONE;
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
    p = (i >= 0 && i < a.n) ? i : 0;          // no candidate compares as better only when every d is NaN: stay inside the arrays
  }
  for (int s = tid; s < t; s += 256) a.hp[s] = a.c[(int64_t)s * a.nt + p];
  if (tid == 0) {
    const double piv = (double)a.d[p];
    const int ok = piv > a.floor ? 1 : 0;
    a.pick->p = p; a.pick->piv = piv; a.pick->ok = ok;
    a.taken[p] = 1;
    if (t >= a.G) a.idx_out[t - a.G] = p;
    a.pivots_out[t] = piv;
    *a.rank_out = (t == 0 ? 0 : *a.rank_out) + ok;
  }
}

template <typename TS, typename T>
struct IndPass {
  int t, D, kind;
  int64_t n, nt;
  const Hyper* h; const T* X;                 // the (embedded) rows, (nt, D)
  const TS* hp; const IndPick* pick;
  TS* c; TS* d;
  const int* taken;
  double* part_g; long long* part_i; double* part_tr;
};

// grid <= min(ceil(nt / 256), GDRF_IND_PARTS) workgroups of 256 threads striding over the tiles; dynamic LDS t solve-precision elements
template <typename TS, typename T, bool ARD>
__global__ __launch_bounds__(256) void inducing_pass_kernel(IndPass<TS, T> a) {
  extern __shared__ __attribute__((aligned(16))) char ind_smem[];
  TS* hs_p = reinterpret_cast<TS*>(ind_smem);        // c_s[p], s < t
  __shared__ double sg[4];
  __shared__ long long si[4];
  __shared__ double sw[4];
  const int tid = threadIdx.x, t = a.t;
  const int64_t nt = a.nt, p = a.pick->p;
  const bool ok = a.pick->ok != 0;
  const int64_t ntiles = (nt + GDRF_IND_ROWS - 1) / GDRF_IND_ROWS;
  const TS var = (TS)a.h->var, ils2 = (TS)a.h->inv_ls2, al = (TS)a.h->alpha;
  TS xp[GDRF_DMAX];
  ind_row<TS, T, ARD>(a.X, p, a.D, a.h, xp);
  // the pivot comes from the preparation, not from d[p]: the pivot's own thread rewrites that while other workgroups are still to start
  const TS sq = ok ? t_sqrt<TS>((TS)a.pick->piv) : TS(1);
  if (ok)
    for (int s = tid; s < t; s += 256) hs_p[s] = a.hp[s];
  __syncthreads();
  double bg = GDRF_IND_NEG; long long bi = GDRF_SEL_NONE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t j = tile * GDRF_IND_ROWS + tid;
    TS dn = 0;
    if (j < nt) {
      dn = a.d[j];
      TS cn = 0;
      if (ok) {
        TS xj[GDRF_DMAX];
        ind_row<TS, T, ARD>(a.X, j, a.D, a.h, xj);
        TS r2 = 0;
#pragma unroll
        for (int dd = 0; dd < GDRF_DMAX; ++dd) { const TS df = xj[dd] - xp[dd]; r2 += df * df; }
        const TS kjp = cov_from_r2<TS>(a.kind, r2 * ils2, var, al);
        // eight entries of the history per round, their loads requested together: one memory latency per round, not per entry
        const TS* cj = a.c + j;
        TS hs = 0;
        int s = 0;
        for (; s + 8 <= t; s += 8) {
          TS cv[8];
#pragma unroll
          for (int x = 0; x < 8; ++x) cv[x] = cj[(int64_t)(s + x) * nt];
#pragma unroll
          for (int x = 0; x < 8; ++x) hs += cv[x] * hs_p[s + x];
        }
        for (; s < t; ++s) hs += cj[(int64_t)s * nt] * hs_p[s];
        cn = (kjp - hs) / sq;
        dn -= cn * cn;
        a.d[j] = dn;
      }
      a.c[(int64_t)t * nt + j] = cn;
    }
    if (j < a.n && !a.taken[j] && sel_better((double)dn, j, bg, bi)) { bg = (double)dn; bi = j; }
    const double tr = ind_block_sum(j < a.n ? (double)dn : 0.0, sw);
    if (tid == 0) a.part_tr[tile] = tr;
  }
  sel_block_best(bg, bi, sg, si, a.part_g, a.part_i);
}

// out (n) float64 from d (nt)
template <typename TS>
__global__ void inducing_resid_out_kernel(const TS* __restrict__ d, int64_t n, double* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) out[j] = (double)d[j];
}

}  // namespace gdrf
