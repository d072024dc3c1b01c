// Fold-in (gdrf_fold_in): the topic proportions of an OBSERVED sample from its own counts, with the GP as the prior - LDA's transform, the
// z site of the reference's SparseGDRF.  For row n let
//   m_k = f_loc[k][n] + mean_function[k][n],   s_k = f_var[k][n] + noise,
// with (f_loc, f_var) what gdrf_predict mode 4 returns: s_k is the scale of the model's mu site, Normal(f_loc, f_var + noise)
// (sparse_gdrf.py:354-357; the variance used as a SCALE, as the reference writes it and as predict_mc.h does for the guide).  With the
// counts w (V of them), R = sum_v w_v, theta = softmax(mu) and p = theta Phi:
//   J(mu) = sum_{v: w_v > 0} w_v log p_v  -  1/2 sum_k ((mu_k - m_k) / s_k)^2
// The fold-in result is mu_hat, a local maximiser of J reached from the start mu = m; theta_hat = softmax(mu_hat).
// The gradient is g_k = r_k - R theta_k - (mu_k - m_k) / s_k^2 with the expected topic counts r_k = theta_k sum_v w_v Phi_kv / p_v (they
// sum to R over k).
//
// Iteration, at most num_iters times per row:
//   E-step   theta, p, r, J and g at the current mu; the row stops once |g|_inf / max(1, R) <= tol
//   M-step   two Newton steps on the concave EM surrogate Q(mu') = r . mu' - R lse(mu') - 1/2 sum ((mu'_k - m_k) / s_k)^2, whose negative
//            Hessian diag(D) - R theta theta^T, D_k = R theta_k + 1 / s_k^2, is solved in O(K) by Sherman-Morrison (its denominator
//            1 - R sum theta_k^2 / D_k is formed as sum_k theta_k / (s_k^2 D_k): positive, no cancellation).  The step is scaled so that
//            max_k |delta_k| <= 4 (a rare topic with 1 / s^2 small and r_k large otherwise asks for a step of 1e4 that no halving tames),
//            then halved up to 12 times until Q(mu + t delta) - Q(mu) >= 0; a step that is never accepted leaves mu as it is.
// Q - Q(mu) bounds J - J(mu) from below, so J never decreases.  Everything O(K) - the softmax, the Newton solve, the line search - runs
// in double in registers and group shuffles: in float32 and at R ~ 1e4 the line search's differences cancel.  Even in double the direct
// form r . td - R (lse(mu + td) - lse(mu)) - ... (td = t delta) loses a small step's gain in the rounding of R lse and stalls at
// |g| / R ~ 1e-8; the difference is evaluated as
//   Q(mu + td) - Q(mu) = q . td - R (log1p(sum_k theta_k expm1(td_k)) - theta . td) - 1/2 sum_k td_k^2 / s_k^2,   q the gradient of Q at mu,
// with the first-order terms taken out of the lse difference (|g| / R reaches 1e-15).  An accepted step updates theta multiplicatively,
// theta_k (1 + expm1(td_k)) / (1 + sum_j theta_j expm1(td_j)); every E-step recomputes it from mu.  The O(K V) part (p_v, c_v = w_v / p_v,
// r_k) runs in the array precision, its logs summed in double.
//
// Layout, as predict_mc_kernel: a group of LG lanes owns a row, lane l holds the topics l, l + LG, ... (KJ of them; lane_group.h).  The
// row's theta goes through LDS; lanes run over the words for p_v and c_v, over the topics for r_k; what a group exchanges through LDS is
// its own, so wave_lds_fence stands between the phases and no barrier.  No atomics; nothing about a row depends on another row or on the
// grid, so every output but the score's sum over rows is bit-identical however the rows are batched.
//   dense  Phi (K, V) in LDS for the workgroup with the row stride padded to an odd number of elements (lanes that walk k for r_k hit
//          different banks), the row's counts and c_v in LDS
//   CSR    a row's stored entries only, LG at a time: one entry per lane for p and c, then every entry's (column, c) is handed round the
//          group by shuffles for r_k.  A stored zero is an absent entry.  Phi is read from global memory: no limit on V.
// Outputs by mode (the array precision):
//   0  theta_hat (n, K)         1  mu_hat (K, n)          2  r at theta_hat (n, K)
//   3  {sum_n sum_v w2 log p_hat, sum w2} for a second count matrix w2 of the same layout (per-workgroup double partials dpart[grid][2])
// and, in every mode, diag (3, n) in double: J at the result, |g|_inf / max(1, R), the iterations used.
#pragma once
#include "common.h"
#include "kernels_n.h"
#include "lane_group.h"

namespace gdrf {

enum { FI_THETA = 0, FI_MU = 1, FI_COUNTS = 2, FI_SCORE = 3 };
enum { FI_INNER = 2, FI_HALVINGS = 12 };
#define GDRF_FI_CAP 4.0

// the padded row stride of Phi in LDS
__host__ __device__ inline int fi_phi_stride(int V) { return V | 1; }
// dynamic LDS of the dense form: Phi [K][V|1] | theta [rows][LG KJ] | c [rows][V] | counts [rows][V], rows = 256 / LG
template <typename T> inline size_t fi_dense_lds(int K, int V, int LG, int KJ) {
  const size_t rows = 256 / LG;
  return ((size_t)K * fi_phi_stride(V) + rows * LG * KJ + rows * V) * sizeof(T) + rows * V * sizeof(int32_t);
}
// the CSR form keeps theta only
template <typename T> inline size_t fi_csr_lds(int LG, int KJ) { return (size_t)(256 / LG) * LG * KJ * sizeof(T); }

template <typename T, int LG, int KJ, bool CSR>
__global__ __launch_bounds__(256) void foldin_kernel(
    int mode, int64_t nrows, int K, int V, int num_iters, double tol, const Hyper* __restrict__ h, const T* __restrict__ qpart, int nqpart,
    const T* __restrict__ loc, const T* __restrict__ tt, int64_t ldk, const T* __restrict__ mean, int64_t mean_sk, int64_t mean_sn,
    const T* __restrict__ phi, const int32_t* __restrict__ ws, const int64_t* __restrict__ crow, const int32_t* __restrict__ col,
    const int32_t* __restrict__ val, const int32_t* __restrict__ ws2, const int64_t* __restrict__ crow2, const int32_t* __restrict__ col2,
    const int32_t* __restrict__ val2, T* __restrict__ out, double* __restrict__ diag, double* __restrict__ dpart) {
  constexpr int RPB = 256 / LG, Kp = LG * KJ;
  __shared__ double scratch[16];
  extern __shared__ __attribute__((aligned(16))) char fi_smem[];
  const int Vs = fi_phi_stride(V);
  const int tid = threadIdx.x, l = tid % LG, g = tid / LG;
  T* phiS = reinterpret_cast<T*>(fi_smem);                    // dense only
  T* thS = CSR ? phiS : phiS + (size_t)K * Vs;
  T* cS = thS + RPB * Kp;                                     // dense only, as is wS
  int32_t* wS = reinterpret_cast<int32_t*>(cS + (size_t)RPB * V);
  T* th_row = thS + g * Kp;
  T* c_row = cS + (size_t)g * V;
  int32_t* w_row = wS + (size_t)g * V;
  if (!CSR) {
    for (int e = tid; e < K * V; e += 256) phiS[(e / V) * Vs + e % V] = phi[e];
    __syncthreads();
  }
  const T var0 = (T)h->var;
  const double noise = h->noise;
  double s_l = 0, s_w = 0;
  const int64_t nblk = (nrows + RPB - 1) / RPB;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t n = blk * RPB + g;
    if (n >= nrows) continue;                                 // the lanes of a group leave together
    const T v0 = row_prior_v0(qpart, nqpart, ldk, n, var0);
    double m[KJ], is2[KJ], mu[KJ], th[KJ], r[KJ];
    bool on[KJ];
#pragma unroll
    for (int j = 0; j < KJ; ++j) {
      const int k = l + LG * j;
      on[j] = k < K;
      m[j] = is2[j] = r[j] = th[j] = 0;
      if (on[j]) {
        T mk, fv;
        row_prior_topic(v0, loc, tt, ldk, mean, mean_sk, mean_sn, k, n, mk, fv);
        const double s = (double)fv + noise;
        m[j] = (double)mk;
        is2[j] = 1.0 / (s * s);
      }
      mu[j] = m[j];
    }
    // the row's counts and their total
    int64_t e0 = 0, e1 = 0;
    double R = 0;
    if (CSR) {
      e0 = crow[n]; e1 = crow[n + 1];
      for (int64_t e = e0 + l; e < e1; e += LG) R += (double)val[e];
    } else {
      for (int v = l; v < V; v += LG) { const int32_t w = ws[n * V + v]; w_row[v] = w; R += (double)w; }
    }
    R = group_sum<LG>(R);
    const double Rn = R > 1.0 ? R : 1.0;
    double J = 0, gn = 0;
    int used = 0;
    for (;;) {
      // ---- E-step: theta = softmax(mu) in double, then p, c and r in the array precision
      double mx = -1.0e300;
#pragma unroll
      for (int j = 0; j < KJ; ++j) if (on[j]) mx = fmax(mx, mu[j]);
      mx = group_max<LG>(mx);
      double se = 0;
#pragma unroll
      for (int j = 0; j < KJ; ++j) { th[j] = on[j] ? exp(mu[j] - mx) : 0.0; se += th[j]; }
      se = group_sum<LG>(se);
      const double ise = 1.0 / se;
#pragma unroll
      for (int j = 0; j < KJ; ++j) { th[j] *= ise; th_row[l + LG * j] = (T)th[j]; }
      wave_lds_fence();
      double ll = 0;
      T acc[KJ];
#pragma unroll
      for (int j = 0; j < KJ; ++j) acc[j] = 0;
      if (CSR) {
        for (int64_t eb = e0; eb < e1; eb += LG) {
          const int64_t e = eb + l;
          int cv = 0;
          T c = 0;
          if (e < e1) {
            const int32_t w = val[e];
            cv = col[e];
            if (w != 0) {
              const T p = theta_phi(th_row, phi + cv, (int64_t)V, K);
              ll += (double)w * (double)t_log<T>(p);
              c = (T)w / p;
            }
          }
          const int cnt = (int)(e1 - eb < LG ? e1 - eb : LG);
          for (int i = 0; i < cnt; ++i) {
            const T ci = __shfl(c, i, LG);
            const int vi = __shfl(cv, i, LG);
#pragma unroll
            for (int j = 0; j < KJ; ++j) if (on[j]) acc[j] += ci * phi[(int64_t)(l + LG * j) * V + vi];
          }
        }
      } else {
        for (int v = l; v < V; v += LG) {
          const int32_t w = w_row[v];
          T c = 0;
          if (w != 0) {
            const T p = theta_phi(th_row, phiS + v, Vs, K);
            ll += (double)w * (double)t_log<T>(p);
            c = (T)w / p;
          }
          c_row[v] = c;
        }
        wave_lds_fence();
#pragma unroll
        for (int j = 0; j < KJ; ++j)
          if (on[j]) { const T* pr = phiS + (l + LG * j) * Vs; for (int v = 0; v < V; ++v) acc[j] += c_row[v] * pr[v]; }
      }
      wave_lds_fence();                                      // theta and c are rewritten by the next E-step
      double pr2 = 0, gmax = 0;
#pragma unroll
      for (int j = 0; j < KJ; ++j) {
        r[j] = th[j] * (double)acc[j];
        const double d = mu[j] - m[j];
        pr2 += d * d * is2[j];
        gmax = fmax(gmax, fabs(r[j] - R * th[j] - d * is2[j]));
      }
      J = group_sum<LG>(ll) - 0.5 * group_sum<LG>(pr2);
      gn = group_max<LG>(gmax) / Rn;
      if (used >= num_iters || gn <= tol) break;
      // ---- M-step: FI_INNER capped, line-searched Newton steps on Q; theta follows mu multiplicatively
      for (int in = 0; in < FI_INNER; ++in) {
        double q[KJ], D[KJ], dl[KJ];
        double sa = 0, den = 0;
#pragma unroll
        for (int j = 0; j < KJ; ++j) {
          q[j] = r[j] - R * th[j] - (mu[j] - m[j]) * is2[j];
          D[j] = on[j] ? R * th[j] + is2[j] : 1.0;
          sa += th[j] * q[j] / D[j];
          den += th[j] * is2[j] / D[j];
        }
        sa = group_sum<LG>(sa);
        den = group_sum<LG>(den);
        const double f = R * sa / den;
        double dmax = 0;
#pragma unroll
        for (int j = 0; j < KJ; ++j) { dl[j] = on[j] ? (q[j] + th[j] * f) / D[j] : 0.0; dmax = fmax(dmax, fabs(dl[j])); }
        dmax = group_max<LG>(dmax);
        if (!(dmax > 0.0)) break;
        double t = dmax > GDRF_FI_CAP ? GDRF_FI_CAP / dmax : 1.0;
        bool ok = false;
        double ex[KJ], u = 0;
        for (int hv = 0; hv <= FI_HALVINGS; ++hv, t *= 0.5) {
          // Q(mu + t delta) - Q(mu) = q . td - R (log1p(sum_k theta_k expm1(td_k)) - theta . td) - 1/2 sum_k td_k^2 / s_k^2: the first-order
          // terms are taken out of the lse difference, so a small step's gain is not lost in R lse's rounding
          double lin = 0, a1 = 0;
          u = 0;
#pragma unroll
          for (int j = 0; j < KJ; ++j) {
            const double td = t * dl[j];
            ex[j] = th[j] * expm1(td);
            u += ex[j];
            a1 += th[j] * td;
            lin += td * (q[j] - 0.5 * is2[j] * td);
          }
          u = group_sum<LG>(u);
          a1 = group_sum<LG>(a1);
          lin = group_sum<LG>(lin);
          if (lin - R * (log1p(u) - a1) >= 0.0) { ok = true; break; }
        }
        if (!ok) break;                                      // no step accepted: a second try from the same point gives the same
        const double isx = 1.0 / (1.0 + u);
#pragma unroll
        for (int j = 0; j < KJ; ++j) { mu[j] += t * dl[j]; th[j] = (th[j] + ex[j]) * isx; }
      }
      ++used;
    }
    // ---- outputs: theta, r, J and g are those of the last E-step, taken at the returned mu
    if (l == 0) { diag[n] = J; diag[nrows + n] = gn; diag[2 * nrows + n] = (double)used; }
#pragma unroll
    for (int j = 0; j < KJ; ++j) {
      const int k = l + LG * j;
      if (!on[j]) continue;
      if (mode == FI_THETA) out[n * K + k] = (T)th[j];
      else if (mode == FI_MU) out[(int64_t)k * nrows + n] = (T)mu[j];
      else if (mode == FI_COUNTS) out[n * K + k] = (T)r[j];
    }
    if (mode == FI_SCORE) {
      double a = 0, sw = 0;
      if (CSR) {
        for (int64_t e = crow2[n] + l; e < crow2[n + 1]; e += LG) {
          const int32_t w = val2[e];
          if (w == 0) continue;
          a += (double)w * (double)t_log<T>(theta_phi(th_row, phi + col2[e], (int64_t)V, K));
          sw += (double)w;
        }
      } else {
        for (int v = l; v < V; v += LG) {
          const int32_t w = ws2[n * V + v];
          if (w == 0) continue;
          a += (double)w * (double)t_log<T>(theta_phi(th_row, phiS + v, Vs, K));
          sw += (double)w;
        }
      }
      wave_lds_fence();                                      // theta is rewritten by the group's next row
      s_l += a; s_w += sw;                                   // per lane: the block sum below adds the lanes
    }
  }
  if (mode == FI_SCORE) dpart_store2(dpart, scratch, s_l, s_w);
}

}  // namespace gdrf
