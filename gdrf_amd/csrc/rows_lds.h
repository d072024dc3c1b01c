// The one-thread-per-row kernels of the per-row ELBO stage.
//   elbo_rows_kernel         the whole stage of gdrf_step_local with Phi (K x V) and its gradient in LDS (row form 0 where the
//                            matrix-core kernel of rows_mfma.h does not apply)
//   rows_mu_kernel           the V-free head:  q, the variance, mu = loc + v eps (+ mean)
//   rows_sites_kernel        the V-free tail:  mubar -> both Normal sites and the row-local backward
//   elbo_rows2_sites_kernel  the V-free tail when guide and model sit at different inputs (gdrf_step_local2)
// Between head and tail the vocabulary part (p = theta Phi, the log-likelihood, thetabar, Phi-bar) is rows_vstream_kernel or
// rows_csr_kernel: that is the streamed row form of gdrf_step_local, and the only form of gdrf_step_local2 and gdrf_step_local_link.
#pragma once
#include "common.h"
#include "kernels_mm.h"

namespace gdrf {

// q_n = the sum of the column tiles' partials, the variance gate a = [var - q_n > 0]; returns v0 = a (var - q_n), so that v_k = v0 + tt_k
template <typename T>
__device__ __forceinline__ T rows_v0(const T* __restrict__ qpart, int nqpart, int64_t ldk, int64_t n, T var, T& qn, T& a) {
  qn = 0;
  for (int c = 0; c < nqpart; ++c) qn += qpart[(int64_t)c * ldk + n];
  a = (var - qn > T(0)) ? T(1) : T(0);
  return a * (var - qn);
}

// both Normal sites of topic k of a row and their row-local backward, given the draw's eps, v = v0 + tt and mub (the likelihood's
// pull-back to mu): shared by elbo_rows_kernel and rows_sites_kernel (rows2_topic is the two-point form)
template <typename T>
__device__ __forceinline__ void rows_topic(int k, int64_t n, T vk, T ek, T mub, T eta, int64_t ldk,
                                           T* __restrict__ vbar, T* __restrict__ locbar, T& site, T& ng, T& vsum) {
  const T s = vk + eta, r = vk / s, e2 = ek * ek;
  site += -t_log<T>(s) + t_log<T>(vk) - T(0.5) * e2 * r * r + T(0.5) * e2;
  const T dcdv = -T(1) / s + T(1) / vk - e2 * r * eta / (s * s);
  ng += -T(1) / s + e2 * r * r / s;
  const T vb = mub * ek + dcdv;
  vbar[(int64_t)k * ldk + n] = vb;
  locbar[(int64_t)k * ldk + n] = mub;
  vsum += vb;
}

// =====================================================================================
// elbo_rows: per observation: variance, reparameterised draw, softmax link, Multinomial
// log-likelihood, both Normal site terms, and the row-local part of the backward.
// One thread per row.  Each lane walks its own row of counts (V int32, contiguous) straight from global memory: the lanes of a wave are
// V * 4 bytes apart, but every lane consumes whole lines over its V iterations, so the 200 MB stream is read once (0.87 ms at the
// headline size); staging the workgroup's rows through LDS with whole-line 16-byte loads was measured SLOWER (1.1-1.5 ms: an
// extra pass and barrier in a kernel that lives on occupancy).  KREG: K <= GDRF_KMAX, the per-topic values of a row live in registers; otherwise
// they are re-read from the (K, n) arrays (coalesced over the rows) and the softmax pull-back goes through LDS - any K.
// =====================================================================================

template <typename T, bool KREG>
__global__ __launch_bounds__(128) void elbo_rows_kernel(
    int64_t nrows, int K, int V, const Hyper* __restrict__ h,
    const T* __restrict__ qpart, int nqpart, const T* __restrict__ loc, const T* __restrict__ tt, const T* __restrict__ eps,
    int64_t ldk, int64_t lde,
    const int32_t* __restrict__ ws, const T* __restrict__ phi,
    const T* __restrict__ mean /*may be null*/, int64_t mean_sk, int64_t mean_sn,
    T* __restrict__ qout, T* __restrict__ vbar, T* __restrict__ locbar, T* __restrict__ asum, T* __restrict__ mu_out,
    double* __restrict__ dpart /*[grid][4]*/, T* __restrict__ phibar_part /*[grid][K*V]*/) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int RB = blockDim.x;
  constexpr int KR = KREG ? GDRF_KMAX : 1;
  double* scratch = reinterpret_cast<double*>(smem);    // [16]
  T* phiS = reinterpret_cast<T*>(smem + 128);           // [K*V]
  T* accS = phiS + K * V;                               // [K*V] phibar accumulator (owner-thread only)
  T* thS = accS + K * V;                                // [RB][K+1]
  T* pbS = thS + RB * (K + 1);                          // [RB][V+1]
  T* tbS = pbS + RB * (V + 1);                          // [RB][K+1], !KREG only
  for (int e = threadIdx.x; e < K * V; e += RB) { phiS[e] = phi[e]; accS[e] = 0; }
  __syncthreads();
  const T var = (T)h->var, eta = (T)h->noise;
  const T feps = t_eps<T>();
  double s_site = 0, s_llw = 0, s_noise = 0, s_vd = 0;
  const int64_t nblk = (nrows + RB - 1) / RB;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t n = blk * RB + threadIdx.x;
    const bool ok = n < nrows;
    T* th = thS + threadIdx.x * (K + 1);
    T* pb = pbS + threadIdx.x * (V + 1);
    T* tbl = tbS + threadIdx.x * (K + 1);
    T v[KR], mu[KR], ep[KR];
    T a = 0, vd = 0;
    if (ok) {
      T qn = 0;
      for (int c = 0; c < nqpart; ++c) qn += qpart[(int64_t)c * ldk + n];
      qout[n] = qn;
      a = (var - qn > T(0)) ? T(1) : T(0);
      const T v0 = a * (var - qn);
      auto topic = [&](int k, T& vk, T& ek, T& mk) {
        ek = eps[(int64_t)k * lde + n];
        vk = v0 + tt[(int64_t)k * ldk + n];
        mk = loc[(int64_t)k * ldk + n] + vk * ek;
        if (mean) mk += mean[(int64_t)k * mean_sk + n * mean_sn];   // f_loc + mean_function(xs): the site terms only see mu - f_loc
      };
      T mx = -3.0e38f;
      if constexpr (KREG) {
#pragma unroll
        for (int k = 0; k < KR; ++k) if (k < K) { topic(k, v[k], ep[k], mu[k]); mx = fmax(mx, mu[k]); }
      } else {
        for (int k = 0; k < K; ++k) { T vk, ek, mk; topic(k, vk, ek, mk); th[k] = mk; mx = fmax(mx, mk); }
      }
      T se = 0;
      if constexpr (KREG) {
#pragma unroll
        for (int k = 0; k < KR; ++k) if (k < K) { const T e = t_exp<T>(mu[k] - mx); th[k] = e; se += e; }
      } else {
        for (int k = 0; k < K; ++k) { const T e = t_exp<T>(th[k] - mx); th[k] = e; se += e; }
      }
      const T ise = T(1) / se;
      for (int k = 0; k < K; ++k) th[k] *= ise;
      // pass 1: p_v = sum_k theta_k phi_kv ; pass 2: log-likelihood and pbar = w * mask / p
      T ps = 0;
      for (int vv = 0; vv < V; ++vv) {
        T p = 0;
        for (int k = 0; k < K; ++k) p += th[k] * phiS[k * V + vv];
        pb[vv] = p;
        ps += p;
      }
      const T ips = T(1) / ps;
      T llw = 0;
      for (int vv = 0; vv < V; ++vv) {
        const T p = pb[vv];
        const T ph = p * ips;
        const T wv = (T)ws[n * V + vv];
        const bool inr = (ph > feps) && (ph < T(1) - feps);
        const T phc = fmin(fmax(ph, feps), T(1) - feps);
        llw += wv * t_log<T>(phc);
        pb[vv] = inr ? wv / p : T(0);
      }
      s_llw += (double)llw;
      // thetabar_k = sum_v phi_kv pbar_v ; softmax Jacobian
      // softmax pull-back mubar_k = theta_k (thetabar_k - sum_j theta_j thetabar_j).  mu = loc + v eps has a spread of tens of units (the
      // reference passes the predictive VARIANCE as the Normal's scale, quirk Q1), so one theta is 1 - O(1e-4) and the literal form
      // subtracts two numbers of size thetabar ~ sum_v w_v that agree to 4 digits: 1e-3 relative error in float.  With ANY constant c,
      // thetabar_k - dot = (thetabar_k - c) + sum_j theta_j (c - thetabar_j)   (sum_j theta_j = 1);  c = thetabar of the dominant topic
      // removes the large term from the sum - every product then carries a small theta_j or is exactly zero.
      T tb[KR];
      T cref = 0;
      if constexpr (KREG) {
#pragma unroll
        for (int k = 0; k < KR; ++k) if (k < K) {
          T s = 0;
          for (int vv = 0; vv < V; ++vv) s += phiS[k * V + vv] * pb[vv];
          tb[k] = s;
          if (mu[k] == mx) cref = s;
        }
      } else {
        T tmax = -1;
        for (int k = 0; k < K; ++k) {
          T s = 0;
          for (int vv = 0; vv < V; ++vv) s += phiS[k * V + vv] * pb[vv];
          tbl[k] = s;
          if (th[k] > tmax) { tmax = th[k]; cref = s; }
        }
      }
      T dot = 0;                                     // = sum_j theta_j (cref - thetabar_j)
      if constexpr (KREG) {
#pragma unroll
        for (int k = 0; k < KR; ++k) if (k < K) dot += th[k] * (cref - tb[k]);
      } else {
        for (int k = 0; k < K; ++k) dot += th[k] * (cref - tbl[k]);
      }
      T site = 0, ng = 0, vsum = 0;
      // the site terms of rows_topic and the gate of rows_v0, written out: calling the helpers here changes this kernel's register allocation
      auto finish_topic = [&](int k, T vk, T ek, T mk, T tbk) {
        const T mub = th[k] * ((tbk - cref) + dot);
        const T s = vk + eta, r = vk / s, e2 = ek * ek;
        site += -t_log<T>(s) + t_log<T>(vk) - T(0.5) * e2 * r * r + T(0.5) * e2;
        const T dcdv = -T(1) / s + T(1) / vk - e2 * r * eta / (s * s);
        ng += -T(1) / s + e2 * r * r / s;
        const T vb = mub * ek + dcdv;
        vbar[(int64_t)k * ldk + n] = vb;
        locbar[(int64_t)k * ldk + n] = mub;
        if (mu_out) mu_out[(int64_t)k * ldk + n] = mk;
        vsum += vb;
      };
      if constexpr (KREG) {
#pragma unroll
        for (int k = 0; k < KR; ++k) if (k < K) finish_topic(k, v[k], ep[k], mu[k], tb[k]);
      } else {
        for (int k = 0; k < K; ++k) { T vk, ek, mk; topic(k, vk, ek, mk); finish_topic(k, vk, ek, mk, tbl[k]); }
      }
      vd = a * vsum;
      asum[n] = vd;
      s_site += (double)site; s_noise += (double)ng; s_vd += (double)vd;
    } else {
      for (int k = 0; k < K; ++k) th[k] = 0;
      for (int vv = 0; vv < V; ++vv) pb[vv] = 0;
    }
    __syncthreads();
    // phibar_kv += sum_rows theta_k pbar_v : each (k,v) pair has one owner thread
    for (int e = threadIdx.x; e < K * V; e += RB) {
      const int k = e / V, vv = e - k * V;
      T s = 0;
      for (int r = 0; r < RB; ++r) s += thS[r * (K + 1) + k] * pbS[r * (V + 1) + vv];
      accS[e] += s;
    }
    __syncthreads();
  }
  dpart_store<DP_ALL>(dpart, scratch, s_site, s_llw, s_noise, s_vd);
  for (int e = threadIdx.x; e < K * V; e += RB) phibar_part[(int64_t)blockIdx.x * K * V + e] = accS[e];
}

// The V-free head of the stage: q, the variance and the draw mu = loc + v eps (+ mean) -> mu_out (K, ldk), which rows_vstream_kernel or
// rows_csr_kernel (softmax link) or the caller's link function reads.  One thread per row, any K.
template <typename T>
__global__ __launch_bounds__(64) void rows_mu_kernel(
    int64_t nrows, int K, const Hyper* __restrict__ h,
    const T* __restrict__ qpart, int nqpart, const T* __restrict__ loc, const T* __restrict__ tt, const T* __restrict__ eps,
    int64_t ldk, int64_t lde, const T* __restrict__ mean /*may be null*/, int64_t mean_sk, int64_t mean_sn,
    T* __restrict__ qout, T* __restrict__ mu_out) {
  const T var = (T)h->var;
  for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < nrows; n += (int64_t)gridDim.x * blockDim.x) {
    T qn, a;
    const T v0 = rows_v0<T>(qpart, nqpart, ldk, n, var, qn, a);
    qout[n] = qn;
    for (int k = 0; k < K; ++k) {
      const T vk = v0 + tt[(int64_t)k * ldk + n];
      T mk = loc[(int64_t)k * ldk + n] + vk * eps[(int64_t)k * lde + n];
      if (mean) mk += mean[(int64_t)k * mean_sk + n * mean_sn];   // f_loc + mean_function(xs): the site terms only see mu - f_loc
      mu_out[(int64_t)k * ldk + n] = mk;
    }
  }
}

// The V-free tail: mub (K, mub_ld) is the likelihood's pull-back to mu - from the streamed or sparse kernel through the softmax, or
// from the caller through its own link's Jacobian.  Both Normal sites and the row-local backward (vbar, locbar, asum); slots 0, 2, 3 of
// dpart - the vocabulary kernel writes slot 1 on the same grid.  One thread per row, any K.
template <typename T>
__global__ __launch_bounds__(64) void rows_sites_kernel(
    int64_t nrows, int K, const Hyper* __restrict__ h,
    const T* __restrict__ qpart, int nqpart, const T* __restrict__ tt, const T* __restrict__ eps, int64_t ldk, int64_t lde,
    const T* __restrict__ mub, int64_t mub_ld,
    T* __restrict__ vbar, T* __restrict__ locbar, T* __restrict__ asum, double* __restrict__ dpart /*[grid][4]*/) {
  __shared__ double scratch[16];
  const T var = (T)h->var, eta = (T)h->noise;
  double s_site = 0, s_noise = 0, s_vd = 0;
  for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < nrows; n += (int64_t)gridDim.x * blockDim.x) {
    T qn, a;
    const T v0 = rows_v0<T>(qpart, nqpart, ldk, n, var, qn, a);
    T site = 0, ng = 0, vsum = 0;
    for (int k = 0; k < K; ++k)
      rows_topic<T>(k, n, v0 + tt[(int64_t)k * ldk + n], eps[(int64_t)k * lde + n], mub[(int64_t)k * mub_ld + n], eta, ldk, vbar, locbar,
                    site, ng, vsum);
    const T vd = a * vsum;
    asum[n] = vd;
    s_site += (double)site; s_noise += (double)ng; s_vd += (double)vd;
  }
  dpart_store<DP_SITES>(dpart, scratch, s_site, 0, s_noise, s_vd);
}

// The same per-row terms when the guide and the model evaluate the GP predictive at DIFFERENT inputs - the reference's quirk Q3
// (gdrf/models/sparse_gdrf.py:376-380: for a world other than the unit cube the guide scales its inputs twice, the model once).
// Guide side (subscript g): mu = loc_g + v_g eps, log q = -log v_g - eps^2 / 2.  Model side (m): log p = -log s_m - (d / s_m)^2 / 2 with
// s_m = v_m + noise, d = mu - loc_m (- the model-side mean).  With mub the pull-back of the likelihood through the softmax link:
//   locbar_g = mub - d / s_m^2 ;  vbar_g = locbar_g eps + 1 / v_g ;  locbar_m = d / s_m^2 ;  vbar_m = -1 / s_m + d^2 / s_m^3 (= d/d noise)
// (for identical inputs their sums are the single-point formulas of rows_topic).  Not a hot path.
// rows2_topic: the model- and guide-side terms of topic k of a row, given mub (the likelihood's pull-back through the softmax link)
template <typename T>
__device__ __forceinline__ void rows2_topic(int k, int64_t n, T mu, T vg, T ek, T mub, T v0m, T eta, int64_t ldk,
                                            const T* __restrict__ tt_m, const T* __restrict__ loc_m,
                                            const T* __restrict__ mean_m, int64_t mm_sk, int64_t mm_sn,
                                            T* __restrict__ vbar_m, T* __restrict__ locbar_m, T* __restrict__ vbar_g, T* __restrict__ locbar_g,
                                            T* __restrict__ mu_out, T& site, T& ng, T& vsm, T& vsg) {
  const T vm = v0m + tt_m[(int64_t)k * ldk + n], sm = vm + eta;
  T lm = loc_m[(int64_t)k * ldk + n];
  if (mean_m) lm += mean_m[(int64_t)k * mm_sk + n * mm_sn];
  const T d = mu - lm;
  site += -t_log<T>(sm) - T(0.5) * (d / sm) * (d / sm) + t_log<T>(vg) + T(0.5) * ek * ek;
  const T lbm = d / (sm * sm), vbm = -T(1) / sm + d * d / (sm * sm * sm);
  const T lbg = mub - lbm, vbg = lbg * ek + T(1) / vg;
  ng += vbm;
  vbar_m[(int64_t)k * ldk + n] = vbm; locbar_m[(int64_t)k * ldk + n] = lbm;
  vbar_g[(int64_t)k * ldk + n] = vbg; locbar_g[(int64_t)k * ldk + n] = lbg;
  if (mu_out) mu_out[(int64_t)k * ldk + n] = mu;
  vsm += vbm; vsg += vbg;
}

// The V-free tail of the two-point step: mub (K, ldk) comes from the streamed or sparse kernel, which took theta from the guide-side mu
// (rows_mu_kernel on the guide's arrays).  Writes slots 0, 2, 3 of dpart; the vocabulary kernel writes slot 1 on the same grid.  One
// thread per row, any K.
template <typename T>
__global__ __launch_bounds__(64) void elbo_rows2_sites_kernel(
    int64_t nrows, int K, const Hyper* __restrict__ h, int nqpart,
    const T* __restrict__ qpart_m, const T* __restrict__ loc_m, const T* __restrict__ tt_m,
    const T* __restrict__ qpart_g, const T* __restrict__ loc_g, const T* __restrict__ tt_g,
    const T* __restrict__ eps, int64_t ldk, int64_t lde, const T* __restrict__ mub,
    const T* __restrict__ mean_m, int64_t mm_sk, int64_t mm_sn, const T* __restrict__ mean_g, int64_t mg_sk, int64_t mg_sn,
    T* __restrict__ qout, T* __restrict__ vbar_m, T* __restrict__ locbar_m, T* __restrict__ asum_m,
    T* __restrict__ vbar_g, T* __restrict__ locbar_g, T* __restrict__ asum_g, T* __restrict__ mu_out, double* __restrict__ dpart /*[grid][4]*/) {
  __shared__ double scratch[16];
  const T var = (T)h->var, eta = (T)h->noise;
  double s_site = 0, s_noise = 0, s_vd = 0;
  for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < nrows; n += (int64_t)gridDim.x * blockDim.x) {
    T qm, qg, am, ag;
    const T v0m = rows_v0<T>(qpart_m, nqpart, ldk, n, var, qm, am), v0g = rows_v0<T>(qpart_g, nqpart, ldk, n, var, qg, ag);
    qout[n] = qm;
    T site = 0, ng = 0, vsm = 0, vsg = 0;
    for (int k = 0; k < K; ++k) {
      const T ek = eps[(int64_t)k * lde + n];
      const T vg = v0g + tt_g[(int64_t)k * ldk + n];
      T mu = loc_g[(int64_t)k * ldk + n] + vg * ek;
      if (mean_g) mu += mean_g[(int64_t)k * mg_sk + n * mg_sn];
      rows2_topic<T>(k, n, mu, vg, ek, mub[(int64_t)k * ldk + n], v0m, eta, ldk, tt_m, loc_m, mean_m, mm_sk, mm_sn,
                     vbar_m, locbar_m, vbar_g, locbar_g, mu_out, site, ng, vsm, vsg);
    }
    asum_m[n] = am * vsm; asum_g[n] = ag * vsg;
    s_site += (double)site; s_noise += (double)ng; s_vd += (double)(am * vsm + ag * vsg);
  }
  dpart_store<DP_SITES>(dpart, scratch, s_site, 0, s_noise, s_vd);
}

}  // namespace gdrf
