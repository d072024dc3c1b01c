// Segment-aware optimizer update (gdrf_optim_step): the pyro.optim rules of gdrf/train_script.py:73-87 other than the plain Adam family
// path of adam_kernel, with pyro's per-parameter clip_args and optim_args.  pyro keeps one torch optimizer per parameter tensor, so every
// scalar (learning rate, bias corrections, clip thresholds, ...) belongs to one segment of the flat parameter vector: a named parameter
// tensor of Engine.named_views().  The host computes them in double for each step and passes the whole table as a kernel argument;
// elements outside every segment are never touched.  Arithmetic is double in registers, stored in the context's element type.
//
// Launches: opt_sumsq_kernel (only when a segment clips by norm) writes one sum of squares of the gradient per workgroup of OPT_NRM
// elements; opt_update_kernel then sums the partials of its segment in a fixed order (every workgroup of a segment forms the same total,
// bitwise: no float atomics) and applies the rule.  Both return at once when the step's Cholesky factorisation failed (flag[0]), so that
// parameters and every state stay as they were, like adam_kernel.
#pragma once
#include "../../include/gdrf_hip.h"

namespace gdrf {

constexpr int OPT_MAX_SEGS = 24;     // segments per launch (the table travels as a kernel argument, about 2.7 KB)
constexpr int OPT_THREADS = 256;
constexpr int OPT_UPD = 1024;        // elements per workgroup of the update: 4 per thread
constexpr int OPT_NRM = 8192;        // elements per workgroup of the sum-of-squares pass: 32 per thread

struct OptTable {
  int nseg;
  int ub[OPT_MAX_SEGS + 1];          // first update workgroup of each segment (ub[nseg] = grid)
  int nb[OPT_MAX_SEGS + 1];          // first sum-of-squares workgroup (= partial) of each segment; none for segments without clip_norm
  gdrf_opt_seg seg[OPT_MAX_SEGS];
};

// the segment a workgroup belongs to: the last s with start[s] <= b (segments without workgroups are skipped)
__device__ inline int opt_find(const int* start, int nseg, int b) {
  int s = 0;
  while (s + 1 < nseg && b >= start[s + 1]) ++s;
  return s;
}

// sum over the 256 threads of a workgroup in a fixed order (butterfly within each wave, then the four wave sums)
__device__ inline double opt_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double t = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return t;
}

template <typename T>
__global__ __launch_bounds__(OPT_THREADS) void opt_sumsq_kernel(const OptTable tab, const T* __restrict__ g, double* __restrict__ part,
                                                                 const int* __restrict__ flag) {
  if (flag && *flag) return;
  __shared__ double red[4];
  const int b = blockIdx.x;
  const int s = opt_find(tab.nb, tab.nseg, b);
  const int64_t off = tab.seg[s].offset, len = tab.seg[s].length;
  const int64_t base = (int64_t)(b - tab.nb[s]) * OPT_NRM;
  const int64_t end = base + OPT_NRM < len ? base + OPT_NRM : len;
  double acc = 0;
  for (int64_t i = base + threadIdx.x; i < end; i += OPT_THREADS) {
    const double x = (double)g[off + i];
    acc = fma(x, x, acc);
  }
  acc = opt_block_sum(acc, red);
  if (threadIdx.x == 0) part[b] = acc;
}

template <typename T>
__global__ __launch_bounds__(OPT_THREADS) void opt_update_kernel(const OptTable tab, int rule, T* __restrict__ p, const T* __restrict__ g,
                                                                 T* __restrict__ s1, T* __restrict__ s2, T* __restrict__ s3,
                                                                 const double* __restrict__ part, const int* __restrict__ flag) {
  if (flag && *flag) return;
  __shared__ double red[4];
  const int b = blockIdx.x;
  const int s = opt_find(tab.ub, tab.nseg, b);
  const int64_t off = tab.seg[s].offset, len = tab.seg[s].length;
  const int flags = tab.seg[s].flags;
  double a[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = tab.seg[s].a[k];
  // clip_grad_norm_(p, c): coef = c / (|g|_2 + 1e-6), applied only when < 1
  double scale = 1.0;
  if (flags & GDRF_OPT_CLIP_NORM) {
    double acc = 0;
    for (int j = tab.nb[s] + threadIdx.x; j < tab.nb[s + 1]; j += OPT_THREADS) acc += part[j];
    const double coef = tab.seg[s].clip_norm / (sqrt(opt_block_sum(acc, red)) + 1e-6);
    if (coef < 1.0) scale = coef;
  }
  const bool clipv = (flags & GDRF_OPT_CLIP_VALUE) != 0;
  const double cv = tab.seg[s].clip_value;
  const int64_t base = (int64_t)(b - tab.ub[s]) * OPT_UPD;
#pragma unroll
  for (int j = 0; j < OPT_UPD / OPT_THREADS; ++j) {
    const int64_t li = base + j * OPT_THREADS + threadIdx.x;
    if (li >= len) break;
    const int64_t i = off + li;
    double gi = (double)g[i] * scale, pi = (double)p[i];
    if (clipv) gi = fmin(fmax(gi, -cv), cv);                                   // clip_grad_value_
    switch (rule) {
      case GDRF_ADAM: case GDRF_ADAMW: case GDRF_CLIPPED_ADAM: {                // a = {lr, b1, b2, eps, wd, clip, bc1, bc2}: adam_kernel's arithmetic
        if (rule == GDRF_CLIPPED_ADAM) gi = fmin(fmax(gi, -a[5]), a[5]);
        if (rule == GDRF_ADAMW) pi *= (1.0 - a[0] * a[4]);
        const double mi = a[1] * (double)s1[i] + (1.0 - a[1]) * gi;
        const double vi = a[2] * (double)s2[i] + (1.0 - a[2]) * gi * gi;
        s1[i] = (T)mi; s2[i] = (T)vi;
        if (rule == GDRF_CLIPPED_ADAM) pi -= a[0] * sqrt(a[7]) / a[6] * mi / (sqrt(vi) + a[3]);
        else pi -= (a[0] / a[6]) * mi / (sqrt(vi) / sqrt(a[7]) + a[3]);
        break;
      }
      case GDRF_ADAMAX: {                                                       // a = {lr / (1 - b1^t), b1, b2, eps, wd}; s1 exp_avg, s2 exp_inf
        gi += a[4] * pi;
        const double mi = a[1] * (double)s1[i] + (1.0 - a[1]) * gi;
        const double ui = fmax(a[2] * (double)s2[i], fabs(gi) + a[3]);
        s1[i] = (T)mi; s2[i] = (T)ui;
        pi -= a[0] * (mi / ui);
        break;
      }
      case GDRF_RMSPROP: {                                                      // a = {lr, alpha, eps, wd, momentum}; s2 square_avg,
        gi += a[3] * pi;                                                        // s1 momentum_buffer, grad_avg in s3 (both) or s1 (centered only)
        const double vi = a[1] * (double)s2[i] + (1.0 - a[1]) * gi * gi;
        s2[i] = (T)vi;
        double den;
        if (flags & GDRF_OPT_CENTERED) {
          T* ga = (flags & GDRF_OPT_MOMENTUM) ? s3 : s1;
          const double ai = a[1] * (double)ga[i] + (1.0 - a[1]) * gi;
          ga[i] = (T)ai;
          den = sqrt(vi - ai * ai) + a[2];
        } else {
          den = sqrt(vi) + a[2];
        }
        if (flags & GDRF_OPT_MOMENTUM) {
          const double bi = a[4] * (double)s1[i] + gi / den;
          s1[i] = (T)bi;
          pi -= a[0] * bi;
        } else {
          pi -= a[0] * (gi / den);
        }
        break;
      }
      case GDRF_ADAGRAD: {                                                      // a = {lr / (1 + (t - 1) lr_decay), eps, wd}; s2 sum
        gi += a[2] * pi;
        const double si = (double)s2[i] + gi * gi;
        s2[i] = (T)si;
        pi -= a[0] * (gi / (sqrt(si) + a[1]));
        break;
      }
      case GDRF_ADADELTA: {                                                     // a = {lr, rho, eps, wd}; s2 square_avg, s1 acc_delta
        gi += a[3] * pi;
        const double vi = a[1] * (double)s2[i] + (1.0 - a[1]) * gi * gi;
        const double di = sqrt((double)s1[i] + a[2]) / sqrt(vi + a[2]) * gi;
        const double ci = a[1] * (double)s1[i] + (1.0 - a[1]) * di * di;
        s2[i] = (T)vi; s1[i] = (T)ci;
        pi -= a[0] * di;
        break;
      }
      case GDRF_ASGD: {                                                         // a = {eta, mu, lambd, wd}; s1 ax
        gi += a[3] * pi;
        pi = pi * (1.0 - a[2] * a[0]) - a[0] * gi;
        const double pt = (double)(T)pi;                                         // ax follows the stored parameter
        s1[i] = (T)(a[1] == 1.0 ? pt : (double)s1[i] + a[1] * (pt - (double)s1[i]));
        break;
      }
      case GDRF_RPROP: {                                                        // a = {eta-, eta+, step min, step max}; s1 prev, s2 step_size
        const double pr = (double)s1[i] * gi;
        const double f = pr > 0.0 ? a[1] : (pr < 0.0 ? a[0] : 1.0);
        const double st = fmin(fmax((double)s2[i] * f, a[2]), a[3]);
        if (f == a[0]) gi = 0.0;                                                // torch: grad[sign == etaminus] = 0
        s2[i] = (T)st; s1[i] = (T)gi;
        pi -= (gi > 0.0 ? st : (gi < 0.0 ? -st : 0.0));
        break;
      }
      case GDRF_ADAGRAD_RMSPROP: {                                              // a = {eta t^(-1/2 + delta), tau, first step}; s2 sum
        const double si = a[2] != 0.0 ? gi * gi : (1.0 - a[1]) * (double)s2[i] + a[1] * gi * gi;
        s2[i] = (T)si;
        pi -= a[0] * (gi / (1.0 + sqrt(si)));
        break;
      }
      default: break;
    }
    p[i] = (T)pi;
  }
}

}  // namespace gdrf
