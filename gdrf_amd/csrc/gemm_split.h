// The f32 GEMM-shaped contractions of the step on the 16-bit matrix path with split-operand emulation.
//
// gfx950 runs f32-input MFMA at 1/16 of the bf16 / f16 rate (MI355X_MICROARCH.md: 157 TF vs ~2.5 PF), and ~85 % of the step
// is bound by it.  Every f32 operand is written as a short sum of 16-bit pieces and a product a*b as the sum of the cross
// terms that matter, accumulated in f32 by v_mfma_f32_16x16x32_{f16,bf16}.  Two policies:
//
//   SplitF16  ("f16x3", default): x 2^e = h + l with fp16 pieces (h = f16(y), l = f16(y - h): 11 + 11 significand bits and the
//             sign of the residual, |y - h - l| <= 2^-23 |y|), products hh + hl + lh; the dropped ll term is <= 2^-22 |ab| and
//             random in sign.  fp16 has 5 exponent bits, so every operand carries ONE power-of-two block scale 2^e that puts its
//             largest magnitude just below 2^15 (bound known: |W| <= sqrt(variance); measured: max |B_k|, max |S_k|, max |vbar_k|,
//             max |Wbar|, by order-independent integer atomicMax); elements down to 2^-18 of the block maximum keep the full 22
//             bits, smaller ones an ABSOLUTE error of 2^-40 of the maximum - negligible in a sum whose f32 accumulation already
//             rounds at 2^-24 of the running total.  The scales are exact (powers of two) and undone in the epilogues.
//             3 MFMAs per f32 multiply-add: 16/3 = 5.3x the f32 MFMA rate, and 3 (not 6 or 32) accumulator roundings per 32
//             reduction indices.
//   SplitBf16 ("bf16x6"): x = x1 + x2 + x3 with bf16 pieces (3 x 8 bits, exact to 2^-24 |x|, f32's exponent range, no scaling),
//             the six cross terms of weight >= 2^-16.  2.7x the f32 MFMA rate.  Kept selectable (mfma_mode).
//
// Both are held to the error of the native f32 MFMA kernels on the same inputs, measured against fp64 products
// (tests/test_gpu_parity.py::test_split_modes_against_fp64_product_of_the_same_inputs).
//
//   split_kernel / split_blocked_kernel   W, B_k = S_k S_k^T and S_k^T -> pieces, once per step (W's come from fwd_w's epilogue)
//   bwd_wbar_split_kernel    Wbar = sum_k diag(2 vbar_k) W B_k + locbar^T U - 2 diag(asum) W   (replaces gemm_nt<BwdWbarProb>)
//   fwd_t_split_cc_kernel / fwd_t_split_q4_kernel   tt[k][n] = |S_k^T w_n|^2                      (replace gemm_nt<FwdTProb>)
//   gemm_tn_split_kernel     A_k = W^T diag(vbar_k) W  and  GT = W^T Wbar                        (replaces gemm_tn_kernel<float>)
//
// All keep the tiling, block maps, deterministic slab reduction and epilogues of the f32 forms they replace.
#pragma once
#include <utility>
#include "common.h"
#include "gemm_nt.h"
#include "kernels_mm.h"

namespace gdrf {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct SplitBf16 {
  using E = __bf16; using V8 = bf16x8; using V4 = bf16x4;
  static constexpr int NP = 3, NPROD = 6, ID = 1;
  // cross products (piece of A, piece of B), smallest weight first
  static __device__ __forceinline__ constexpr int pa(int t) { constexpr int v[6] = {0, 1, 2, 0, 1, 0}; return v[t]; }
  static __device__ __forceinline__ constexpr int pb(int t) { constexpr int v[6] = {2, 1, 0, 1, 0, 0}; return v[t]; }
  static __device__ __forceinline__ f32x4 mma(V8 a, V8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ void split(float x, E (&p)[NP]) {
    p[0] = (__bf16)x;
    const float r1 = x - (float)p[0];
    p[1] = (__bf16)r1;
    p[2] = (__bf16)(r1 - (float)p[1]);
  }
};
struct SplitF16 {
  using E = _Float16; using V8 = f16x8; using V4 = f16x4;
  static constexpr int NP = 2, NPROD = 3, ID = 2;
  static __device__ __forceinline__ constexpr int pa(int t) { constexpr int v[3] = {0, 1, 0}; return v[t]; }
  static __device__ __forceinline__ constexpr int pb(int t) { constexpr int v[3] = {1, 0, 0}; return v[t]; }
  static __device__ __forceinline__ f32x4 mma(V8 a, V8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ void split(float y, E (&p)[NP]) {     // y = x * block scale
    p[0] = (_Float16)y;
    p[1] = (_Float16)(y - (float)p[0]);
  }
};

// ---- block scales -------------------------------------------------------------------------------------------------
// Device float array of (scale, 1 / scale) pairs and the unsigned array of maxima (bit patterns of non-negative floats, which
// order like the floats) they come from.  SplitBf16 runs with every scale = 1.
struct SplitLay {
  int K;
  __host__ __device__ int w() const { return 0; }                    // W: from the bound |W| <= sqrt(variance)
  __host__ __device__ int wbar() const { return 2; }
  __host__ __device__ int b(int k) const { return 4 + 2 * k; }
  __host__ __device__ int st(int k) const { return 4 + 2 * K + 2 * k; }
  __host__ __device__ int v(int k) const { return 4 + 4 * K + 2 * k; }
  __host__ __device__ int dk() const { return 4 + 6 * K; }          // dK_nm / d log(lengthscale): from the bound |dK| <= 0.75 variance (hyper_tn.h)
  __host__ __device__ int nfloats() const { return 6 + 6 * K; }
  __host__ __device__ int mx_wbar() const { return 0; }
  __host__ __device__ int mx_b(int k) const { return 1 + k; }
  __host__ __device__ int mx_st(int k) const { return 1 + K + k; }
  __host__ __device__ int mx_v(int k) const { return 1 + 2 * K + k; }
  __host__ __device__ int nmax() const { return 1 + 3 * K; }
};
// power of two s with bound * s in [2^(top-1), 2^top)
__device__ __forceinline__ float split_pow2_scale(float bound, int top) {
  if (!(bound > 0.0f) || !(bound < 3.0e38f)) return 1.0f;
  int ex;
  (void)frexpf(bound, &ex);                 // bound = m 2^ex, m in [0.5, 1)
  int e = top - ex;
  e = e > 100 ? 100 : (e < -100 ? -100 : e);
  return ldexpf(1.0f, e);
}
enum { SPLIT_SC_W = 1, SPLIT_SC_BST = 2, SPLIT_SC_V = 4, SPLIT_SC_WBAR = 8 };
// what: which groups to (re)compute.  f16 = 0 writes ones.
__global__ void split_scales_kernel(int f16, const Hyper* __restrict__ h, const unsigned* __restrict__ mx, float* __restrict__ sc, int K, int what) {
  const SplitLay L{K};
  auto put = [&](int idx, float s) { sc[idx] = s; sc[idx + 1] = 1.0f / s; };
  const int t = threadIdx.x;
  if ((what & SPLIT_SC_W) && t == 0)          // |w_nj| <= ||w_n|| <= sqrt(k(x,x)) = sqrt(variance); 4x headroom for rounding in the solve
    put(L.w(), f16 ? split_pow2_scale(sqrtf((float)h->var), 13) : 1.0f);
  // |dk / d log ls| <= 0.75 variance for every kernel kind (RBF: k r^2 <= 2/e var; Matern-5/2: 0.59 var; Matern-3/2: 0.54; exponential: 0.37)
  if ((what & SPLIT_SC_W) && t == 0) put(L.dk(), f16 ? split_pow2_scale(0.75f * (float)h->var, 15) : 1.0f);
  if ((what & SPLIT_SC_WBAR) && t == 0) put(L.wbar(), f16 ? split_pow2_scale(__uint_as_float(mx[L.mx_wbar()]), 15) : 1.0f);
  for (int k = t; k < K; k += blockDim.x) {
    if (what & SPLIT_SC_BST) {
      put(L.b(k), f16 ? split_pow2_scale(__uint_as_float(mx[L.mx_b(k)]), 15) : 1.0f);
      put(L.st(k), f16 ? split_pow2_scale(__uint_as_float(mx[L.mx_st(k)]), 15) : 1.0f);
    }
    // operand of the A_k contraction: vbar_kn w_nj, bounded by max_n |vbar_kn| sqrt(variance) (same 4x headroom as W)
    if (what & SPLIT_SC_V) put(L.v(k), f16 ? split_pow2_scale(__uint_as_float(mx[L.mx_v(k)]) * sqrtf((float)h->var), 13) : 1.0f);
  }
}
// A wave's maximum of m >= 0 (one value per lane) into *mx.  Order-independent, hence deterministic: non-negative floats order like their
// bit patterns, so the butterfly and the integer atomicMax give the same bits whichever wave or workgroup arrives first.  A zero is not
// published (mx starts at zero: zeroed by the caller).  Call it with the whole wave.
__device__ __forceinline__ void wave_max_publish(unsigned* mx, float m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(mx, __float_as_uint(m));
}

// mx[b] = max |x[b][i]|, i < n (grid: (blocks, batches)); mx zeroed by the caller
__global__ __launch_bounds__(256) void absmax_batched_kernel(const float* __restrict__ x, int64_t n, int64_t ld, unsigned* __restrict__ mx) {
  const int b = blockIdx.y;
  float m = 0;
  const f32x4* p = reinterpret_cast<const f32x4*>(x + (int64_t)b * ld);          // ld a multiple of 4
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n >> 2); i += (int64_t)gridDim.x * blockDim.x) {
    const f32x4 v = p[i];
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) m = fmaxf(m, fabsf(x[(int64_t)b * ld + (n & ~(int64_t)3) + threadIdx.x]));
  wave_max_publish(mx + b, m);
}

template <class SP> struct SplitCfg {
  static constexpr int BK = 32;                 // f32 reduction indices per chunk = one 16x16x32 MFMA deep
  static constexpr int LDH = BK;                // LDS row = 32 halfwords = 64 bytes = four 16-byte quads, no padding
  static constexpr int PIECE = GDRF_TILE * LDH; // halfwords per piece image of a 128-row operand tile
  static constexpr int IMG = SP::NP * PIECE;    // halfwords per operand image
  static constexpr int LDS_BYTES = 2 * IMG * 2; // A and B images
};
// LDS image of an operand tile: element (row, k) lives at halfword  row*32 + ((k>>3) ^ swz(row))*8 + (k&7), swz(row) = 3 if
// (row & 8) else 0.  ds_read_b128 serves a wave in the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, ... with bank =
// dword mod 64 (MI355X_MICROARCH.md, LDS): an MFMA fragment read (lane -> row lane&15, quad lane>>4) then touches, in every
// group, all 16 (row mod 4, physical quad) pairs exactly once - conflict-free; a padded 80-byte row is not (measured: 47 %
// of the LDS cycles were bank conflicts).  ds_write_b128 (8 contiguous lanes = 2 whole rows = 32 distinct banks) is too.
__device__ __forceinline__ int split_swz(int row) { return (row & 8) ? 3 : 0; }
__device__ __forceinline__ int split_off(int row, int k) { return row * 32 + (((k >> 3) ^ split_swz(row)) << 3) + (k & 7); }

// LDS-DMA issued from inline asm: hipcc then neither counts it nor - which is the point - drains it with a vmcnt(0) in front of the
// next LDS read of the issuing wave (a builtin glds is a pending LDS write to the compiler, so every ds_read behind it waits for it:
// the "prefetch" of the next chunk was retired BEFORE the current chunk's MFMAs).  The caller orders it by hand: it is older than
// any register load issued after it, vmcnt retires in order, so the wait hipcc puts in front of the first use of such a load also
// covers it; a barrier then publishes it to the other waves.  M0 is written in the statement that reads it
// (cdna_hip_programming.md 5.7).  lds_dst: wave-uniform LDS byte address; gsrc: this lane's 16 source bytes.
__device__ __forceinline__ void glds16_asm(const void* gsrc, unsigned lds_dst) {
  // M0 is not restored: a write to M0 directly behind the DMA waits until the DMA has consumed it - measured ~100-200 cycles of wave
  // stall per request.  Nothing else in these kernels uses M0 (no builtin LDS-DMA, no s_movrel / sendmsg; DS instructions do not need
  // it on gfx9+), and every statement that needs it sets it itself.
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(gsrc), "s"(lds_dst) : "memory");
}
// the same with a wave-uniform 64-bit base (scalar registers) and a 32-bit unsigned byte offset per lane: one address VGPR instead of two
__device__ __forceinline__ void glds16_asm_s(const void* sbase, unsigned voff, unsigned lds_dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const void*)p;
}

// compile-time loop: f(std::integral_constant<int, 0>{}), ..., f(std::integral_constant<int, N - 1>{}).  (A `#pragma unroll` of 20 stages x 24
// MFMAs with inline asm in the body is refused by hipcc's unroller - "loop not unrolled" - and the accumulator arrays land in scratch.)
template <int... Is, class F> __device__ __forceinline__ void static_for_impl(std::integer_sequence<int, Is...>, F&& f) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F> __device__ __forceinline__ void static_for(F&& f) { static_for_impl(std::make_integer_sequence<int, N>{}, f); }

// ---- device helpers shared by the W-bar and tt kernels ------------------------------------------------------------------------
// A kernel below is its staging and its phase schedule on top of these.  All of them inline; what a kernel does not use costs nothing.

// Where a thread sits in its wave group: 256 threads = 4 waves as 2 x 2 on a 128 x 128 tile, each wave 4 x 4 MFMA tiles of 16 x 16.
// The derived values are functions: a kernel takes the ones it needs where its schedule wants them computed (computed up front, in the
// constructor, they cost bwd_wbar_split_cc_kernel two registers and bwd_wbar_f16_k64_kernel 60 bytes of scratch).
struct SplitLane {
  int tid, lane, wave;   // inside the wave group
  int wr, wc;            // the wave's 64-row / 64-column quadrant of the tile
  int lr, lg;            // MFMA operand lane: row (A) or column (B) lr of a 16-row group, k quad lg; accumulator: column lr, rows 4 lg + r
  __device__ __forceinline__ SplitLane() {
    tid = threadIdx.x & 255; lane = tid & 63; wave = tid >> 6;
    wr = wave >> 1; wc = wave & 1; lr = lane & 15; lg = lane >> 4;
  }
  // = wave, provably wave-uniform: a DMA's LDS base goes to M0 without a waterfall loop
  __device__ __forceinline__ int wave_u() const { return __builtin_amdgcn_readfirstlane(wave); }
  // this lane's fragment offset (halfwords) inside a 16-row group of a swizzled image
  __device__ __forceinline__ int frag() const { return lr * 32 + ((lg ^ split_swz(lr)) << 3); }
  // LDS-DMA (global_load_lds_dwordx4): one wave-instruction moves a 16-row block of one piece image, 1 KB: lane l lands at block + 16 l =
  // row l>>2, physical quad l&3, so its SOURCE is logical quad (l&3) ^ swz(row) - the image swizzle goes on the global address
  // (cdna_hip_programming.md 5.4 rule 21): row drow of the block, halfword dq of the 32-deep chunk
  __device__ __forceinline__ int drow() const { return lane >> 2; }
  __device__ __forceinline__ int dq() const { return ((lane & 3) ^ split_swz(drow())) * 8; }
};

__device__ __forceinline__ void split_zero(f32x4 (&acc)[4][4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0, 0, 0, 0};
}
// this lane's MFMA fragment (8 halfwords) of piece p of a swizzled operand image, for the 16 rows from row0
template <class SP> __device__ __forceinline__ typename SP::V8 split_frag(const typename SP::E* img, int p, int row0, int frag) {
  return *reinterpret_cast<const typename SP::V8*>(img + p * SplitCfg<SP>::PIECE + row0 * 32 + frag);
}
// the same for all pieces
template <class SP> __device__ __forceinline__ void split_frags(typename SP::V8 (&f)[SP::NP], const typename SP::E* img, int row0, int frag) {
#pragma unroll
  for (int p = 0; p < SP::NP; ++p) f[p] = split_frag<SP>(img, p, row0, frag);
}
// P (+)= A B^T, a wave's four 16-row groups against one 16-column group, through the cross products in the order SP::pa/pb(t), small terms
// first; FIRST: P starts from zero
template <class SP, bool FIRST>
__device__ __forceinline__ void split_products(f32x4 (&P)[4], const typename SP::V8 (&fa)[4][SP::NP], const typename SP::V8 (&fb)[SP::NP]) {
#pragma unroll
  for (int t = 0; t < SP::NPROD; ++t)
#pragma unroll
    for (int a = 0; a < 4; ++a) P[a] = SP::mma(fa[a][SP::pa(t)], fb[SP::pb(t)], (FIRST && t == 0) ? f32x4{0, 0, 0, 0} : P[a]);
}
// the per-row factors of a wave's accumulator rows (4 lg + r of each 16-row group) from one topic's row of a [K][128] table in LDS
__device__ __forceinline__ void split_row_scales(f32x4 (&s4)[4], const float* sc_row, const SplitLane& L) {
#pragma unroll
  for (int a = 0; a < 4; ++a) s4[a] = *reinterpret_cast<const f32x4*>(sc_row + L.wr * 64 + a * 16 + L.lg * 4);
}
// acc[.][b] += diag(s4) P, column group b
__device__ __forceinline__ void split_scaled_acc(f32x4 (&acc)[4][4], int b, const f32x4 (&s4)[4], const f32x4 (&P)[4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[a][b][r] += s4[a][r] * P[a][r];
}
// End of a phase of the concurrent forms.  vmcnt(0): this wave's DMAs of the next chunk have landed (they were requested inside the phase and
// had it to land); lgkmcnt(0): its fragment reads of this chunk are done; the barrier publishes both, so that after it every wave may
// read the buffers just filled and request into the buffers just read.  A raw s_barrier: the waits it needs stand in front of it.
__device__ __forceinline__ void split_phase_end() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  gdrf_raw_barrier();
}


// out[p * stride + i] = p-th piece of in[i] * scale; 4 elements per thread (n multiple of 4)
template <class SP>
__global__ void split_kernel(const float* __restrict__ in, int64_t n, typename SP::E* __restrict__ out, int64_t stride, const float* __restrict__ scale) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= n) return;
  const float s = scale[0];
  const f32x4 x = *reinterpret_cast<const f32x4*>(in + i);
  typename SP::V4 pv[SP::NP];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    typename SP::E p[SP::NP];
    SP::split(x[e] * s, p);
#pragma unroll
    for (int q = 0; q < SP::NP; ++q) pv[q][e] = p[q];
  }
#pragma unroll
  for (int q = 0; q < SP::NP; ++q) *reinterpret_cast<typename SP::V4*>(out + q * stride + i) = pv[q];
}

// the same pieces in k-blocked order for the NT kernels' small operands (B_k, S_k^T):  in[b][r][c] (b < nb, r < R, c < C, C a
// multiple of 32)  ->  out[p][b][c / 32][r][c % 32], batch b scaled by scale[2 b].  A tile's 32-wide reduction chunk is then ONE
// contiguous block of whole 128-byte lines (rows x 64 B), instead of 64 B out of every 1 KB row: the row-major form left the
// load path saturated (measured: ~4000 cycles per prefetched load, 1500 of every 4600 cycles per chunk spent waiting for them).
template <class SP>
__global__ void split_blocked_kernel(const float* __restrict__ in, int64_t n, int R, int C, typename SP::E* __restrict__ out, int64_t stride,
                                     const float* __restrict__ scale) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= n) return;
  const int64_t rc = (int64_t)R * C, b = i / rc, rem = i - b * rc;
  const float s = scale[2 * b];
  const f32x4 x = *reinterpret_cast<const f32x4*>(in + i);
  typename SP::V4 pv[SP::NP];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    typename SP::E p[SP::NP];
    SP::split(x[e] * s, p);
#pragma unroll
    for (int q = 0; q < SP::NP; ++q) pv[q][e] = p[q];
  }
  const int r = (int)(rem / C), c = (int)(rem - (int64_t)r * C);
  const int64_t o = b * rc + ((int64_t)(c >> 5) * R + r) * 32 + (c & 31);
#pragma unroll
  for (int q = 0; q < SP::NP; ++q) *reinterpret_cast<typename SP::V4*>(out + q * stride + o) = pv[q];
}

template <class SP> struct BwdWbarSplitArgs {
  const float* W; const typename SP::E* Wh; int64_t w_stride;   // W (f32, epilogue) and its pieces [p][row][Mp]
  int64_t nrows; int M, Mp, K;
  const typename SP::E* Bh; int64_t piece_stride;     // Bh[p][k][i / 32][col][i % 32] (k-blocked), piece_stride = K*Mp*Mp
  const float* vbar; const float* locbar; int64_t ldk;
  const float* asum; const float* U; float* Wbar;
  const float* sc;                             // block scales (SplitLay)
  unsigned* wbar_max;                          // max |Wbar| (bits), for the scale of the G^T contraction's operand
  // bwd_wbar_f16_k64_kernel only, few rows (mini-batches): gridDim.y = nslice slices of the reduction blocks, slice y writes its partial
  // sum to slab + y * slab_stride (slice 0 carries the rank-K and the -2 a W terms); wbar_slab_sum_kernel adds them into Wbar
  float* slab = nullptr; int64_t slab_stride = 0; int nslice = 1;
};

// the [K][128] table of the per-(topic, row) factors of the row tile at m0: 2 vbar_kn, with the block scales of W and B_k taken off;
// rows past the end get 0.  Filled by the 256 threads of a wave group; a barrier publishes it.
template <class SP> __device__ __forceinline__ void wbar_fill_scales(const BwdWbarSplitArgs<SP>& g, float* scaleS, int64_t m0, int tid) {
  const SplitLay SL{g.K};
  const float unw = g.sc[SL.w() + 1];
  for (int e = tid; e < g.K * GDRF_TILE; e += 256) {
    const int k = e / GDRF_TILE, r = e - k * GDRF_TILE;
    scaleS[e] = (m0 + r < g.nrows) ? 2.0f * g.vbar[(int64_t)k * g.ldk + m0 + r] * (unw * g.sc[SL.b(k) + 1]) : 0.0f;
  }
}
// rank-K epilogue term locbar^T U on the native f32 matrix instruction (exact f32, no split, no range question): lane (lr, lg) supplies
// A[row lr][k = lg] and B[k = lg][col lr] of v_mfma_f32_16x16x4_f32, whose C/D layout is the accumulators'.  Four topics per round of loads
// (bwd_wbar_f16_k64_kernel batches sixteen and keeps its own form).
template <class SP>
__device__ __forceinline__ void wbar_rank_k(f32x4 (&acc)[4][4], const BwdWbarSplitArgs<SP>& g, int64_t m0, int n0, const SplitLane& L) {
  for (int k0 = 0; k0 < g.K; k0 += 4) {
    const int k = k0 + L.lg;
    float av[4], bv[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int64_t row = m0 + L.wr * 64 + a * 16 + L.lr;
      av[a] = (k < g.K && row < g.nrows) ? g.locbar[(int64_t)k * g.ldk + row] : 0.0f;
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int col = n0 + L.wc * 64 + b * 16 + L.lr;
      bv[b] = (k < g.K && col < g.M) ? g.U[(int64_t)k * g.M + col] : 0.0f;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b], acc[a][b], 0, 0, 0);
  }
}
// The epilogue Wbar = acc - 2 asum W of a wave's 64 x 64 quadrant; returns the lane's max |Wbar|.  The MFMA accumulator layout (a lane owns
// one column of four rows) would make this 64 scalar loads of W and 64 scalar stores per lane in a dependent sequence - measured ~300k
// cycles per workgroup, a third of its lifetime.  Instead each wave transposes its quadrant through a private LDS tile (over the operand
// images, which every wave is done with after the barrier), 32 rows at a time, and moves whole 256-byte row segments: 16 float4 loads and
// 16 float4 stores per lane.  In round i (of 8) of half h a lane moves row wbar_seg_row, columns wbar_seg_col .. + 3 of the tile; Mp is a
// multiple of 32, so a float4 never straddles the edge.  The pieces: the wave's tile, half h of the accumulators into it, a lane's
// segment out of it, and o = t - as2 w stored with the running maximum; wbar_store_transposed puts them together with W and asum loaded
// behind the bounds test (bwd_wbar_f16_k64_kernel puts them together itself, with the values it loaded up front).
constexpr int WBAR_TS = 68;   // tile row stride in floats (272 B: 16-byte aligned, bank-shifted)
__device__ __forceinline__ float* wbar_tile(char* smem, int gp, const SplitLane& L) {
  return reinterpret_cast<float*>(smem) + (size_t)(gp * 4 + L.wave) * (32 * WBAR_TS);
}
__device__ __forceinline__ void wbar_tile_put(float* tile, const f32x4 (&acc)[4][4], int h, const SplitLane& L) {
#pragma unroll
  for (int a2 = 0; a2 < 2; ++a2)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) tile[(a2 * 16 + L.lg * 4 + r) * WBAR_TS + b * 16 + L.lr] = acc[2 * h + a2][b][r];
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         // same wave writes and reads: LDS is in order per wave
}
__device__ __forceinline__ f32x4 wbar_tile_get(const float* tile, int i, const SplitLane& L) {
  return *reinterpret_cast<const f32x4*>(tile + ((L.lane >> 4) + 4 * i) * WBAR_TS + (L.lane & 15) * 4);
}
__device__ __forceinline__ int wbar_seg_row(const SplitLane& L, int h, int i) { return L.wr * 64 + h * 32 + (L.lane >> 4) + 4 * i; }
__device__ __forceinline__ int wbar_seg_col(const SplitLane& L) { return L.wc * 64 + (L.lane & 15) * 4; }
__device__ __forceinline__ void wbar_seg_store(float* dst, const f32x4& t, float as2, const f32x4& w, float& wmax) {
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) { o[e] = t[e] - as2 * w[e]; wmax = fmaxf(wmax, fabsf(o[e])); }
  *reinterpret_cast<f32x4*>(dst) = o;
}
template <class SP>
__device__ __forceinline__ float wbar_store_transposed(const f32x4 (&acc)[4][4], char* smem, int gp, const SplitLane& L, const BwdWbarSplitArgs<SP>& g,
                                                       int64_t m0, int n0) {
  __syncthreads();                                           // every wave is done with the operand images
  float wmax = 0.0f;
  float* tile = wbar_tile(smem, gp, L);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    wbar_tile_put(tile, acc, h, L);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int64_t m = m0 + wbar_seg_row(L, h, i);
      const int n = n0 + wbar_seg_col(L);
      const f32x4 t = wbar_tile_get(tile, i, L);
      if (m < g.nrows && n < g.Mp)
        wbar_seg_store(g.Wbar + m * g.Mp + n, t, 2.0f * g.asum[m], *reinterpret_cast<const f32x4*>(g.W + m * g.Mp + n), wmax);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // reads done before the tile is overwritten with the other half
  }
  return wmax;
}

// NG = 1: one 256-thread workgroup per tile, two workgroups per CU (they share the CU's SIMDs at random).
// NG = 2: one 512-thread workgroup per CU holding TWO such tiles, one per wave group (waves 0-3 / 4-7: a workgroup's waves
// go to the SIMDs cyclically, so every SIMD hosts one wave of each group), run phase-shifted on purpose: in every phase one
// group multiplies its staged chunk while the other issues the LDS-DMA loads of the one after, then they swap.  Measured
// cause (s_memtime per wave, NG = 1): the multiply phase is 1810 cycles (MFMA 1536) but every wave then waits ~1500 cycles at
// the barrier - each SIMD's two waves contend for the matrix pipe at random and the barrier paces a workgroup by its
// unluckiest wave.  With the groups alternating, the multiplying wave has its SIMD's pipe to itself and the staging hides
// behind it.  The phase barrier is a raw s_barrier after s_waitcnt lgkmcnt(0): a __syncthreads() would also drain vmcnt and
// wait for the prefetch just issued.
template <class SP, int NG>
__global__ __launch_bounds__(256 * NG, 2) void bwd_wbar_split_kernel(BwdWbarSplitArgs<SP> g) {
  using CF = SplitCfg<SP>;
  using E = typename SP::E;
  using V8 = typename SP::V8;
  constexpr int NP = SP::NP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int gp = NG == 2 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8)) : 0;
  // LDS: NG = 1: [A][B][scale];  NG = 2: [A of group 0][A of group 1][B buffer 0][B buffer 1][scale 0][scale 1] - the two
  // groups work on the same column tile, so the B chunk is staged ONCE (by group 1) into a double-buffered image both read
  constexpr int IMG = CF::IMG;
  const size_t tab = ((size_t)g.K * GDRF_TILE * sizeof(float) + 15) & ~(size_t)15;
  E* As = reinterpret_cast<E*>(smem) + (NG == 2 ? gp * IMG : 0);              // [NP][128][LDH]
  E* Bs = reinterpret_cast<E*>(smem) + (NG == 2 ? 2 * IMG : IMG);             // [NG][NP][128][LDH]
  float* scaleS = reinterpret_cast<float*>(smem + (size_t)(NG == 2 ? 4 : 2) * IMG * 2 + (size_t)gp * tab);  // [K][128]  2 vbar_kn / (sW sB_k)

  const SplitLane L;
  const int tid = L.tid;
  const int nct = (g.Mp + GDRF_TILE - 1) / GDRF_TILE;
  int64_t rtile; int ct;
  if constexpr (NG == 1) NTXcdMap{}.map_block(blockIdx.x, nct, false, rtile, ct);
  else nt_xcd_map_paired(blockIdx.x, nct, gp, rtile, ct);
  const int64_t m0 = rtile * GDRF_TILE;
  const int n0 = ct * GDRF_TILE;
  const int K = g.K, Mp = g.Mp;
  wbar_fill_scales(g, scaleS, m0, tid);
  f32x4 acc[4][4];
  split_zero(acc);

  // staging map, both operands: per piece 2 x 16-byte vectors of 8 halfwords per thread (vector v = tid + 256 j: row v>>2,
  // k offset 8*(v&3))
  V8 ra[NP][2], rb[NP][2];
  auto load_a = [&](int kA) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int v = tid + 256 * j, kq = (v & 3) * 8;
      int64_t row = m0 + (v >> 2);
      row = row < g.nrows ? row : 0;          // rows past the end read row 0; their output rows are never stored
#pragma unroll
      for (int p = 0; p < NP; ++p) ra[p][j] = *reinterpret_cast<const V8*>(g.Wh + p * g.w_stride + row * Mp + kA + kq);
    }
  };
  auto load_b = [&](int kA, int rep) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int v = tid + 256 * j, row = v >> 2, kq = (v & 3) * 8;
      const int col = (n0 + row < Mp) ? n0 + row : 0;     // likewise: columns >= Mp are never stored
#pragma unroll
      for (int p = 0; p < NP; ++p)
        rb[p][j] = *reinterpret_cast<const V8*>(g.Bh + p * g.piece_stride + (((int64_t)rep * (Mp >> 5) + (kA >> 5)) * Mp + col) * 32 + kq);
    }
  };
  auto store_a = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int v = tid + 256 * j, off = split_off(v >> 2, (v & 3) * 8);
#pragma unroll
      for (int p = 0; p < NP; ++p) *reinterpret_cast<V8*>(As + p * CF::PIECE + off) = ra[p][j];
    }
  };
  auto store_b = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int v = tid + 256 * j, off = split_off(v >> 2, (v & 3) * 8);
#pragma unroll
      for (int p = 0; p < NP; ++p) *reinterpret_cast<V8*>(Bs + (buf * NP + p) * CF::PIECE + off) = rb[p][j];
    }
  };
  // one staged chunk: P = A B^T through the cross products (small terms first), then acc += diag(scale) P.
  // The A fragments of a chunk serve all K topic reps, so they are read from LDS once (rep 0) and stay in registers; the
  // B fragments are read one 16-column group at a time.
  V8 fa[4][NP];
  const int frag = L.frag();
  auto read_a = [&]() {
#pragma unroll
    for (int a = 0; a < 4; ++a) split_frags<SP>(fa[a], As, L.wr * 64 + a * 16, frag);
  };
  auto compute = [&](const float* sc_row /* scaleS + rep*128 */, int buf) {
    const E* Bb = Bs + buf * IMG;
    f32x4 s4[4];
    split_row_scales(s4, sc_row, L);
    V8 fbq[2][NP];                         // the next column group's fragments are read while this one multiplies
    split_frags<SP>(fbq[0], Bb, L.wc * 64, frag);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      if (b + 1 < 4) split_frags<SP>(fbq[(b + 1) & 1], Bb, L.wc * 64 + (b + 1) * 16, frag);
      f32x4 P[4];
      split_products<SP, true>(P, fa, fbq[b & 1]);
      split_scaled_acc(acc, b, s4, P);
    }
  };

  const int nk = Mp / CF::BK, nchunks = nk * K;
  if constexpr (NG == 1) {
    load_a(0);
    load_b(0, 0);
    for (int c = 0; c < nchunks; ++c) {
      const int q = c / K, rep = c - q * K;
      __syncthreads();
      if (rep == 0) store_a();
      store_b(0);
      __syncthreads();
      if (c + 1 < nchunks) {
        const int q1 = (c + 1) / K, rep1 = (c + 1) - q1 * K;
        if (rep1 == 0) load_a(q1 * CF::BK);
        load_b(q1 * CF::BK, rep1);
      }
      if (rep == 0) read_a();
      compute(scaleS + rep * GDRF_TILE, 0);
    }
  } else {
    // Staging by LDS-DMA (global_load_lds_dwordx4: no destination registers, no ds_write - a staging wave's ds_write_b128
    // were measured starving, ~1600 cycles for six, while its SIMD's other wave streams MFMAs); lane map: SplitLane.
    const int drow = L.drow(), dq = L.dq(), wave_u = L.wave_u();
    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    auto dma_b = [&](int c) {             // B chunk c -> buffer c & 1; this wave moves row blocks wave and wave + 4 of each piece
      if (c >= nchunks) return;
      const int q = c / K, rep = c - q * K;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int rbk = wave_u + 4 * i, row = rbk * 16 + drow;
        const int col = (n0 + row < Mp) ? n0 + row : 0;
#pragma unroll
        for (int p = 0; p < NP; ++p)
          __builtin_amdgcn_global_load_lds((gptr_t)(g.Bh + p * g.piece_stride + (((int64_t)rep * (Mp >> 5) + q) * Mp + col) * 32 + dq),
                                           (lptr_t)(Bs + ((c & 1) * NP + p) * CF::PIECE + rbk * 512), 16, 0, 0);
      }
    };
    auto dma_a = [&](int q) {             // this group's A image for reduction block q
      if (q >= nk) return;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int rbk = wave_u + 4 * i;
        int64_t row = m0 + rbk * 16 + drow;
        row = row < g.nrows ? row : 0;
#pragma unroll
        for (int p = 0; p < NP; ++p)
          __builtin_amdgcn_global_load_lds((gptr_t)(g.Wh + p * g.w_stride + row * Mp + q * CF::BK + dq),
                                           (lptr_t)(As + p * CF::PIECE + rbk * 512), 16, 0, 0);
      }
    };
    auto mult = [&](int c) {
      const int q = c / K, rep = c - q * K;
      if (rep == 0) read_a();
      compute(scaleS + rep * GDRF_TILE, c & 1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the DMAs this group issued one phase ago have had a whole phase
    };
    auto phase_barrier = [&]() {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave's LDS reads are done; a DMA just issued stays in flight
      gdrf_raw_barrier();
    };
    // Chunk t is multiplied by group 0 in phase 2t and by group 1 in phase 2t+1, both from B buffer t & 1 and their own A
    // image (whose fragments then stay in registers for the K topic reps).  DMAs are issued in a group's idle phase, land
    // during its next multiply phase, are retired by the vmcnt(0) that ends it, and are first read a barrier later:
    //   group 1, phase 2u   : B chunk u+1 -> buffer (u+1)&1 (last read in phase 2u-1); its own A if chunk u+1 opens a block
    //   group 0, phase 2u+1 : its own A if chunk u+2 opens a block (needed in phase 2u+4; image last read >= 2 phases ago, K >= 2)
    dma_a(0);
    if (gp == 1) dma_b(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    phase_barrier();
    for (int ph = 0; ph < 2 * nchunks; ++ph) {
      const int t = ph >> 1;
      if ((ph & 1) == gp) {
        mult(t);
        phase_barrier();
      } else if (gp == 0) {
        const int c = t + 2;
        if (c < nchunks && c % K == 0) dma_a(c / K);
        phase_barrier();
      } else {
        const int c = t + 1;
        dma_b(c);
        if (c < nchunks && c % K == 0) dma_a(c / K);
        phase_barrier();
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  wbar_rank_k(acc, g, m0, n0, L);
  const float wmax = wbar_store_transposed(acc, smem, gp, L, g, m0, n0);   // Wbar = acc - 2 asum W
  if (g.wbar_max) wave_max_publish(g.wbar_max, wmax);
}

// bwd_wbar with BOTH wave groups multiplying in every phase (see fwd_t_split_cc_kernel): one phase = one (reduction block q,
// topic rep) chunk for all 8 waves; the next chunk's B image (shared, double-buffered) and - when the next chunk opens a new
// reduction block - the groups' next A images (double-buffered) are requested by asm LDS-DMA at the top of the phase and retired
// by the vmcnt(0) in front of the barrier that ends it.
template <class SP>
__global__ __launch_bounds__(512, 2) void bwd_wbar_split_cc_kernel(BwdWbarSplitArgs<SP> g) {
  using CF = SplitCfg<SP>;
  using E = typename SP::E;
  using V8 = typename SP::V8;
  constexpr int NP = SP::NP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int gp = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
  constexpr int IMG = CF::IMG;
  const size_t tab = ((size_t)g.K * GDRF_TILE * sizeof(float) + 15) & ~(size_t)15;
  E* As = reinterpret_cast<E*>(smem) + gp * 2 * IMG;                     // [2 buffers][NP][128][LDH] of this group
  E* Bs = reinterpret_cast<E*>(smem) + 4 * IMG;                          // [2 buffers][NP][128][LDH] shared
  float* scaleS = reinterpret_cast<float*>(smem + (size_t)6 * IMG * 2 + (size_t)gp * tab);  // [K][128]  2 vbar_kn / (sW sB_k)

  const SplitLane L;
  const int nct = (g.Mp + GDRF_TILE - 1) / GDRF_TILE;
  int64_t rtile; int ct;
  nt_xcd_map_paired(blockIdx.x, nct, gp, rtile, ct);
  const int64_t m0 = rtile * GDRF_TILE;
  const int n0 = ct * GDRF_TILE;
  const int K = g.K, Mp = g.Mp;
  wbar_fill_scales(g, scaleS, m0, L.tid);
  f32x4 acc[4][4];
  split_zero(acc);
  V8 fa[4][NP];
  const int frag = L.frag(), drow = L.drow(), dq = L.dq(), wave_u = L.wave_u();
  const unsigned a_lds = lds_addr(As), b_lds = lds_addr(Bs);
  const int nk = Mp / CF::BK, nchunks = nk * K;
  // One LDS-DMA instruction costs its wave ~190 cycles of issue here (s_memtime: 380 cycles for two, in front of the MFMAs, with the
  // other wave of the SIMD not yet multiplying either): the requests of a phase are therefore issued one at a time BETWEEN the
  // MFMA groups of the phase, where the stall of the issuing wave is covered by MFMAs already in the pipe and by its partner's.
  const int b_rbk = wave_u + 4 * gp, b_row = b_rbk * 16 + drow;
  const int b_col = (n0 + b_row < Mp) ? n0 + b_row : 0;
  auto dma_b1 = [&](int c, int p) {       // piece p of B chunk c -> buffer c & 1: this wave (of 8) moves one 16-row block
    const int q = c / K, rep = c - q * K;
    glds16_asm(g.Bh + p * g.piece_stride + (((int64_t)rep * (Mp >> 5) + q) * Mp + b_col) * 32 + dq,
               b_lds + (unsigned)((((c & 1) * NP + p) * CF::PIECE + b_rbk * 512) * 2));
  };
  auto dma_a1 = [&](int q, int i, int p) { // piece p, row block wave + 4 i of this group's A image of reduction block q -> buffer q & 1
    const int rbk = wave_u + 4 * i;
    int64_t row = m0 + rbk * 16 + drow;
    row = row < g.nrows ? row : 0;
    glds16_asm(g.Wh + p * g.w_stride + row * Mp + q * CF::BK + dq, a_lds + (unsigned)((((q & 1) * NP + p) * CF::PIECE + rbk * 512) * 2));
  };
#pragma unroll
  for (int p = 0; p < NP; ++p) { dma_a1(0, 0, p); dma_a1(0, 1, p); dma_b1(0, p); }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();                        // also publishes the scale table
  for (int c = 0; c < nchunks; ++c) {
    const int q = c / K, rep = c - q * K;
    const bool more = c + 1 < nchunks, more_a = more && rep == K - 1;
    const E* Ab = As + (q & 1) * IMG;
    const E* Bb = Bs + (c & 1) * IMG;
    if (rep == 0) {                       // the A fragments serve all K topic reps of the block
#pragma unroll
      for (int a = 0; a < 4; ++a) split_frags<SP>(fa[a], Ab, L.wr * 64 + a * 16, frag);
    }
    f32x4 s4[4];
    split_row_scales(s4, scaleS + rep * GDRF_TILE, L);
    V8 fbq[2][NP];                        // the next column group's fragments are read while this one multiplies
    split_frags<SP>(fbq[0], Bb, L.wc * 64, frag);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      if (b + 1 < 4) split_frags<SP>(fbq[(b + 1) & 1], Bb, L.wc * 64 + (b + 1) * 16, frag);
      f32x4 P[4];
      split_products<SP, true>(P, fa, fbq[b & 1]);
      // the next chunk's requests, behind this column group's MFMAs: B (buffer (c + 1) & 1, last read one phase ago) after groups
      // 0 .. NP - 1; when the next chunk opens a reduction block, the group's next A image (last read K phases ago) after them
      if (more && b < NP) dma_b1(c + 1, b);
      if (more_a) {
        if (NP == 2) { dma_a1(q + 1, b >> 1, b & 1); }
        else if (b < 3) { dma_a1(q + 1, 0, b); dma_a1(q + 1, 1, b); }
      }
      split_scaled_acc(acc, b, s4, P);
    }
    split_phase_end();
  }
  wbar_rank_k(acc, g, m0, n0, L);
  const float wmax = wbar_store_transposed(acc, smem, gp, L, g, m0, n0);   // Wbar = acc - 2 asum W
  if (g.wbar_max) wave_max_publish(g.wbar_max, wmax);
}


// bwd_wbar, concurrent form, 64 reduction indices per phase (f16x3 only).  Stamps of the 32-deep form: a phase is ~2650 cycles for
// 2 x 768 cycles of MFMA per SIMD; what fills it is ISSUE - per wave 48 MFMAs (8 issue cycles each) plus ~100 vector instructions of
// which 64 are the acc += s P update that the per-(topic, row) factor forces after every chunk - not the matrix pipe.  Two 32-deep
// k-steps per (reduction block, topic) halve that update per MFMA: 96 MFMAs, one update, one barrier per phase.  LDS: the A image
// (this group's rows x 64 k, 32 KB) is SINGLE-buffered - its fragments live in registers for the K topic phases of a block, so the
// next block's image is requested in the phase after they were read (K >= 2) -; B (shared, 32 KB) is double-buffered.
__global__ __launch_bounds__(512, 2) void bwd_wbar_f16_k64_kernel(BwdWbarSplitArgs<SplitF16> g) {
  using SP = SplitF16;
  using CF = SplitCfg<SP>;
  using E = typename SP::E;
  using V8 = typename SP::V8;
  constexpr int NP = SP::NP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int gp = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
  constexpr int IMG = CF::IMG;                                            // one 32-deep image: [NP][128][32]
  const size_t tab = ((size_t)g.K * GDRF_TILE * sizeof(float) + 15) & ~(size_t)15;
  E* As = reinterpret_cast<E*>(smem) + gp * 2 * IMG;                     // [2 k-steps][NP][128][32] of this group
  E* Bs = reinterpret_cast<E*>(smem) + 4 * IMG;                          // [2 buffers][2 k-steps][NP][128][32] shared
  float* scaleS = reinterpret_cast<float*>(smem + (size_t)8 * IMG * 2 + (size_t)gp * tab);

  const SplitLane L;
  const int nct = (g.Mp + GDRF_TILE - 1) / GDRF_TILE;
  int64_t rtile; int ct;
  nt_xcd_map_paired(blockIdx.x, nct, gp, rtile, ct);
  const int64_t m0 = rtile * GDRF_TILE;
  const int n0 = ct * GDRF_TILE;
  const int K = g.K, Mp = g.Mp;
  wbar_fill_scales(g, scaleS, m0, L.tid);
  f32x4 acc[4][4];
  split_zero(acc);
  V8 fa[2][4][NP];
  const int frag = L.frag(), drow = L.drow(), dq = L.dq(), wave_u = L.wave_u();
  const unsigned a_lds = lds_addr(As), b_lds = lds_addr(Bs);
  const int nk = Mp / 64;                                               // Mp % 64 == 0 (checked by the host)
  // this workgroup's reduction blocks [q_lo, q_hi): all of them, or slice blockIdx.y of nslice
  const int q_lo = (int)(((int64_t)nk * blockIdx.y) / g.nslice), q_hi = (int)(((int64_t)nk * (blockIdx.y + 1)) / g.nslice);
  const int c_lo = q_lo * K, nchunks = q_hi * K;
  const bool first_slice = blockIdx.y == 0;
  float* const out_base = g.nslice > 1 ? g.slab + (int64_t)blockIdx.y * g.slab_stride : g.Wbar;
  const int b_rbk = wave_u + 4 * gp, b_row = b_rbk * 16 + drow;
  const int b_col = (n0 + b_row < Mp) ? n0 + b_row : 0;
  // B chunk c = (block q, topic rep), k-step ks, piece p -> buffer c & 1: this wave (of 8) moves one 16-row block
  auto dma_b1 = [&](int c, int ks, int p) {
    const int q = c / K, rep = c - q * K;
    glds16_asm(g.Bh + p * g.piece_stride + (((int64_t)rep * (Mp >> 5) + 2 * q + ks) * Mp + b_col) * 32 + dq,
               b_lds + (unsigned)(((((c & 1) * 2 + ks) * NP + p) * CF::PIECE + b_rbk * 512) * 2));
  };
  // this group's A image of block q: k-step ks, piece p, row block wave + 4 i
  auto dma_a1 = [&](int q, int ks, int i, int p) {
    const int rbk = wave_u + 4 * i;
    int64_t row = m0 + rbk * 16 + drow;
    row = row < g.nrows ? row : 0;
    glds16_asm(g.Wh + p * g.w_stride + row * Mp + q * 64 + ks * 32 + dq, a_lds + (unsigned)(((ks * NP + p) * CF::PIECE + rbk * 512) * 2));
  };
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int p = 0; p < NP; ++p) { dma_a1(q_lo, ks, 0, p); dma_a1(q_lo, ks, 1, p); dma_b1(c_lo, ks, p); }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();                        // also publishes the scale table
  for (int c = c_lo; c < nchunks; ++c) {
    const int q = c / K, rep = c - q * K;
    const bool more = c + 1 < nchunks, more_a = rep == 1 && q + 1 < q_hi;   // A(q + 1) into the image whose fragments were read one phase ago
    const E* Bb = Bs + (c & 1) * 2 * IMG;
    if (rep == 0) {                       // the A fragments serve all K topic reps of the block
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int a = 0; a < 4; ++a) split_frags<SP>(fa[ks][a], As + ks * IMG, L.wr * 64 + a * 16, frag);
    }
    f32x4 s4[4];
    split_row_scales(s4, scaleS + rep * GDRF_TILE, L);
    V8 fbq[2][2][NP];                     // the next column group's fragments are read while this one multiplies
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) split_frags<SP>(fbq[0][ks], Bb + ks * IMG, L.wc * 64, frag);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      if (b + 1 < 4) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) split_frags<SP>(fbq[(b + 1) & 1][ks], Bb + ks * IMG, L.wc * 64 + (b + 1) * 16, frag);
      }
      f32x4 P[4];
      split_products<SP, true>(P, fa[0], fbq[b & 1][0]);      // the two 32-deep k-steps, the second on top of the first
      split_products<SP, false>(P, fa[1], fbq[b & 1][1]);
      // the next chunk's requests behind the first two column groups' MFMAs, so that they have the second half of the phase to land: an
      // LDS-DMA instruction stalls its wave at issue, but spread over all four groups (one or two each) the last request was issued just
      // in front of the phase's closing vmcnt(0) and its whole latency showed - 13.3 -> 12.1 ms.  (Also measured: the two wave groups
      // staggered - group 0 behind b = 0, 1, group 1 behind b = 2, 3: 13.7 ms.)
      if (b < 2) {
        if (more) { dma_b1(c + 1, b, 0); dma_b1(c + 1, b, 1); }
        if (more_a) { dma_a1(q + 1, b, 0, 0); dma_a1(q + 1, b, 1, 0); dma_a1(q + 1, b, 0, 1); dma_a1(q + 1, b, 1, 1); }
      }
      split_scaled_acc(acc, b, s4, P);
    }
    split_phase_end();
  }
  // ---- epilogue.  One workgroup per CU: nothing else runs on the CU while it reads and writes, so every global load it needs is issued up
  // front, from clamped addresses and unconditionally (the fragment registers of the loop are free now) - the W tile of both 32-row halves,
  // asum, and the locbar / U values of the rank-K term - and their latencies overlap instead of following one another: five dependent round
  // trips to HBM per workgroup were 0.9 ms of the 12.3 (measured without the epilogue: 11.4).
  f32x4 wv[2][8];
  float as2v[2][8];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int64_t m = m0 + wbar_seg_row(L, h, i);           // the row segment this lane moves in round i of half h of the store
      const int n = n0 + wbar_seg_col(L);
      const int64_t mc = m < g.nrows ? m : 0;
      const int nc = n < Mp ? n : 0;
      wv[h][i] = *reinterpret_cast<const f32x4*>(g.W + mc * Mp + nc);
      as2v[h][i] = first_slice ? 2.0f * g.asum[mc] : 0.0f;
    }
  // rank-K term as wbar_rank_k, but 16 topics per batch of loads, from clamped addresses
  const int wr = L.wr, wc = L.wc, lr = L.lr, lg = L.lg;
  for (int kb = 0; kb < (first_slice ? K : 0); kb += 16) {
    float av[4][4], bv[4][4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int k = kb + 4 * it + lg, kc = k < K ? k : 0;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int64_t row = m0 + wr * 64 + a * 16 + lr;
        const float v = g.locbar[(int64_t)kc * g.ldk + (row < g.nrows ? row : 0)];
        av[it][a] = (k < K && row < g.nrows) ? v : 0.0f;
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int col = n0 + wc * 64 + b * 16 + lr;
        const float v = g.U[(int64_t)kc * g.M + (col < g.M ? col : 0)];
        bv[it][b] = (k < K && col < g.M) ? v : 0.0f;
      }
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      if (kb + 4 * it < K) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[it][a], bv[it][b], acc[a][b], 0, 0, 0);
      }
    }
  }
  // out = acc - 2 asum W as wbar_store_transposed, from the registers loaded above
  __syncthreads();                                           // every wave is done with the operand images
  float wmax = 0.0f;
  float* tile = wbar_tile(smem, gp, L);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    wbar_tile_put(tile, acc, h, L);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      // = m0 + wbar_seg_row, n0 + wbar_seg_col in this kernel's tuned order (scratch)
      const int64_t m = m0 + L.wr * 64 + h * 32 + ((L.lane >> 4) + 4 * i);
      const int n = n0 + L.wc * 64 + (L.lane & 15) * 4;
      const f32x4 t = wbar_tile_get(tile, i, L);
      if (m < g.nrows && n < Mp) wbar_seg_store(out_base + m * Mp + n, t, as2v[h][i], wv[h][i], wmax);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // reads done before the tile is overwritten with the other half
  }
  if (g.wbar_max && g.nslice == 1) wave_max_publish(g.wbar_max, wmax);   // sliced: wbar_slab_sum_kernel publishes the maximum of the sum
}


// bwd_wbar, ONE WAVE PER SIMD, B_k fed from L2 to registers (f16x3 only; unsliced reductions, 2 <= K <= 16, Mp % 64 == 0).
//
// What bwd_wbar_f16_k64_kernel spends beside its MFMAs (profiles/r03/README.md item 3) is almost all B_k: four of a wave's ~4.8 LDS-DMA
// requests per phase, the B fragment reads out of the shared image, and the vmcnt(0) + barrier over 8 waves that every phase ends in because
// B_k goes through that image.  Bh is stored k-blocked ([piece][topic][k / 32][column][32]) and the MFMA operand lane is (lr = column, lg =
// k quad) in natural k order, so a 16-column x 32-k fragment is 1 024 contiguous bytes and ONE global_load_dwordx4 per wave delivers it
// finished from the XCD's L2 (where the block map keeps the column tile's panels) - no M0, no LDS image, no ds_read, no barrier.  That needs
// registers k64 (256 VGPRs at two waves per SIMD) does not have.  Here four waves, one per SIMD, share the same 256 x 128 workgroup tile:
// wave w owns the 128 rows of row tile w >> 1 and the 64 columns of half w & 1.  Per lane:
//   VGPR  acc 128, P of one 16-column group 32, the topic's row factors 32, addresses
//   AGPR  a[0:127]    W fragments of the current 64-deep block: [k-step][row group 0-7][piece]
//         a[128:255]  B_k fragment ring: [phase parity][k-step][column group 0-3][piece]
// MFMA A/B operands, ds_read and global-load destinations may be AGPRs on gfx950; VALU cannot address them, which is why the accumulators
// stay in VGPRs.  The AGPRs are named literally in the asm (the compiler never sees them; every statement that writes them lists all 256
// as clobbers, which also makes the kernel descriptor allocate them), the MFMAs are issued from asm with C/D in VGPRs.
// THIS IS A CONTRACT HIPCC DOES NOT KNOW ABOUT: the MFMA statements read a[0:255] without declaring them, so the kernel is right only while
// the compiler puts nothing of its own into an AGPR between the prologue's barrier and the end of the loop - no spill, no copy - with the
// VGPRs at exactly 256.  It holds for all three instantiations today.  After ANY edit of this kernel, and after a compiler change, repeat
// the check: `hipcc -save-temps`, then in each instantiation's assembly no `v_accvgpr_*` and no `scratch_*` between the first `s_barrier`
// and the `s_waitcnt vmcnt(0)` that follows the loop (hipcc may and does use the AGPRs as spill space in the epilogue, where they are dead),
// and `make resources`: ScratchSize 0.  tests/test_gpu_wbar_w1.py runs every instantiation (K = 10, 9, 16: <2>; K = 5: <4>; K = 2, 3: <8>).
//
// Schedule.  A phase = (reduction block q, topic rep) = 4 column groups x 48 MFMAs.  P of a group is written product-major, (k-step, product,
// row group): per accumulator the same six products in the same order as k64.  `acc += s P` of group b sits in front of the first eight
// MFMAs of group b + 1 (of the next phase for b = 3), one row group each: P[a] was finished seven MFMAs earlier and is overwritten by the MFMA
// that follows its update.  Behind group 0's MFMAs: the phase's row factors, R requests of the NEXT block's W image (LDS-DMA, double-buffered
// now that B_k needs no LDS: 16 requests per wave and block, R = 2 / 4 / 8 per phase so that K >= 8 / 4 / 2 phases carry them all) and the 16
// B loads of the NEXT phase into the other half of the ring.  The counts are the same in every phase (the last phase re-requests itself, a
// finished block re-requests itself into the idle buffer), so every wait is a literal vmcnt(n): in front of group b, the 4 (3 - b) later
// loads of this phase's B and - for b > 0 - the R + 16 requests issued behind group 0 may still be in flight.  One workgroup barrier per
// reduction block publishes the W image; phases are barrier-free.  The loop body is two phases (the ring halves are register names); an odd
// phase count runs one more phase with all-zero row factors.
#define GDRF_A10(p) "a" p "0", "a" p "1", "a" p "2", "a" p "3", "a" p "4", "a" p "5", "a" p "6", "a" p "7", "a" p "8", "a" p "9"
#define GDRF_A100(p) GDRF_A10(p "0"), GDRF_A10(p "1"), GDRF_A10(p "2"), GDRF_A10(p "3"), GDRF_A10(p "4"), GDRF_A10(p "5"), GDRF_A10(p "6"), \
                     GDRF_A10(p "7"), GDRF_A10(p "8"), GDRF_A10(p "9")
#define GDRF_ALL_AGPRS "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", GDRF_A10("1"), GDRF_A10("2"), GDRF_A10("3"), GDRF_A10("4"), \
                       GDRF_A10("5"), GDRF_A10("6"), GDRF_A10("7"), GDRF_A10("8"), GDRF_A10("9"), GDRF_A100("1"), GDRF_A10("20"), GDRF_A10("21"), \
                       GDRF_A10("22"), GDRF_A10("23"), GDRF_A10("24"), "a250", "a251", "a252", "a253", "a254", "a255"
constexpr int wb1_wreg(int ks, int a, int p) { return ((ks * 8 + a) * 2 + p) * 4; }
constexpr int wb1_breg(int h, int ks, int b, int p) { return 128 + (((h * 2 + ks) * 4 + b) * 2 + p) * 4; }
// P = (or +=) W fragment a[WA:WA+3] x B fragment a[BA:BA+3]
template <int WA, int BA, bool ZERO> __device__ __forceinline__ void wb1_mfma(f32x4& P) {
  if constexpr (ZERO) asm volatile("v_mfma_f32_16x16x32_f16 %0, a[%c1:%c2], a[%c3:%c4], 0" : "=v"(P) : "i"(WA), "i"(WA + 3), "i"(BA), "i"(BA + 3));
  else asm volatile("v_mfma_f32_16x16x32_f16 %0, a[%c1:%c2], a[%c3:%c4], %0" : "+v"(P) : "i"(WA), "i"(WA + 3), "i"(BA), "i"(BA + 3));
}
// a[REG:REG+3] = the lane's 16 bytes at sbase (wave-uniform) + voff + OFF.  Not counted by hipcc: the caller waits by vmcnt(n).
template <int REG, int OFF> __device__ __forceinline__ void wb1_gload(const void* sbase, unsigned voff) {
  asm volatile("global_load_dwordx4 a[%c2:%c3], %0, %1 offset:%c4" : : "v"(voff), "s"(sbase), "i"(REG), "i"(REG + 3), "i"(OFF) : "memory", GDRF_ALL_AGPRS);
}
template <int REG, int OFF> __device__ __forceinline__ void wb1_ldsread(unsigned addr) {
  asm volatile("ds_read_b128 a[%c1:%c2], %0 offset:%c3" : : "v"(addr), "i"(REG), "i"(REG + 3), "i"(OFF) : "memory", GDRF_ALL_AGPRS);
}
// c0, c1 += rows R0, R0 + 1 of s P, as two single v_fmac_f32 that stay where they are written
template <int R0> __device__ __forceinline__ void wb1_update2(float& c0, float& c1, const f32x4& s, const f32x4& p) {
  asm volatile("v_fmac_f32 %0, %1, %2" : "+v"(c0) : "v"(s[R0]), "v"(p[R0]));
  asm volatile("v_fmac_f32 %0, %1, %2" : "+v"(c1) : "v"(s[R0 + 1]), "v"(p[R0 + 1]));
}
template <int N> __device__ __forceinline__ void wb1_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" : : "n"(N) : "memory"); }

// The W side of the one-wave-per-SIMD kernels (bwd_wbar_f16_w1_kernel, fwd_t_f16_w1_kernel): NW = 2 or 4 waves stage and read the image of one
// 128-row tile's 64-deep reduction block - [2 k-steps][2 pieces][128][32] halfwords, swizzled (SplitLane), 32 LDS-DMA requests of 16 rows -,
// wave wsub of them the row blocks wsub + NW i, i < 8 / NW.  Buffer buf of the double-buffered image lies buf * buf_stride bytes behind w_lds.
// Request r = 0 .. 32 / NW - 1 of a wave for block q: (k-step, piece, i) = r in mixed radix (2, 2, 8 / NW).  A wave-uniform base (the tile's
// first row, or row 0 for a tile wholly past the end) + one 32-bit lane offset per row block, the lane's row clamped to the last one (clamped
// rows are never stored).  A caller that spreads its requests over its phases R at a time issues r = rep_c R + j, j < R: j is a literal, so the
// row block is one too (R a multiple of 8 / NW) or one of two (NW = 2, R = 2).  s_nop 4: the base may come straight from v_readfirstlane.
constexpr int W1_WIMG = 4 * SplitCfg<SplitF16>::PIECE * 2;              // bytes of one row tile's image
template <int NW> struct W1Image {
  static_assert(NW == 2 || NW == 4, "row blocks per wave: 4 or 2");
  static constexpr int PER = 8 / NW;
  const _Float16* w_row; int64_t w_stride;
  unsigned w_lds, buf_stride;
  int wsub;
  unsigned vw0, vw1, vw2, vw3;
  __device__ __forceinline__ W1Image(const _Float16* Wh, int64_t w_stride_, int64_t nrows, int Mp, int64_t m0, unsigned w_lds_, unsigned buf_stride_, int wsub_,
                                     const SplitLane& L)
      : w_stride(w_stride_), w_lds(w_lds_), buf_stride(buf_stride_), wsub(wsub_) {
    const int drow = L.drow(), dq = L.dq();
    const int64_t mbase = m0 < nrows ? m0 : 0;
    auto w_off = [&](int i) {
      const int64_t rel = (wsub + NW * i) * 16 + drow, last = nrows - 1 - mbase;
      unsigned v = (unsigned)(((int)(rel < last ? rel : last) * Mp + dq) * 2);
      asm volatile("" : "+v"(v));             // single registers, not an array hipcc may index in memory
      return v;
    };
    vw0 = w_off(0); vw1 = w_off(1);
    if constexpr (NW == 2) { vw2 = w_off(2); vw3 = w_off(3); } else { vw2 = 0; vw3 = 0; }
    w_row = Wh + mbase * Mp;
  }
  template <int R, int J> __device__ __forceinline__ void request(int q, int buf, int rep_c) const {
    static_assert(NW == 2 || R % 2 == 0, "the row block must follow from J");
    const int r = rep_c * R + J, ks = r / (2 * PER), p = (r / PER) & 1;
    const unsigned va = (J & 1) ? vw1 : vw0, vb = (J & 1) ? vw3 : vw2;
    const unsigned vo = NW == 4 ? va : (R >= 4 ? ((J & 2) ? vb : va) : ((rep_c & 1) ? vb : va));
    const int rbk = wsub + NW * (r & (PER - 1));
    const _Float16* src = w_row + (p ? w_stride : 0) + q * 64 + ks * 32;
    const unsigned dst = w_lds + (unsigned)buf * buf_stride + (unsigned)((ks * 2 + p) * SplitCfg<SplitF16>::PIECE * 2 + rbk * 1024);
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 4\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(vo), "s"(src), "s"(dst) : "memory");
  }
};

template <int R>
__global__ __launch_bounds__(256, 1) void bwd_wbar_f16_w1_kernel(BwdWbarSplitArgs<SplitF16> g) {
  using SP = SplitF16;
  using CF = SplitCfg<SP>;
  using E = typename SP::E;
  static_assert(R == 2 || R == 4 || R == 8, "16 requests per block in K >= 16 / R phases");
  constexpr int PIECE = CF::PIECE;
  constexpr int WIMG = 4 * PIECE * 2;                                    // bytes of one group's W image: [2 k-steps][2 pieces][128][32] halfwords
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // LDS: W images [2 buffers][2 row tiles] (128 KB), then the row-factor tables [2 row tiles][K + 1][128] (row K: zeros)
  SplitLane L;
  const int w = L.wave_u(), gp = w >> 1, wc = w & 1;
  L.wc = wc;
  const int K = g.K, Mp = g.Mp;
  const int tabf = (K + 1) * GDRF_TILE;
  float* const tab0 = reinterpret_cast<float*>(smem + 4 * WIMG);
  const int nct = (Mp + GDRF_TILE - 1) / GDRF_TILE;
  int64_t rtile; int ct;
  nt_xcd_map_paired(blockIdx.x, nct, gp, rtile, ct);
  const int64_t m0 = rtile * GDRF_TILE;
  const int n0 = ct * GDRF_TILE;
  wbar_fill_scales(g, tab0, (rtile - gp) * GDRF_TILE, L.tid);
  wbar_fill_scales(g, tab0 + tabf, (rtile - gp + 1) * GDRF_TILE, L.tid);
  tab0[(L.tid >> 7) * tabf + K * GDRF_TILE + (L.tid & 127)] = 0.0f;
  const float* const tab = tab0 + gp * tabf;

  const int nk = Mp / 64, nph = nk * K;
  const int lr = L.lr, lg = L.lg;
  const unsigned w_lds = lds_addr(smem) + (unsigned)(gp * WIMG);       // this row tile's image, buffer 0; buffer 1 is 2 WIMG further
  const unsigned frag_addr = w_lds + (unsigned)(L.frag() * 2);
  // The W image's requests (W1Image): in phase rep the wave issues r = min(rep, 16 / R - 1) R + j, j < R (phases past 16 / R repeat the last
  // ones).  Clamped rows have factor 0.
  const W1Image<2> WI(g.Wh, g.w_stride, g.nrows, Mp, m0, w_lds, 2 * WIMG, wc, L);
  auto dma_w = [&](int q, int buf, int rep_c, auto jc) { WI.template request<R, decltype(jc)::value>(q, buf, rep_c); };
  // B fragments of phase (q, rep): a wave-uniform base per (k-step, piece), one lane offset, the column group in the immediate offset
  const int col0 = (n0 + wc * 64 < Mp) ? n0 + wc * 64 : 0;            // Mp % 64 == 0: a wave's 64 columns are inside or past the end together
  const unsigned voff_b = (unsigned)((lr * 32 + 8 * lg) * 2);
  const int64_t b_ks = (int64_t)Mp * 32, b_rep = (int64_t)(Mp >> 5) * b_ks;   // elements per 32-deep k block and per topic
  const E* sb[2][2];
  auto b_bases = [&](const E* b0) {
    sb[0][0] = b0; sb[1][0] = b0 + b_ks; sb[0][1] = b0 + g.piece_stride; sb[1][1] = b0 + b_ks + g.piece_stride;
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("" : "+s"(sb[i >> 1][i & 1]));   // they exist here, far ahead of the loads that read them
  };
  const E* b_blk = g.Bh + (int64_t)col0 * 32;   // k-step 0, piece 0 of (block q, topic 0) and of the current phase
  const E* b_cur = b_blk;

  // the accumulators as single registers (row group, column group, row 4 lg + r): the updates below are single v_fmac_f32 - beside MFMAs a
  // packed-f32 instruction costs more than the two it replaces -, and nothing in the loop needs them as tuples
  float acc[8][4][4];
  f32x4 P[8], s8[8];
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    P[a] = f32x4{0, 0, 0, 0}; s8[a] = f32x4{0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.0f;
  }
  // prologue: the first block's W image, the first phase's B fragments
  for (int rp = 0; rp < 16 / R; ++rp) static_for<R>([&](auto jc) { dma_w(0, 0, rp, jc); });
  b_bases(b_cur);
  static_for<16>([&](auto jc) {
    constexpr int j = decltype(jc)::value, bb = j >> 2, ks = (j >> 1) & 1, p = j & 1;
    wb1_gload<wb1_breg(0, ks, bb, p), bb * 1024>(sb[ks][p], voff_b);
  });
  wb1_vmcnt<0>();
  __syncthreads();                            // also publishes the factor tables

  // Where things sit in a phase (gap m = behind MFMA m of a column group; an MFMA holds the issue port for 8 of its 16 cycles, so a gap
  // hides two 4-cycle instructions or one dearer one):
  //   MFMAs      two halves of 24, row groups 0 - 3 then 4 - 7, each (k-step, product, row group); P[a] starts from 0 in its first
  //   updates    gaps 4 - 11 of a half, two v_fmac each: in the first half the row groups 4 - 7 of the column group BEFORE (finished 8 MFMAs
  //              earlier, overwritten from gap 24 on), in the second half the row groups 0 - 3 of this one
  //   factors    group 0: rows of the row groups 0 - 3 in gaps 0 - 3, of 4 - 7 in gaps 13 - 19 (behind the last update with the old ones)
  //   B loads    of the next phase: 8 in group 0, 8 in group 1, gaps 12, 14 .. 26
  //   W requests R / 2 in group 0 and R / 2 in group 2, gaps 38, 40 ..: far apart - a request waits for M0 until the one before has read it
  constexpr int N1 = R / 2, N2 = R / 2;
  int c = 0, q = 0, rep = 0;
  for (int it = 0; it < (nph + 1) / 2; ++it) {
    static_for<2>([&](auto hc) {
      constexpr int h = decltype(hc)::value;  // phase c multiplies ring half h and fills half 1 - h
      const bool live = c < nph;
      const int qq = q < nk ? q : nk - 1;
      if (live && rep == 0) {                 // a new reduction block: its W image is complete and every wave is done with the one before
        if (c > 0) { wb1_vmcnt<0>(); gdrf_raw_barrier(); }
        const unsigned fa = frag_addr + (unsigned)((qq & 1) * 2 * WIMG);
        static_for<32>([&](auto fc) {
          constexpr int f = decltype(fc)::value, ks = f >> 4, p = (f >> 3) & 1, a = f & 7;
          wb1_ldsread<wb1_wreg(ks, a, p), ((ks * 2 + p) * PIECE + a * 16 * 32) * 2>(fa);
        });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      const unsigned saddr = lds_addr(tab + (live ? rep : K) * GDRF_TILE + lg * 4);
      // the next phase (the last one re-requests itself) and the next block (likewise)
      const E* const b_next = c + 1 >= nph ? b_cur : (rep + 1 == K ? b_blk + 2 * b_ks : b_cur + b_rep);
      b_bases(b_next);
      const int qn = qq + 1 < nk ? qq + 1 : nk - 1, bufn = (qq + 1) & 1;
      const int rep_c = (live && rep < 16 / R) ? rep : 16 / R - 1;
      static_for<4>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        // in flight behind the four loads this group needs (issued one phase ago): the later loads of that phase, its requests, and what
        // this phase has issued so far
        wb1_vmcnt<b == 0 ? 12 + N1 + N2 : (b == 1 ? 16 + 2 * N1 + N2 : (b == 2 ? 20 + N1 + N2 : 16 + N1 + 2 * N2))>();
        static_for<48>([&](auto mc) {
          constexpr int m = decltype(mc)::value, half = m / 24, mm = m % 24, ks = mm / 12, t = (mm >> 2) % 3, a = half * 4 + (mm & 3);
          wb1_mfma<wb1_wreg(ks, a, SP::pa(t)), wb1_breg(h, ks, b, SP::pb(t)), mm < 4>(P[a]);
          if constexpr (mm >= 4 && mm < 12) {
            constexpr int i = mm - 4, au = (half == 0 ? 4 : 0) + (i >> 1), bu = half == 0 ? (b + 3) & 3 : b;
            wb1_update2<2 * (i & 1)>(acc[au][bu][2 * (i & 1)], acc[au][bu][2 * (i & 1) + 1], s8[au], P[au]);
          }
          if constexpr (b == 0) {             // this phase's row factors (asm reads: hipcc neither counts nor moves them; waited for in gap 27)
            if constexpr (m < 4) asm volatile("ds_read_b128 %0, %1 offset:%c2" : "=v"(s8[m]) : "v"(saddr), "i"(m * 64) : "memory");
            if constexpr (m >= 13 && m < 20 && (m & 1)) asm volatile("ds_read_b128 %0, %1 offset:%c2" : "=v"(s8[4 + (m - 13) / 2]) : "v"(saddr), "i"((4 + (m - 13) / 2) * 64) : "memory");
            if constexpr (m == 27) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(s8[0]), "+v"(s8[1]), "+v"(s8[2]), "+v"(s8[3]), "+v"(s8[4]), "+v"(s8[5]), "+v"(s8[6]), "+v"(s8[7]) : : "memory");
          }
          if constexpr (b < 2 && m >= 12 && m < 28 && (m & 1) == 0) {
            constexpr int j = 8 * b + (m - 12) / 2, bb = j >> 2, ks2 = (j >> 1) & 1, p2 = j & 1;
            wb1_gload<wb1_breg(1 - h, ks2, bb, p2), bb * 1024>(sb[ks2][p2], voff_b);
          }
          if constexpr ((b == 0 || b == 2) && m >= 38 && m < 38 + 2 * N1 && (m & 1) == 0)
            dma_w(qn, bufn, rep_c, std::integral_constant<int, (b == 0 ? 0 : N1) + (m - 38) / 2>{});
        });
      });
      ++c;
      b_cur = b_next;
      if (++rep == K) { rep = 0; ++q; b_blk += 2 * b_ks; }
    });
  }
  wb1_vmcnt<0>();
  // the last column group's row groups 4 - 7: their MFMAs' results are not covered by following MFMAs
  asm volatile("s_nop 15\n\ts_nop 15" : "+v"(P[4]), "+v"(P[5]), "+v"(P[6]), "+v"(P[7]));
  static_for<8>([&](auto ic) {
    constexpr int i = decltype(ic)::value;
    wb1_update2<2 * (i & 1)>(acc[4 + (i >> 1)][3][2 * (i & 1)], acc[4 + (i >> 1)][3][2 * (i & 1) + 1], s8[4 + (i >> 1)], P[4 + (i >> 1)]);
  });
  f32x4 accv[2][4][4];                        // the epilogue takes them as the MFMA's tuples
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) accv[a >> 2][a & 3][b] = f32x4{acc[a][b][0], acc[a][b][1], acc[a][b][2], acc[a][b][3]};

  // the lane's place again, from the hardware lane counter: the values derived from threadIdx before the loop need not live through it
  L.lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  L.lr = L.lane & 15; L.lg = L.lane >> 4;
  // ---- epilogue, as k64's: the global loads up front from clamped addresses (the lower 64 rows' W tile behind the upper rows' first store),
  // the rank-K term on the f32 MFMA - from asm: in a kernel that may use more than 256 registers hipcc gives every builtin MFMA the AGPR form
  // and would shuttle the accumulators -, then out = acc - 2 asum W through the wave's transposition tile, 32 rows at a time.
  f32x4 wv[2][2][8];
  float as2v[2][2][8];
  auto load_w = [&](int hr) {
    L.wr = hr;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t m = m0 + wbar_seg_row(L, h, i);
        const int n = n0 + wbar_seg_col(L);
        wv[hr][h][i] = *reinterpret_cast<const f32x4*>(g.W + (m < g.nrows ? m : 0) * Mp + (n < Mp ? n : 0));
      }
  };
  load_w(0);
#pragma unroll
  for (int hr = 0; hr < 2; ++hr) {
    L.wr = hr;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t m = m0 + wbar_seg_row(L, h, i);
        as2v[hr][h][i] = 2.0f * g.asum[m < g.nrows ? m : 0];
      }
  }
  for (int kb = 0; kb < K; kb += 8) {
    float av[2][8], bv[2][4];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int k = kb + 4 * it + L.lg, kc = k < K ? k : 0;
#pragma unroll
      for (int a = 0; a < 8; ++a) {
        const int64_t row = m0 + a * 16 + L.lr;
        const float v = g.locbar[(int64_t)kc * g.ldk + (row < g.nrows ? row : 0)];
        av[it][a] = (k < K && row < g.nrows) ? v : 0.0f;
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int col = n0 + wc * 64 + b * 16 + L.lr;
        const float v = g.U[(int64_t)kc * g.M + (col < g.M ? col : 0)];
        bv[it][b] = (k < K && col < g.M) ? v : 0.0f;
      }
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      if (kb + 4 * it < K) {
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b)      // s_nop 1: av / bv / acc may come straight from compiler VALU code
            asm volatile("s_nop 1\n\tv_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(accv[a >> 2][a & 3][b]) : "v"(av[it][a]), "v"(bv[it][b]));
      }
    }
  }
#pragma unroll
  for (int hr = 0; hr < 2; ++hr)            // the rank-K MFMAs' results (inline asm: outside hipcc's hazard tables)
#pragma unroll
    for (int a = 0; a < 4; ++a)
      asm volatile("s_nop 15" : "+v"(accv[hr][a][0]), "+v"(accv[hr][a][1]), "+v"(accv[hr][a][2]), "+v"(accv[hr][a][3]));
  __syncthreads();                            // every wave is done with the W images, and every request into them has landed
  float wmax = 0.0f;
  L.wave = w;
  float* tile = wbar_tile(smem, 0, L);
#pragma unroll
  for (int hr = 0; hr < 2; ++hr) {
    L.wr = hr;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      wbar_tile_put(tile, accv[hr], h, L);
      if (hr == 0 && h == 1) { load_w(1); L.wr = 0; }         // the lower rows' W tile: requested while the upper rows' second half is stored
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t m = m0 + wbar_seg_row(L, h, i);
        const int n = n0 + wbar_seg_col(L);
        const f32x4 t = wbar_tile_get(tile, i, L);
        if (m < g.nrows && n < Mp) wbar_seg_store(g.Wbar + m * Mp + n, t, as2v[hr][h][i], wv[hr][h][i], wmax);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // reads done before the tile is overwritten with the next half
    }
  }
  if (g.wbar_max) wave_max_publish(g.wbar_max, wmax);
}

// Wbar = the sum of the slices' partial sums (fixed order), and its maximum for the block scale of the G^T operand
__global__ __launch_bounds__(256) void wbar_slab_sum_kernel(const float* __restrict__ slab, int64_t slab_stride, int nslice, int64_t n4 /*float4 count*/,
                                                           float* __restrict__ Wbar, unsigned* __restrict__ wbar_max) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  float wmax = 0.0f;
  if (i < n4) {
    f32x4 acc = *reinterpret_cast<const f32x4*>(slab + 4 * i);
    for (int sl = 1; sl < nslice; ++sl) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(slab + (int64_t)sl * slab_stride + 4 * i);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += t[e];
    }
    *reinterpret_cast<f32x4*>(Wbar + 4 * i) = acc;
#pragma unroll
    for (int e = 0; e < 4; ++e) wmax = fmaxf(wmax, fabsf(acc[e]));
  }
  if (wbar_max) wave_max_publish(wbar_max, wmax);
}

// ------------------------------------------------------------------------------------------------------------------
// tt[k][n] = || S_k^T w_n ||^2 on the same emulation: T_k = W S_k lives only in the accumulators; a row tile and topic walk
// the column tiles (triangular k range i >= j), as gemm_nt<FwdTProb> does.
template <class SP> struct FwdTSplitArgs {
  const typename SP::E* Wh; int64_t w_stride; int64_t nrows; int Mp, K;
  int KG; int rt8;                            // topics per group (see the block map), ceil(row-tile pairs / 8)
  const typename SP::E* STh; int64_t piece_stride;    // STh[p][k][i / 32][j][i % 32] = pieces of S_k[i][j] (k-blocked)
  float* tt; int64_t ldt;
  const float* sc;
  int k_lo = 0, k_n = 0;                      // fwd_t_f16_w1_kernel only: the topics [k_lo, k_lo + k_n) of this launch
};

// Block map of the tt kernels.  Grid: 8 * K * rt8 with rt8 = ceil(row-tile pairs / 8).  XCD = blockIdx & 7 owns the pairs r * 8 + xcd; topics
// go in groups of KG, group-major (every XCD first runs all its pairs for topics [0, KG), then [KG, 2 KG), ...) so that only KG topics'
// S^T pieces are live in its 4 MB L2 at a time; the KG workgroups of one pair are adjacent.  rt0: the pair's first row tile; bz: the topic.
template <class SP> __device__ __forceinline__ void fwd_t_map_block(const FwdTSplitArgs<SP>& g, int64_t& rt0, int& bz) {
  const unsigned xcd = blockIdx.x & 7u, idx = blockIdx.x >> 3;
  const unsigned per_group = (unsigned)g.KG * (unsigned)g.rt8;
  const int grp = (int)(idx / per_group);
  const unsigned rem = idx - (unsigned)grp * per_group;
  const int kg = min(g.KG, g.K - grp * g.KG);
  rt0 = 2 * ((int64_t)(rem / (unsigned)kg) * 8 + xcd);
  bz = grp * g.KG + (int)(rem % (unsigned)kg);
}
// Folding a finished column tile ct into the row sums of squares: a lane's column of 16-column group b counts if it lies inside Mp, and
// an accumulator entry then adds its square.  The two kernels sum these in different fixed orders (registers / per-wave LDS slots), so each keeps
// its loop.
__device__ __forceinline__ bool fwd_t_col_ok(int ct, int b, int Mp, const SplitLane& L) { return ct * GDRF_TILE + L.wc * 64 + b * 16 + L.lr < Mp; }
__device__ __forceinline__ float fwd_t_sq(float x, bool cok) { return cok ? x * x : 0.0f; }
// Lane 0 of every 16-lane row gets the row's sum (the other lanes get it in other orders of addition): four DPP rotations on the VALU instead of
// group16_sum's four trips through the LDS crossbar.  Fixed order, so deterministic.
__device__ __forceinline__ float row16_sum_lane0(float v) {
  auto rot = [](float x, auto nc) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x120 + decltype(nc)::value, 0xf, 0xf, false));   // row_ror:n
  };
  v += rot(v, std::integral_constant<int, 8>{});
  v += rot(v, std::integral_constant<int, 4>{});
  v += rot(v, std::integral_constant<int, 2>{});
  v += rot(v, std::integral_constant<int, 1>{});
  return v;
}
// tt of row m0 + tid (tid < 128) and topic bz from its sum of squares v; the block scales of W and S_k^T come off here
template <class SP> __device__ __forceinline__ void fwd_t_store_tt(const FwdTSplitArgs<SP>& g, int bz, int64_t m0, int tid, float v) {
  const int64_t m = m0 + tid;
  const SplitLay SL{g.K};
  const float un = g.sc[SL.w() + 1] * g.sc[SL.st(bz) + 1];
  if (m < g.nrows) g.tt[(int64_t)bz * g.ldt + m] = v * (un * un);
}


// tt[k][n] = |S_k^T w_n|^2: a 512-thread workgroup holds two adjacent row tiles of one topic, one per wave group, with BOTH wave
// groups multiplying in every phase ("concurrent" form).  Both walk the same (column tile, reduction chunk) sequence, so the S_k^T
// chunk is staged once into a double-buffered image both read, and every group double-buffers its own W chunk.  Grid: fwd_t_map_block.
// A removed form alternated the groups so that a SIMD's matrix pipe served one wave at a time; measured per phase (s_memtime, f16x3, mid-launch
// workgroup): multiply 1184 cycles for 768 cycles of MFMA, + ~110 (vmcnt) + ~180 (barrier) + ~400 (loop / address code) = ~1900
// cycles during which the OTHER group's wave on that SIMD idles - the pipe is busy 40 %.  That structure paid off when a chunk was
// 96 MFMAs (bf16x6) and staging went through ds_write; with 48 MFMAs per chunk the fixed per-phase costs dominate.  Here a chunk
// is ONE phase for all 8 waves: the next chunk's LDS-DMAs are issued first (from asm: hipcc would otherwise retire them in front
// of the fragment reads), then 16 fragment reads and 48 MFMAs per wave; the two waves of a SIMD share its pipe (2 x 768 cycles
// per phase) and hide each other's read latency and address code; vmcnt(0) + one barrier end the phase.
template <class SP>
__global__ __launch_bounds__(512, 2) void fwd_t_split_cc_kernel(FwdTSplitArgs<SP> g) {
  using CF = SplitCfg<SP>;
  using E = typename SP::E;
  using V8 = typename SP::V8;
  constexpr int NP = SP::NP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int IMG = CF::IMG;
  const int gp = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
  E* As = reinterpret_cast<E*>(smem) + gp * 2 * IMG;      // [2 buffers][NP][128][32] of this group
  E* Bs = reinterpret_cast<E*>(smem) + 4 * IMG;           // [2 buffers][NP][128][32] shared
  const int Mp = g.Mp;
  const int nct = (Mp + GDRF_TILE - 1) / GDRF_TILE;
  int64_t rt0; int bz;
  fwd_t_map_block(g, rt0, bz);
  const int64_t m0 = (rt0 + gp) * GDRF_TILE;                   // a tile past the end runs on clamped rows; its tt is never stored
  const SplitLane L;
  const int tid = L.tid, wr = L.wr, wc = L.wc, lr = L.lr, lg = L.lg;

  const int drow = L.drow(), dq = L.dq(), wave_u = L.wave_u();
  const unsigned a_lds = lds_addr(As), b_lds = lds_addr(Bs);
  // chunk (ct, kA) -> buffer buf: A rows of this group (2 row blocks per wave), B columns (1 row block per wave of the 8)
  // the requests of a chunk, one at a time (see bwd_wbar_split_cc_kernel: an LDS-DMA instruction stalls its wave ~190 cycles at issue,
  // which the MFMAs around it cover): slot 0 .. 2 NP - 1 = this group's A rows (2 row blocks per wave), 2 NP .. 3 NP - 1 = the B columns
  auto dma1 = [&](int ct, int kA, int buf, int slot) {
    if (slot < 2 * NP) {
      const int i = slot / NP, p = slot - i * NP;
      const int rbk = wave_u + 4 * i;
      int64_t row = m0 + rbk * 16 + drow;
      row = row < g.nrows ? row : 0;
      glds16_asm(g.Wh + p * g.w_stride + row * Mp + kA + dq, a_lds + (unsigned)(((buf * NP + p) * CF::PIECE + rbk * 512) * 2));
    } else {
      const int p = slot - 2 * NP;
      const int rbk = wave_u + 4 * gp, row = rbk * 16 + drow;
      const int col = (ct * GDRF_TILE + row < Mp) ? ct * GDRF_TILE + row : 0;
      glds16_asm(g.STh + p * g.piece_stride + (((int64_t)bz * (Mp >> 5) + (kA >> 5)) * Mp + col) * 32 + dq,
                 b_lds + (unsigned)(((buf * NP + p) * CF::PIECE + rbk * 512) * 2));
    }
  };
  auto dma = [&](int ct, int kA, int buf) {
#pragma unroll
    for (int sl = 0; sl < 3 * NP; ++sl) dma1(ct, kA, buf, sl);
  };
  float rs[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) rs[a][r] = 0;
  f32x4 acc[4][4];
  split_zero(acc);
  const int frag = L.frag();
  int ct = 0, kA = 0, buf = 0;
  dma(0, 0, 0);
  split_phase_end();
  while (ct < nct) {
    // the chunk after this one: next k block of the column tile, or the first one (k = 128 ct') of the next column tile
    int ct1 = ct, kA1 = kA + CF::BK;
    const bool last = kA1 >= Mp;
    if (last) { ct1 = ct + 1; kA1 = ct1 * GDRF_TILE; }
    const bool more = ct1 < nct;                               // buffers buf ^ 1 were last read one phase ago
    const E* Ab = As + buf * IMG;
    const E* Bb = Bs + buf * IMG;
    V8 fb[NP][4];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int b = 0; b < 4; ++b) fb[p][b] = split_frag<SP>(Bb, p, wc * 64 + b * 16, frag);
    V8 faq[2][NP];                                              // the next row group's fragments are read while this one multiplies
    split_frags<SP>(faq[0], Ab, wr * 64, frag);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      if (a + 1 < 4) split_frags<SP>(faq[(a + 1) & 1], Ab, wr * 64 + (a + 1) * 16, frag);
#pragma unroll
      for (int t = 0; t < SP::NPROD; ++t)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = SP::mma(faq[a & 1][SP::pa(t)], fb[SP::pb(t)][b], acc[a][b]);
      if (more) {                                               // the next chunk's requests, spread behind the MFMA groups
        constexpr int NS = 3 * NP, PER = (NS + 2) / 3;          // over a = 0, 1, 2
#pragma unroll
        for (int sl = a * PER; sl < (a + 1) * PER && sl < NS; ++sl) if (a < 3) dma1(ct1, kA1, buf ^ 1, sl);
      }
    }
    if (last) {                                                 // fold the finished column tile into the row sums, restart the accumulators
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const bool cok = fwd_t_col_ok(ct, b, Mp, L);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
          for (int r = 0; r < 4; ++r) rs[a][r] += fwd_t_sq(acc[a][b][r], cok);
          acc[a][b] = f32x4{0, 0, 0, 0};
        }
      }
    }
    split_phase_end();
    ct = ct1; kA = kA1; buf ^= 1;
  }
  // row sums: 16-lane groups, then the two waves of a group that share the rows, through LDS; the block scales come off here
  float* rsum = reinterpret_cast<float*>(smem) + gp * GDRF_TILE;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) rs[a][r] = group16_sum(rs[a][r]);
  __syncthreads();
  if (wc == 0 && lr == 0) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) rsum[wr * 64 + a * 16 + lg * 4 + r] = rs[a][r];
  }
  __syncthreads();
  if (wc == 1 && lr == 0) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) rsum[wr * 64 + a * 16 + lg * 4 + r] += rs[a][r];
  }
  __syncthreads();
  if (tid < GDRF_TILE) fwd_t_store_tt(g, bz, m0, tid, rsum[tid]);
}

// ------------------------------------------------------------------------------------------------------------------
// The concurrent form on a 256 x 256 workgroup tile: FOUR wave groups (2 row tiles x 2 column tiles, 16 waves, four per SIMD).
// Per 32-deep chunk the 512-thread form above moves 48 KB into LDS for 768 matrix-pipe cycles - 62 B/clk/CU, about twice what
// a CU's L2 -> LDS path sustains, so its phases were as long as their DMAs (9.8 ms for 4.5 ms of MFMAs at the held clock).
// Here both W images are read by two column groups and both S_k^T images by two row groups: 64 KB per 1536 pipe cycles.
// The triangle is kept at 128-column granularity: column group 1 of a pair starts 128 reduction indices later than group 0
// (S_k^T is zero above), sits those chunks out (its waves only issue their share of the DMAs) and its B image is not fetched.
// 8 images of NP x 8 KB: two-piece modes only (128 KB).
// The next chunk's requests are issued at the top of the phase (8.8 ms; behind the first two MFMA groups instead: 9.0 ms), and a
// scheduling barrier opens every row block (without it: 9.2 ms).
template <class SP>
__global__ __launch_bounds__(1024) void fwd_t_split_q4_kernel(FwdTSplitArgs<SP> g) {
  using CF = SplitCfg<SP>;
  using E = typename SP::E;
  using V8 = typename SP::V8;
  constexpr int NP = SP::NP;
  static_assert(NP == 2, "eight operand images must fit in LDS");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int IMG = CF::IMG;
  const int gp = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
  const int gr = gp >> 1, gc = gp & 1;
  const SplitLane L;
  const int tid = L.tid, lane = L.lane, wr = L.wr, wc = L.wc, lr = L.lr, lg = L.lg;
  const int w16 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // the wave among the workgroup's 16
  E* Asm = reinterpret_cast<E*>(smem);                    // [2 row groups][2 buffers][NP][128][32]
  E* Bsm = reinterpret_cast<E*>(smem) + 4 * IMG;          // [2 column groups][2 buffers][NP][128][32]
  const int Mp = g.Mp;
  const int nct = (Mp + GDRF_TILE - 1) / GDRF_TILE, ncp = (nct + 1) / 2;
  int64_t rt0; int bz;
  fwd_t_map_block(g, rt0, bz);
  const int64_t m0 = (rt0 + gr) * GDRF_TILE;                   // a tile past the end runs on clamped rows; its tt is never stored

  const int drow = L.drow(), dq = L.dq();
  const unsigned a_lds = lds_addr(Asm), b_lds = lds_addr(Bsm);
  // the 2 x NP x 8 requests (16 rows each) of either operand of a chunk are dealt over the 16 waves: slot s < NP of a wave is
  // request w16 NP + s of the W images, slot NP + s the same request of the S_k^T images (skipped while that column group is idle).
  // Sources are a wave-uniform base (row tile / reduction block, scalar) plus a per-lane 32-bit byte offset fixed for the launch.
  unsigned a_off[NP], b_off[NP];
#pragma unroll
  for (int sl = 0; sl < NP; ++sl) {
    const int rq = w16 * NP + sl, gi = rq / (8 * NP), rm = rq - gi * 8 * NP, rbk = rm & 7;
    const int r = rbk * 16 + drow;
    a_off[sl] = (unsigned)((((rt0 + gi) * GDRF_TILE + r < g.nrows) ? r : 0) * Mp + dq) * 2u;      // rows past the end read the tile's first row
    b_off[sl] = (unsigned)(r * 32 + dq) * 2u;
  }
  auto dma1 = [&](int cp, int kA, int buf, int slot) {
    const int sl = slot < NP ? slot : slot - NP;
    const int rq = w16 * NP + sl, gi = rq / (8 * NP), rm = rq - gi * 8 * NP, p = rm >> 3, rbk = rm & 7;
    if (slot < NP) {
      int64_t tb = (rt0 + gi) * GDRF_TILE;
      tb = tb < g.nrows ? tb : 0;
      glds16_asm_s(g.Wh + p * g.w_stride + tb * Mp + kA, a_off[sl], a_lds + (unsigned)((((gi * 2 + buf) * NP + p) * CF::PIECE + rbk * 512) * 2));
    } else {
      const int ctq = 2 * cp + gi;
      if (ctq < nct && kA >= ctq * GDRF_TILE) {
        // a partial last column tile: its rows past Mp are never summed; they read from column 0 of the same block instead
        const int cbase = (ctq * GDRF_TILE + rbk * 16 + 15 < Mp) ? ctq * GDRF_TILE : -(rbk * 16);
        glds16_asm_s(g.STh + p * g.piece_stride + (((int64_t)bz * (Mp >> 5) + (kA >> 5)) * Mp + cbase) * 32, b_off[sl],
                     b_lds + (unsigned)((((gi * 2 + buf) * NP + p) * CF::PIECE + rbk * 512) * 2));
      }
    }
  };
  // row sums of squares: one LDS slot per (row group, column group, wave column, row), behind the images; a finished column tile
  // is folded into it by its own wave (no other writer), so the order of the additions is fixed
  float* rsum = reinterpret_cast<float*>(smem + (size_t)8 * IMG * 2) + (gp * 2 + wc) * GDRF_TILE;
  rsum[wr * 64 + lane] = 0.0f;                            // this wave's 64 rows (ordered before its own later updates: same wave, LDS in order)
  f32x4 acc[4][4];
  split_zero(acc);
  const int frag = L.frag();
  int buf = 0;
#pragma unroll
  for (int sl = 0; sl < 2 * NP; ++sl) dma1(0, 0, 0, sl);
  split_phase_end();
  // Every chunk issues the requests of the chunk after it (the last one re-requests itself into the idle buffers: nobody reads them),
  // so the multiply loop has no branch around its DMAs; a group's idle chunks run in a loop of their own that never touches the
  // accumulators (with both in one loop body hipcc kept copies of them across the branch and spilled at 128 registers).
  auto next_chunk = [&](int cp, int kA, int& cp1, int& kA1) {
    cp1 = cp; kA1 = kA + CF::BK;
    if (kA1 >= Mp) {
      if (cp + 1 < ncp) { cp1 = cp + 1; kA1 = cp1 * 2 * GDRF_TILE; } else kA1 = kA;
    }
  };
#pragma unroll 1
  for (int cp = 0; cp < ncp; ++cp) {
    const int ct = 2 * cp + gc;
    int kA = cp * 2 * GDRF_TILE;
    // this wave multiplies the chunks kA >= k_act: S_k^T is zero above the diagonal, and for the wave's 64 columns (wc) that is every
    // reduction index below ct 128 + 64 wc - the triangle at 64-column granularity (10 % fewer MFMAs than at 128; the products skipped are exact zeros)
    const int k_act = (ct < nct) ? ct * GDRF_TILE + __builtin_amdgcn_readfirstlane(wc) * 64 : Mp;
#pragma unroll 1
    for (; kA < k_act && kA < Mp; kA += CF::BK) {
      int cp1, kA1;
      next_chunk(cp, kA, cp1, kA1);
#pragma unroll
      for (int sl = 0; sl < 2 * NP; ++sl) dma1(cp1, kA1, buf ^ 1, sl);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      gdrf_raw_barrier();
      buf ^= 1;
    }
#pragma unroll 1
    for (; kA < Mp; kA += CF::BK) {
      int cp1, kA1;
      next_chunk(cp, kA, cp1, kA1);
      const E* Ab = Asm + (gr * 2 + buf) * IMG;
      const E* Bb = Bsm + (gc * 2 + buf) * IMG;
#pragma unroll
      for (int sl = 0; sl < 2 * NP; ++sl) dma1(cp1, kA1, buf ^ 1, sl);
      V8 fb[NP][4];
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int b = 0; b < 4; ++b) fb[p][b] = split_frag<SP>(Bb, p, wc * 64 + b * 16, frag);
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        __builtin_amdgcn_sched_barrier(0);                       // keeps hipcc from hoisting the later row blocks' reads
        V8 fa[NP];                                               // one row block at a time: the SIMD's other three waves cover the read
        split_frags<SP>(fa, Ab, wr * 64 + a * 16, frag);
#pragma unroll
        for (int t = 0; t < SP::NPROD; ++t)
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] = SP::mma(fa[SP::pa(t)], fb[SP::pb(t)][b], acc[a][b]);
      }
      split_phase_end();
      buf ^= 1;
    }
    if (ct < nct) {                                             // fold the finished column tile into the row sums, restart the accumulators
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const bool cok = fwd_t_col_ok(ct, b, Mp, L);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[a][b][r] = fwd_t_sq(acc[a][b][r], cok);
        }
      }
#pragma unroll
      for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = group16_sum((acc[a][0][r] + acc[a][1][r]) + (acc[a][2][r] + acc[a][3][r]));
          if (lr == 0) rsum[wr * 64 + a * 16 + lg * 4 + r] += v;
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0, 0, 0, 0};
      }
    }
  }
  // the four partial sums of a row (2 column groups x 2 wave columns), added in a fixed order
  __syncthreads();
  if (gc == 0 && tid < GDRF_TILE) {
    const float* q = reinterpret_cast<const float*>(smem + (size_t)8 * IMG * 2) + (gr * 2) * 2 * GDRF_TILE + tid;
    fwd_t_store_tt(g, bz, m0, tid, (q[0] + q[GDRF_TILE]) + (q[2 * GDRF_TILE] + q[3 * GDRF_TILE]));
  }
}

// ------------------------------------------------------------------------------------------------------------------
// tt, ONE WAVE PER SIMD, S_k^T fed from L2 to registers (f16x3 only; Mp % 64 == 0, 2 <= K <= 16, many rows: the gate of bwd_wbar_f16_w1_kernel).
//
// What fwd_t_split_q4_kernel spends beside its MFMAs is requests and fragment reads behind a 16-wave barrier per 32-deep chunk, half of them
// for the small operand.  STh has Bh's k-blocked layout, so - as in bwd_wbar_f16_w1_kernel - a 16-column x 32-k MFMA B fragment is 1 024
// contiguous bytes and one global_load_dwordx4 per wave delivers it finished from the XCD's L2: no M0, no image, no ds_read, no barrier.
// 256 threads, one wave per SIMD; a wave owns 128 rows and, of the current 128-column tile, the 64 columns of half w & 1, for TWO topics.  Two
// geometries of a workgroup (g.KG counts its topic groups per L2 group; the launch covers the topics [g.k_lo, g.k_lo + g.k_n), a topic past
// the end is the last one again and is not stored):
//   pair (QUAD = false)  two row tiles x two topics: wave pair w >> 1 = row tile, W-bar w1's geometry, 16 W requests per wave and block.  Every
//                        column tile re-streams its W blocks for two topics only (25 GB per launch at the headline shape unless the KG adjacent
//                        workgroups of a row pair share them in L2): alone it only matched q4
//   quad (QUAD = true)   ONE row tile x four topics: wave pair w >> 1 = topic pair, all four waves read one 32 KB image, 8 requests per wave and
//                        block, g.rt8 counts single row tiles.  Half the W bytes per topic and row with no reliance on L2 sharing
// The host runs K / 4 * 4 topics on the quad form and the rest on the pair form.  The workgroup walks the column tiles ct and, per tile, the
// 64-deep reduction blocks q = 2 ct .. Mp / 64 - 1 (S_k^T is zero above the diagonal); the triangle is kept at 64 columns per wave: the waves of
// column half 1 sit out a tile's first block and only issue their share of its W requests.  Per lane, ALL named literally in the asm:
//   a[0:255]    accumulators [topic 0/1][row group 0-7][column group 0-3][4]: C/D of MFMAs with A/B in VGPRs.  Nothing but MFMAs writes them
//               until a column tile is finished; a tile's first product of each uses C = 0 (the wave's first block of a tile is a second
//               instantiation of the block body): nothing is ever cleared
//   v[64:191]   W fragments of the block [k-step][row group][piece], ds_read_b128 once per block from the double-buffered image (W1Image)
//   v[192:255]  S_k^T fragment ring [column group][k-step][piece]: a register is requested again, for the next (block, topic) phase, right
//               behind its last MFMA of this phase - every load is three column groups (~2 300 pipe cycles) ahead of its use
//   v[0:63]     hipcc's
// (Compiler-allocated f16x8 variables for the fragments and the ring, loaded by asm with "+v": hipcc copied and spilled ring registers whose
// loads were in flight - 201 spilled VGPRs.)
// THE REGISTERS ARE A CONTRACT HIPCC DOES NOT KNOW ABOUT: it sees them only as clobbers - of the first MFMA of a column group, of every
// statement that loads a fragment, of the fold's reads (the ring is live, even in flight, across the fold) -, which keeps everything of its own
// that lives across such a statement in v[0:63] and makes the kernel descriptor allocate 256 + 256.  The kernel is right only while no
// compiler-generated instruction touches v[64:255] or an AGPR between the prologue's barrier and the final one, and while hipcc issues no
// vector-memory or scalar-memory instruction of its own there (the waits are literal counts).  After ANY edit of this kernel or of W1Image, and
// after a compiler change, repeat the check: `hipcc -save-temps`; in the assembly of both instantiations, between those barriers, no instruction
// outside the #ASMSTART / #ASMEND pairs names v64 or higher or an AGPR, the 256 `v_accvgpr_read_b32` all belong to the fold, and there is no
// `v_accvgpr_write`, no `scratch_`, no `s_load`, no `global_load` / `buffer_load` of hipcc's; and `make resources`: VGPRs 256, AGPRs 256,
// ScratchSize 0, occupancy 1.  tests/test_gpu_fwd_t_w1.py runs both instantiations at every edge.
//
// Schedule of a phase = (block, topic) = 4 column groups x 48 MFMAs, each group two halves of 24 (row groups 0 - 3, then 4 - 7; per half
// k-step-major, then the products SP::pa/pb(t): per accumulator q4's six products per 64-deep block in q4's order).  Behind MFMA m of a group:
//   W requests   of the NEXT block's image: NG = 4 (pair) or 2 (quad) behind m = 2, 8, .. of the groups 0 and 2 (1 per 24 / 48 MFMAs, far
//                apart: a request waits for M0 until the one before has read it)
//   ring loads   of the group's own registers for the next phase, behind m = 27, 35, 39, 47: the last MFMA that reads each
//   W fragments  eight are read behind the block's barrier, the other 24 one per gap behind the first 24 MFMAs of the block, in the order
//                of their first use; LDS returns in order, so MFMA m waits by lgkmcnt(issued so far - needed so far)
// The counts are the same in every phase (the last phase re-requests itself, the last block's image goes to the idle buffer), so every wait
// is a literal vmcnt: in front of a group, the 12 + NG (even group) or 12 + 2 NG (odd group) operations issued since its loads; in front of a
// block's barrier the 8 ring loads issued behind the last W request (0 after a block the wave sat out).  vmcnt retires in order: the requests
// of a phase have to land within one phase, whatever the depth of the image's buffering.  One workgroup barrier per block publishes the image.
// The fold of a finished tile (two s_nop 15, then v_accvgpr_read, the squares masked by fwd_t_col_ok and summed over the four column groups,
// the 16 lanes by row16_sum_lane0) adds into one LDS slot per (topic, row tile, tile parity, column half, row) in q4's order; the final sum is
// q4's too: (q0 + q1) + (q2 + q3).  No atomics: tt is bit-identical from run to run.
constexpr int ft1_acc(int tp, int a, int b) { return ((tp * 8 + a) * 4 + b) * 4; }
// v64 .. v255, as GDRF_ALL_AGPRS
#define GDRF_V10(p) "v" p "0", "v" p "1", "v" p "2", "v" p "3", "v" p "4", "v" p "5", "v" p "6", "v" p "7", "v" p "8", "v" p "9"
#define GDRF_RING_VGPRS "v192", "v193", "v194", "v195", "v196", "v197", "v198", "v199", GDRF_V10("20"), GDRF_V10("21"), GDRF_V10("22"), \
                        GDRF_V10("23"), GDRF_V10("24"), "v250", "v251", "v252", "v253", "v254", "v255"
#define GDRF_W1_VGPRS "v64", "v65", "v66", "v67", "v68", "v69", GDRF_V10("7"), GDRF_V10("8"), GDRF_V10("9"), GDRF_V10("10"), GDRF_V10("11"), \
                      GDRF_V10("12"), GDRF_V10("13"), GDRF_V10("14"), GDRF_V10("15"), GDRF_V10("16"), GDRF_V10("17"), GDRF_V10("18"), "v190", "v191", \
                      GDRF_RING_VGPRS
constexpr int ft1_wreg(int ks, int a, int p) { return 64 + ((ks * 8 + a) * 2 + p) * 4; }
constexpr int ft1_rreg(int b, int ks, int p) { return 192 + ((b * 2 + ks) * 2 + p) * 4; }
// a[D:D+3] = (ZERO ? 0 : a[D:D+3]) + W fragment v[WA:WA+3] x S_k^T fragment v[RB:RB+3]; CLOB: tell hipcc that the registers are in use
template <int D, int WA, int RB, bool ZERO, bool CLOB> __device__ __forceinline__ void ft1_mfma() {
  if constexpr (ZERO && CLOB)
    asm volatile("v_mfma_f32_16x16x32_f16 a[%c0:%c1], v[%c2:%c3], v[%c4:%c5], 0" : : "i"(D), "i"(D + 3), "i"(WA), "i"(WA + 3), "i"(RB), "i"(RB + 3) : GDRF_ALL_AGPRS, GDRF_W1_VGPRS);
  else if constexpr (ZERO)
    asm volatile("v_mfma_f32_16x16x32_f16 a[%c0:%c1], v[%c2:%c3], v[%c4:%c5], 0" : : "i"(D), "i"(D + 3), "i"(WA), "i"(WA + 3), "i"(RB), "i"(RB + 3));
  else if constexpr (CLOB)
    asm volatile("v_mfma_f32_16x16x32_f16 a[%c0:%c1], v[%c2:%c3], v[%c4:%c5], a[%c0:%c1]" : : "i"(D), "i"(D + 3), "i"(WA), "i"(WA + 3), "i"(RB), "i"(RB + 3) : GDRF_ALL_AGPRS, GDRF_W1_VGPRS);
  else
    asm volatile("v_mfma_f32_16x16x32_f16 a[%c0:%c1], v[%c2:%c3], v[%c4:%c5], a[%c0:%c1]" : : "i"(D), "i"(D + 3), "i"(WA), "i"(WA + 3), "i"(RB), "i"(RB + 3));
}
// v[REG:REG+3] = the lane's 16 bytes at sbase (wave-uniform) + voff + OFF / at LDS address addr + OFF.  Not counted by hipcc: the caller waits
// by vmcnt(n) / lgkmcnt(n).
template <int REG, int OFF> __device__ __forceinline__ void ft1_gload(const void* sbase, unsigned voff) {
  asm volatile("global_load_dwordx4 v[%c2:%c3], %0, %1 offset:%c4" : : "v"(voff), "s"(sbase), "i"(REG), "i"(REG + 3), "i"(OFF) : "memory", GDRF_W1_VGPRS);
}
template <int REG, int OFF> __device__ __forceinline__ void ft1_ldsread(unsigned addr) {
  asm volatile("ds_read_b128 v[%c1:%c2], %0 offset:%c3" : : "v"(addr), "i"(REG), "i"(REG + 3), "i"(OFF) : "memory", GDRF_W1_VGPRS);
}
// the fold's reads: the ring is live (in flight, even) across them
template <int REG> __device__ __forceinline__ float ft1_accread() {
  float x;
  asm volatile("v_accvgpr_read_b32 %0, a[%c1]" : "=v"(x) : "i"(REG) : GDRF_ALL_AGPRS, GDRF_RING_VGPRS);
  return x;
}

template <bool QUAD>
__global__ __launch_bounds__(256, 1) void fwd_t_f16_w1_kernel(FwdTSplitArgs<SplitF16> g) {
  using SP = SplitF16;
  using CF = SplitCfg<SP>;
  using E = typename SP::E;
  constexpr int PIECE = CF::PIECE, WIMG = W1_WIMG;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // LDS: W images [2 buffers][NT row tiles] (128 or 64 KB), then the row sums: pair form [topic 0/1][row tile][tile parity][column half][128],
  // quad form [topic 0-3][tile parity][column half][128]
  constexpr int NT = QUAD ? 1 : 2, G = QUAD ? 4 : 2;                    // row tiles and topics of a workgroup
  constexpr int RS_TP = QUAD ? 4 : 8;                                   // slots between a wave's two topics
  SplitLane L;
  const int w = L.wave_u(), gp = w >> 1, wc = w & 1;
  L.wc = wc;
  const int Mp = g.Mp;
  const int nk = Mp / 64, nct = (Mp + GDRF_TILE - 1) / GDRF_TILE;
  FwdTSplitArgs<SP> gm = g;
  gm.K = (g.k_n + G - 1) / G;                                             // the block map deals topic groups (and row-tile pairs)
  int64_t rt0; int bp;
  fwd_t_map_block(gm, rt0, bp);
  if constexpr (QUAD) rt0 >>= 1;                                          // ... single row tiles here: gm.rt8 counts them
  // pair form: wave pair gp = row tile gp, both on the group's two topics; quad form: one row tile, wave pair gp = the group's topic pair gp
  const int k_end = g.k_lo + g.k_n, kw = g.k_lo + G * bp + (QUAD ? 2 * gp : 0);
  const int k0 = min(kw, k_end - 1), k1 = min(kw + 1, k_end - 1);      // a topic past the end: the last one again, never stored
  const int64_t m0 = (rt0 + (QUAD ? 0 : gp)) * GDRF_TILE;               // a tile past the end runs on clamped rows; its tt is never stored
  const int lr = L.lr, lg = L.lg;
  const unsigned w_lds = lds_addr(smem) + (unsigned)(QUAD ? 0 : gp * WIMG);
  const unsigned frag_addr = w_lds + (unsigned)(L.frag() * 2);
  const W1Image<QUAD ? 4 : 2> WI(g.Wh, g.w_stride, g.nrows, Mp, m0, w_lds, NT * WIMG, QUAD ? w : wc, L);
  constexpr int NREQ = 32 / (QUAD ? 4 : 2), RQ = NREQ / 2, NG = RQ / 2; // requests per wave and block, per topic phase, per column group 0 / 2
  float* const rs_base = reinterpret_cast<float*>(smem + 2 * NT * WIMG);
  float* const rs_wave = rs_base + ((QUAD ? gp * 8 : gp * 4) + wc) * GDRF_TILE;           // + (topic * RS_TP + 2 * parity) * 128
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    rs_wave[((i >> 1) * RS_TP + 2 * (i & 1)) * GDRF_TILE + L.lane] = 0.0f;
    rs_wave[((i >> 1) * RS_TP + 2 * (i & 1)) * GDRF_TILE + 64 + L.lane] = 0.0f;
  }

  // S_k^T fragments of phase (ct, q, topic): a wave-uniform base per (k-step, piece), one lane offset, the column group in the immediate offset
  const unsigned voff_b = (unsigned)((lr * 32 + 8 * lg) * 2);
  const int64_t b_ks = (int64_t)Mp * 32, b_top = (int64_t)(Mp >> 5) * b_ks;     // elements per 32-deep k block and per topic
  const int64_t dtop = (int64_t)(k1 - k0) * b_top;
  const E* const st0 = g.STh + (int64_t)k0 * b_top;
  const int64_t p_stride = g.piece_stride;
  auto phase_base = [&](int ct, int q) {    // topic k0; a column half past Mp is never multiplied: its loads read the tile's first columns
    const int col = ct * GDRF_TILE + wc * 64;
    return st0 + (int64_t)(2 * q) * b_ks + (int64_t)(col < Mp ? col : ct * GDRF_TILE) * 32;
  };
  const E* sb[2][2];
  auto b_bases = [&](const E* b0) {
    sb[0][0] = b0; sb[1][0] = b0 + b_ks; sb[0][1] = b0 + p_stride; sb[1][1] = b0 + b_ks + p_stride;
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("" : "+s"(sb[i >> 1][i & 1]));   // they exist here, far ahead of the loads that read them
  };


  // prologue: the first block's W image, the fragments of the wave's first phase (column half 1: block 1, if there is one)
  static_for<NREQ>([&](auto jc) { WI.template request<RQ, decltype(jc)::value % RQ>(0, 0, decltype(jc)::value / RQ); });
  const E* b_cur = phase_base(0, wc < nk ? wc : 0);
  b_bases(b_cur);
  static_for<16>([&](auto jc) {
    constexpr int j = decltype(jc)::value, bb = j >> 2, ks = (j >> 1) & 1, p = j & 1;
    ft1_gload<ft1_rreg(bb, ks, p), bb * 1024>(sb[ks][p], voff_b);
  });
  wb1_vmcnt<0>();
  __syncthreads();

  // one active block: both topic phases.  FIRST: the wave's first block of the column tile
  auto block_body = [&](auto firstc, int qn, int bufn, const E* next_blk, unsigned fa) {
    constexpr bool FIRST = decltype(firstc)::value;
    // W fragment f = 0 .. 31, in the order of their first use: (half, k-step, piece, row group of the half).  Eight up front, the others one per
    // gap behind the first 24 MFMAs; LDS returns in order, so MFMA m waits for its fragments by lgkmcnt(issued so far - needed so far)
    auto wread = [&](auto fc) {
      constexpr int f = decltype(fc)::value, ks = (f >> 3) & 1, p = (f >> 2) & 1, a = (f >> 4) * 4 + (f & 3);
      ft1_ldsread<ft1_wreg(ks, a, p), ((ks * 2 + p) * PIECE + a * 16 * 32) * 2>(fa);
    };
    static_for<8>(wread);
    static_for<2>([&](auto tc) {
      constexpr int tp = decltype(tc)::value;
      const E* const b_next = tp == 0 ? b_cur + dtop : next_blk;
      b_bases(b_next);
      static_for<4>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        wb1_vmcnt<(b & 1) ? 12 + 2 * NG : 12 + NG>();
        static_for<48>([&](auto mc) {
          constexpr int m = decltype(mc)::value, half = m / 24, mm = m % 24, ks = mm / 12, t = (mm >> 2) % 3, a = half * 4 + (mm & 3);
          if constexpr (tp == 0 && b == 0) {
            if constexpr (m == 0 || m == 4 || m == 36) asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
            if constexpr (m == 12 || m == 16 || m == 28) asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
            if constexpr (m == 24) asm volatile("s_waitcnt lgkmcnt(12)" ::: "memory");
            if constexpr (m == 40) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          }
          ft1_mfma<ft1_acc(tp, a, b), ft1_wreg(ks, a, SP::pa(t)), ft1_rreg(b, ks, SP::pb(t)), FIRST && mm < 4, m == 0>();
          if constexpr (tp == 0 && b == 0 && m < 24) wread(std::integral_constant<int, 8 + m>{});
          if constexpr ((b == 0 || b == 2) && m < 6 * NG && m % 6 == 2) WI.template request<RQ, (b == 0 ? 0 : NG) + (m - 2) / 6>(qn, bufn, tp);
          if constexpr (m == 27) ft1_gload<ft1_rreg(b, 0, 1), b * 1024>(sb[0][1], voff_b);
          if constexpr (m == 35) ft1_gload<ft1_rreg(b, 0, 0), b * 1024>(sb[0][0], voff_b);
          if constexpr (m == 39) ft1_gload<ft1_rreg(b, 1, 1), b * 1024>(sb[1][1], voff_b);
          if constexpr (m == 47) ft1_gload<ft1_rreg(b, 1, 0), b * 1024>(sb[1][0], voff_b);
        });
      });
      b_cur = b_next;
    });
  };

  int ct = 0, q = 0, s = 0;
  bool sat = false;
#pragma unroll 1
  for (;;) {
    // the workgroup's next block (the last one requests its own image again, into the idle buffer)
    int ctn = ct, qn = q + 1;
    bool more = true;
    if (qn >= nk) {
      ctn = ct + 1; qn = 2 * ctn;
      if (ctn >= nct) { more = false; ctn = ct; qn = q; }
    }
    const int bufn = (s + 1) & 1;
    if (s > 0) {                              // this block's W image is complete and every wave has read the one before
      if (sat) wb1_vmcnt<0>(); else wb1_vmcnt<8>();
      gdrf_raw_barrier();
    }
    if (q >= 2 * ct + wc) {
      // the wave's next block (the last phase requests its own fragments again)
      const E* next_blk = b_cur + dtop;
      if (q + 1 < nk) next_blk = phase_base(ct, q + 1);
      else if (ct + 1 < nct && 2 * (ct + 1) + wc < nk) next_blk = phase_base(ct + 1, 2 * (ct + 1) + wc);
      const unsigned fa = frag_addr + (unsigned)((s & 1) * NT * WIMG);
      if (q == 2 * ct + wc) block_body(std::true_type{}, qn, bufn, next_blk, fa);
      else block_body(std::false_type{}, qn, bufn, next_blk, fa);
      sat = false;
    } else {                                  // column half 1, first block of a tile: only its share of the next image
      static_for<NREQ>([&](auto jc) { WI.template request<RQ, decltype(jc)::value % RQ>(qn, bufn, decltype(jc)::value / RQ); });
      sat = true;
    }
    if (q == nk - 1) {                        // fold the finished column tile into the row sums; the next tile's first products start from 0
      asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
      float* const slot = rs_wave + 2 * (ct & 1) * GDRF_TILE + lg * 4;
      bool cok[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) cok[b] = fwd_t_col_ok(ct, b, Mp, L);
      static_for<16>([&](auto ic) {
        constexpr int tp = decltype(ic)::value >> 3, a = decltype(ic)::value & 7;
        f32x4 v;
        static_for<4>([&](auto rc) {
          constexpr int r = decltype(rc)::value;
          const float x0 = fwd_t_sq(ft1_accread<ft1_acc(tp, a, 0) + r>(), cok[0]), x1 = fwd_t_sq(ft1_accread<ft1_acc(tp, a, 1) + r>(), cok[1]);
          const float x2 = fwd_t_sq(ft1_accread<ft1_acc(tp, a, 2) + r>(), cok[2]), x3 = fwd_t_sq(ft1_accread<ft1_acc(tp, a, 3) + r>(), cok[3]);
          v[r] = row16_sum_lane0((x0 + x1) + (x2 + x3));
        });
        if (lr == 0) {
          f32x4* const p = reinterpret_cast<f32x4*>(slot + tp * RS_TP * GDRF_TILE + a * 16);
          *p = *p + v;
        }
      });
    }
    if (!more) break;
    ct = ctn; q = qn; ++s;
  }
  wb1_vmcnt<0>();
  // the four partial sums of a row (2 tile parities x 2 column halves), added in a fixed order; an odd K's second topic is the first again
  __syncthreads();
  for (int e = L.tid; e < 4 * GDRF_TILE; e += 256) {
    const int sl = e >> 7, row = e & 127;                                // pair form: slot group (topic, row tile); quad form: topic
    const int kt = g.k_lo + G * bp + (QUAD ? sl : sl >> 1);
    const float* qd = rs_base + sl * 4 * GDRF_TILE + row;
    if (kt < k_end)
      fwd_t_store_tt(g, kt, (rt0 + (QUAD ? 0 : sl & 1)) * GDRF_TILE, row, (qd[0] + qd[GDRF_TILE]) + (qd[2 * GDRF_TILE] + qd[3 * GDRF_TILE]));
  }
}

// ------------------------------------------------------------------------------------------------------------------
// TN form (reduction over observations):  C[i][j] = sum_n A[n][i] * s[n] * B[n][j]  on the same emulation; replaces
// gemm_tn_kernel<float> for A_k = W^T diag(vbar_k) W (sym) and GT = W^T Wbar.  A comes pre-split (Wh), B is f32 and is
// scaled by s[n] (and its block scale) and split when it is staged (the scale runs along the reduction index, so it cannot be
// pulled out of the product).  Both operands are staged as they lie in memory (n-major rows) and the MFMA fragments (8
// consecutive n per lane) are gathered with the transposing LDS read ds_read_b64_tr_b16 (cdna_hip_programming.md T10).
//
// LDS piece image of a 32 (n) x 128 (column) chunk: row-major (256-byte rows, so an LDS-DMA instruction fills 4 whole rows
// from the row-major pieces), with the 8-byte column quad c4 XOR-swizzled by the row:
//   seg(k, c4) = k * 32 + (c4 ^ (code(k) << 2)),  code(k) = ((k >> 3) & 1) << 2 | (k & 3)      (8-byte segments)
// A transposing fragment read of a half-wave touches rows k = 8 lg + 4 h + q (lg in {0,1} or {2,3}, q = 0..3) x quads base + p,
// p = 0..3: the eight (lg & 1, q) codes send the eight rows to eight different 32-byte groups of the 256-byte bank window -
// conflict-free.  The pre-split A operand is staged by DMA (double-buffered, no registers, no LDS stores); the B operand, which
// must be scaled and split, goes through registers and NP ds_write_b128 per row pair.
template <class SP> struct TNSplitArgs {
  const typename SP::E* Ah; int64_t a_stride; int64_t lda;     // pieces [p][n][lda]
  const float* B; int64_t ldb;                         // [n][ldb]
  const float* scale; int64_t scale_bs;                // optional per-row scale, batch stride; nullptr = 1
  int64_t nrows, rows_per_split;                       // rows_per_split multiple of 32
  int ncols, sym;
  float* slab;                                         // [nsplit][nbatch][ncols][ncols]
  int nbatch, nsplit;
  const float* sc; int sidx_a;                         // block scales: pair index of the A pieces' scale,
  int sidx_b, sidx_b_stride;                           //   of the (row-scaled) B operand's: sidx_b + stride * batch
};

__device__ __forceinline__ int tnb_code(int k) { return (((k >> 3) & 1) << 2) | (k & 3); }
__device__ __forceinline__ int tnb_seg(int k, int c4) { return k * 32 + (c4 ^ (tnb_code(k) << 2)); }

__device__ __forceinline__ bf16x4 tr_read(const __bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)p);
}
__device__ __forceinline__ f16x4 tr_read(const _Float16* p) {
  typedef __fp16 h4 __attribute__((__vector_size__(4 * sizeof(__fp16))));       // the builtin's own vector type; same bits
  return __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) h4*)p));
}

// 192 registers at most (amdgpu_num_vgpr counts half of the unified file): one wave of this kernel then shares a SIMD's 512 with two
// 160-register waves of bwd_knm on the other stream (api.hip), which is how G^T runs inside that kernel's stalls
template <class SP>
__global__ __launch_bounds__(256, 2) __attribute__((amdgpu_num_vgpr(96))) void gemm_tn_split_kernel(TNSplitArgs<SP> g) {
  using E = typename SP::E;
  using V8 = typename SP::V8;
  using V4 = typename SP::V4;
  constexpr int NP = SP::NP;
  constexpr int PIECE = 32 * 128;             // halfwords per piece image (8 KB)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  E* As = reinterpret_cast<E*>(smem);         // [2 buffers][NP][32][128]
  E* Bs = As + 2 * NP * PIECE;                // [NP][32][128]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, lr = lane & 15, lg = lane >> 4;
  const int nt = (g.ncols + GDRF_TILE - 1) / GDRF_TILE;
  const int ntiles = g.sym ? nt * (nt + 1) / 2 : nt * nt;
  int tile, b, sp;                            // block -> (tile, batch, split) exactly as gemm_tn_kernel (gemm_tn.h)
  {
    const unsigned bid = blockIdx.x;
    if ((g.nsplit & 7) == 0) {
      const unsigned xcd = bid & 7u, idx = bid >> 3, per = (unsigned)(ntiles * g.nbatch);
      const unsigned sl = idx / per, r = idx - sl * per;
      sp = (int)(sl * 8u + xcd); b = (int)(r / (unsigned)ntiles); tile = (int)(r % (unsigned)ntiles);
    } else {
      tile = (int)(bid % (unsigned)ntiles);
      const unsigned r = bid / (unsigned)ntiles;
      b = (int)(r % (unsigned)g.nbatch); sp = (int)(r / (unsigned)g.nbatch);
    }
  }
  int ti, tj;
  if (g.sym) {
    int t = tile; ti = 0;
    while (t >= ti + 1) { t -= ti + 1; ++ti; }
    tj = t;
  } else { ti = tile / nt; tj = tile % nt; }
  const int i0 = ti * GDRF_TILE, j0 = tj * GDRF_TILE;
  const int64_t r0 = (int64_t)sp * g.rows_per_split;
  int64_t r1 = r0 + g.rows_per_split; if (r1 > g.nrows) r1 = g.nrows;
  const float* sc = g.scale ? g.scale + (int64_t)b * g.scale_bs : nullptr;
  const int sb = g.sidx_b + g.sidx_b_stride * b;
  const float bscale = g.sc[sb];                               // applied to s[n] B[n][j] at the split
  const float unscale = g.sc[g.sidx_a + 1] * g.sc[sb + 1];     // taken off the result

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = f32x4{0, 0, 0, 0};

  // A: DMA, 4 rows (1 KB) per instruction: lane l -> row l>>4, physical 16-byte unit l&15 = logical unit (l&15) ^ (code << 1);
  // this wave moves row blocks wave and wave + 4 of every piece.  Rows past the split / the end meet a zero B row; columns past
  // the end give rows of C that are never stored.
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);     // provably wave-uniform: the DMA's LDS base goes to M0 without a waterfall loop
  typedef const __attribute__((address_space(1))) void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  const int nch = r0 < r1 ? (int)((r1 - r0 + 31) / 32) : 0;
  const unsigned as_base = lds_addr(As) + (unsigned)wave_u * 1024u;
  auto dma_a = [&](int c) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int blk = wave_u + 4 * i, k = 4 * blk + (lane >> 4);
      const int c8 = (lane & 15) ^ (tnb_code(k) << 1);
      int64_t n = r0 + (int64_t)c * 32 + k;
      n = n < g.nrows ? n : g.nrows - 1;
      const int col = (i0 + c8 * 8 < g.ncols) ? i0 + c8 * 8 : 0;
#pragma unroll
      for (int p = 0; p < NP; ++p)
        glds16_asm(g.Ah + p * g.a_stride + n * g.lda + col, as_base + (unsigned)((((c & 1) * NP + p) * PIECE + 4 * i * 512) * 2));
    }
  };
  // B: 8 columns of a row per vector pair (q = tid&3 -> row 4*(khi + 4 i) + q, c8 = (tid>>2)&15, khi = tid>>6), 2 rows per thread:
  // two adjacent f32x4 loads, and after the split ONE ds_write_b128 per piece (the swizzle keeps the quads 2 c8, 2 c8 + 1 adjacent)
  const int sq = tid & 3, b_c8 = (tid >> 2) & 15, b_kh = tid >> 6;
  const bool b_ok = (j0 + b_c8 * 8) < g.ncols;                // ncols multiple of 32
  f32x4 rb[4];                                                 // [2 i + half]
  float rs[2], okf[2];
  // Nothing here may depend on the loaded VALUES: a select or a scale applied to the prefetched registers at load time makes
  // hipcc wait for the loads (vmcnt(0)) right here, in front of the MFMAs of the current chunk - the whole HBM latency exposed
  // once per chunk.  Rows past the split / the end are read from a valid (clamped) row and annihilated by okf = 0 at the split.
  auto load_b = [&](int c) {
    const int64_t rbase = r0 + (int64_t)c * 32;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t n = rbase + 4 * (b_kh + 4 * i) + sq;
      const int64_t nn = n < g.nrows ? n : g.nrows - 1;
      const float* src = g.B + nn * g.ldb + (b_ok ? j0 + b_c8 * 8 : 0);
      rb[2 * i] = *reinterpret_cast<const f32x4*>(src);
      rb[2 * i + 1] = *reinterpret_cast<const f32x4*>(src + 4);
      rs[i] = sc ? sc[nn] : 1.0f;
      okf[i] = (b_ok && n < r1) ? 1.0f : 0.0f;
    }
  };
  // fragments: two transposing reads (k = 8 lg + q and + 4) of 4 rows x 16 columns each; seg = (8 lg + 4 h + q) * 32 + ((4 w + t) ^ code) * 4 + p
  const int fq = lr >> 2, fp = lr & 3, fcode = ((lg & 1) << 2) | fq;
  const int fbase = (8 * lg + fq) * 32 + fp;
  int xa[4], xb[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) { xa[t] = fbase + (((4 * wr + t) ^ fcode) << 2); xb[t] = fbase + (((4 * wc + t) ^ fcode) << 2); }
  auto frag = [&](const E* img, int seg) -> V8 {
    const V4 lo = tr_read(img + seg * 4);
    const V4 hi = tr_read(img + (seg + 128) * 4);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  };

  // symmetric problem, diagonal tile: the quadrant above the diagonal (rows 0-63 x columns 64-127) is the mirror image of the one
  // below it and reduce_slabs_kernel takes it from there.  Its wave skips fragment reads and MFMAs - a quarter of the tile's LDS
  // read traffic - and only stages.
  const bool idle = g.sym && ti == tj && __builtin_amdgcn_readfirstlane(wave) == 1;
  if (nch > 0) { dma_a(0); load_b(0); }
  for (int c = 0; c < nch; ++c) {
    // scale and split the prefetched B vectors BEFORE the barrier: the conversion then overlaps the other waves' MFMAs
    // instead of sitting in the barrier-to-barrier staging section
    V8 pb[2][NP];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float s = rs[i] * okf[i] * bscale;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        E p[NP];
        SP::split(rb[2 * i + (e >> 2)][e & 3] * s, p);
        // f16x3: the row-scaled operand's block scale comes from a maximum (an outlier statistic), the bulk of its entries sits many
        // binades lower and their low piece would fall into fp16's subnormals: it is stored as l' = 2^11 l and multiplied with 2^-11 h_a
        // (gemm_tn_topics.h has the measurement: 15 -> 22 bits on a contracted posterior)
        if constexpr (SP::ID == 2) {
          float r = rb[2 * i + (e >> 2)][e & 3] * s - (float)p[0];
          asm volatile("" : "+v"(r));                  // keeps the SLP vectorizer off this arithmetic (gemm_tn_topics.h: split_pair)
          p[1] = (E)(r * 2048.0f);
        }
#pragma unroll
        for (int q = 0; q < NP; ++q) pb[i][q][e] = p[q];
      }
    }
    __syncthreads();                       // (its vmcnt(0) also retires this wave's DMA of chunk c, issued one iteration ago)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int so = tnb_seg(4 * (b_kh + 4 * i) + sq, 2 * b_c8) * 4;
#pragma unroll
      for (int q = 0; q < NP; ++q) *reinterpret_cast<V8*>(Bs + q * PIECE + so) = pb[i][q];
    }
    __syncthreads();
    if (c + 1 < nch) { dma_a(c + 1); load_b(c + 1); }          // A buffer (c+1)&1 was last read in iteration c-1
    if (idle) continue;                                        // staged and synchronised with the others; nothing of its own to multiply
    const E* Ab = As + (c & 1) * NP * PIECE;
    V8 fb[NP][4];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int t = 0; t < 4; ++t) fb[p][t] = frag(Bs + p * PIECE, xb[t]);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      V8 fa[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) fa[p] = frag(Ab + p * PIECE, xa[a]);
      V8 fa2 = fa[0];
      if constexpr (SP::ID == 2) fa2 = fa[0] * (E)0.00048828125f;          // 2^-11 h_a: partner of the B operand's up-scaled low piece (product 0 = h_a l_b)
#pragma unroll
      for (int t2 = 0; t2 < SP::NPROD; ++t2)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[a][t] = SP::mma((SP::ID == 2 && t2 == 0) ? fa2 : fa[SP::pa(t2)], fb[SP::pb(t2)][t], acc[a][t]);
    }
  }
  if (idle) return;
  float* out = g.slab + ((int64_t)sp * g.nbatch + b) * (int64_t)g.ncols * g.ncols;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + wr * 64 + a * 16 + lg * 4 + r;
        const int j = j0 + wc * 64 + c * 16 + lr;
        if (i < g.ncols && j < g.ncols) out[(int64_t)i * g.ncols + j] = acc[a][c][r] * unscale;
      }
}

}  // namespace gdrf
