// The kernel form of every shape-dispatched stage, and what its launch derives from the shape, as pure functions of a handful of integers.
// Host only, plain C++17, the standard library alone: api.hip asks these plans and switches on the form; tools/ and tests/host/forms_table.cpp
// ask the same functions without a GPU.  The form codes are the numbers of gdrf_last_forms (include/gdrf_hip.h).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace gdrf {
namespace forms {

// ---- constants the kernels also use, restated; api.hip ties each one to its original with a static_assert
constexpr int F_TILE = 128;              // GDRF_TILE
constexpr int F_MPAD = 32;               // GDRF_MPAD
constexpr int F_DMAX = 4;                // GDRF_DMAX
constexpr int F_KMAX = 32;               // GDRF_KMAX
constexpr int F_LOC_KMAX = 16;           // LOC_KMAX
constexpr int F_TNT_KT = 10;             // TNT_KT
constexpr int F_TN1_CH = 64;             // TN1_CH
constexpr int F_VEC = 16;                // bytes of a Vec16<T>
constexpr int F_IMG_F16 = 2 * 128 * 32;  // SplitCfg<SplitF16>::IMG, halfwords per operand image
constexpr int F_IMG_BF16 = 3 * 128 * 32; // SplitCfg<SplitBf16>::IMG
constexpr int F_W1_WIMG = 4 * 128 * 32 * 2;   // W1_WIMG, bytes of one row tile's image
constexpr int F_RATIONALQUADRATIC = 4;   // GDRF_RATIONALQUADRATIC
// ---- constants only the host reads
constexpr int FWD_T_W1_KGP = 2;          // topic pairs per L2 group of the pair form: four S_k^T panels, ~2.6 MB at Mp = 512, as the quad form holds
constexpr size_t LDS_MAX = 160 * 1024;   // dynamic LDS of a workgroup
constexpr size_t LDS_ROWS = 150 * 1024;  // the budget of the row kernels, which keep static LDS beside it
constexpr size_t LDS_FORM = 64 * 1024;   // the budget under which the predictive forms keep their operands in LDS

// ---- form codes, one enum per named slot of gdrf_last_forms
enum WbarForm { WBAR_NONE = 0, WBAR_GEMM_NT, WBAR_GEMM_NT_T, WBAR_SPLIT1, WBAR_SPLIT2, WBAR_SPLIT_CC, WBAR_K64, WBAR_W1, WBAR_LAST = WBAR_W1 };
enum AkForm { AK_NONE = 0, AK_GEMM_TN, AK_TN_SPLIT, AK_TN_TOPICS, AK_W2, AK_LAST = AK_W2 };
enum FwdTForm { FWD_T_NONE = 0, FWD_T_GEMM_NT, FWD_T_Q4, FWD_T_CC, FWD_T_W1, FWD_T_LAST = FWD_T_W1 };
enum LocForm { LOC_NONE = 0, LOC_ROWS, LOC_GEMM_NT, LOC_GEMM_NT_WIDE, LOC_LAST = LOC_GEMM_NT_WIDE };
enum RowsForm { ROWS_NONE = 0, ROWS_MFMA, ROWS_THREAD, ROWS_STREAMED, ROWS_LAST = ROWS_STREAMED };
enum GtForm { GT_NONE = 0, GT_GEMM_TN, GT_TN_SPLIT, GT_LAST = GT_TN_SPLIT };
enum HyperForm { HYPER_NONE = 0, HYPER_F64, HYPER_TN, HYPER_LAST = HYPER_TN };
enum MmForm { MM_NONE = 0, MM_DIRECT, MM_SPLIT8, MM_LAST = MM_SPLIT8 };
enum PredictForm { PREDICT_NONE = 0, PREDICT_MFMA, PREDICT_ROWS_LDS, PREDICT_ROWS_MEM, PREDICT_ROWS_BIGK, PREDICT_STREAMED, PREDICT_LAST = PREDICT_STREAMED };

// what the rules read of a context and a call
struct FormShape {
  int64_t n = 0, n_cap = 0;      // rows of the call, of the context
  int M = 0, Mp = 0, K = 0, V = 0, D = 0;       // D: coordinates the covariance kernels see (embedded ones in a periodic context)
  int esz = 4, ssz = 8;          // element sizes: arrays, solve
  int split = 0;                 // 0 native MFMA, 1 bf16x6, 2 f16x3
  bool stored_t = false;         // T_k = W S_k kept for the backward
  int rows_form = 0;             // gdrf_set_rows_form
  bool csr = false;              // a CSR count matrix is bound
  int hyper_tn = 0, learn_z = 0, ard = 0, per = 0, kind = 0;   // what hyper_tn_on reads
  int nsplit_cap = 0;            // splits the slab buffer has room for (nsplit_cap_rule)
  int64_t erows_grid_cap = 1024; // workgroups the LDS row forms' Phi-bar partials have room for
  int predict_mode = 0;          // gdrf_predict's mode
  bool unwhitened = false;       // the guide's u in the unwhitened form: Sbar chained through L^-T on the main stream

  int nt() const { return (Mp + F_TILE - 1) / F_TILE; }          // 128-wide tiles over Mp
  int64_t rtiles() const { return (n + F_TILE - 1) / F_TILE; }   // 128-row tiles of the call
  int64_t ldk() const { return (n_cap + 3) / 4 * 4; }            // leading dimension of the (K, n) arrays
  int nct_solve() const { const int cw = ssz == 4 ? 128 : 64; return (Mp + cw - 1) / cw; }   // column tiles of the NT core in the solve precision
  int tn_br() const { return 128 / esz; }                        // TNCfg<T>::BR, rows per chunk of the TN core
};

inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// row blocks of the ubar partial kernel: ~1024 workgroups, multiples of its 256-row staging step
inline int64_t ubar_rows_per_block(int64_t n) { return std::max<int64_t>(256, round_up((n + 1023) / 1024, 256)); }

// number of row splits of the TN kernels: fill the chip's resident-workgroup slots (256 CUs x 3) with as
// little last-round idling as possible, keep >= 8 chunks per split, cap the slab memory
inline int tn_nsplit(int K, int nt, int64_t n, int BR, int wg_per_cu = 3) {
  const int tiles = K * nt * (nt + 1) / 2;
  const double slots = 256.0 * wg_per_cu;
  int64_t maxs = (n + 8 * BR - 1) / (8 * BR);
  if (maxs > 64) maxs = 64;
  if (maxs < 1) maxs = 1;
  int best = 1; double best_eff = 0;
  for (int ns = 1; ns <= maxs; ++ns) {
    const double rounds = tiles * (double)ns / slots;
    const double eff = rounds / std::ceil(rounds);
    if (eff > best_eff + 1e-9 || (eff > best_eff - 0.02 && rounds >= 2.0 && tiles * (double)best / slots < 2.0)) { best_eff = eff; best = ns; }
  }
  return best;
}

// Row splits of the G^T = W^T Wbar contraction on the bf16 TN kernel.  Its nt*nt tiles are few, so the split count decides both the
// fill and the block -> XCD map: with a multiple of 8 every XCD owns whole row slabs and the 16 tiles of a slab share their W / Wbar
// panels through that XCD's L2 (measured at N = 1e6, M = 512: 18.8 -> 8.2 GB fetched, 4.46 -> 3.22 ms at 64 splits).
inline int tn_nsplit_gt(int K, int nt, int64_t n, int BR) {
  int64_t maxs = (n + 8 * BR - 1) / (8 * BR);
  if (maxs > 64) maxs = 64;
  if (maxs < 8) return tn_nsplit(K, nt, n, BR, 2);
  const int tiles = nt * nt;
  int best = 8; double best_eff = 0;
  for (int ns = 8; ns <= maxs; ns += 8) {
    const double rounds = tiles * (double)ns / 512.0;
    const double eff = rounds / std::ceil(rounds);
    if (eff > best_eff + 1e-9 || (eff > best_eff - 0.02 && rounds >= 2.0 && tiles * (double)best / 512.0 < 2.0)) { best_eff = eff; best = ns; }
  }
  return best;
}

// tiles (I, J) of the all-topics A_k kernels: 128-column block I of the rows i, 64-column block J <= 2 I + 1 of the columns j
// (tnt_ntiles of gemm_tn_topics.h, which the launch itself still calls)
inline int tnt_tiles(int ncols) {
  const int nI = (ncols + 127) / 128, nJ = (ncols + 63) / 64;
  int t = 0;
  for (int I = 0; I < nI; ++I) t += (2 * I + 2 < nJ ? 2 * I + 2 : nJ);
  return t;
}

// Row splits of the all-topics A_k kernel (gemm_tn_topics.h): one 512-thread workgroup per CU, tiles x topic groups x splits
// workgroups; fill the 256 CUs' rounds, >= 16 chunks per split, at most 64 splits
inline int tn_topics_nsplit(int K, int Mp, int64_t n) {
  const int units = tnt_tiles(Mp) * ((K + F_TNT_KT - 1) / F_TNT_KT);
  int64_t maxs = (n + 16 * 32 - 1) / (16 * 32);
  if (maxs > 64) maxs = 64;
  if (maxs < 1) maxs = 1;
  // cost model (relative units): rounds of one workgroup per CU, each walking n / ns rows, plus the slab traffic that grows with ns (K Mp^2
  // floats written and read per split: 0.13 ms at 64 splits, M = 512, K = 10 - a fixed cost that does not shrink with a rank's share
  // of the rows; at the 8-GPU per-rank size of the headline workload the optimum moves from 64 to ~25 splits)
  const double chunk_us = 3.7;                                   // one 32-row chunk of a (tile, topic group) unit: 9.0 ms at N = 1e6, M = 512, K = 10
  const double slab_us_per_split = 2.0 * (double)K * Mp * Mp * 4.0 / 5.0e6;       // bytes at ~5 TB/s, in us
  int best = 1; double best_t = 1e300;
  for (int ns = 1; ns <= maxs; ++ns) {
    const double rounds = std::ceil(units * (double)ns / 256.0);
    const double t = rounds * std::ceil((double)n / (32.0 * ns)) * chunk_us + ns * slab_us_per_split;
    if (t < best_t * 0.995) { best_t = t; best = ns; }
  }
  return best;
}

// splits the slab buffer of a context is sized for (gdrf_ctx_create_ex)
inline int nsplit_cap_rule(int K, int Mp, int64_t n_cap, int esz) {
  const int nt = (Mp + F_TILE - 1) / F_TILE;
  int cap = tn_nsplit(K, nt, n_cap, 128 / esz);
  if (esz == 4) cap = std::max({cap, tn_nsplit(K, nt, n_cap, 32, 2), tn_nsplit_gt(K, nt, n_cap, 32), 64});   // the split TN forms run 2 workgroups per CU; the all-topics form up to 64 splits
  return cap;
}

// K_nm parts of the hyper-parameter gradients through Hd = dK^T Wbar on the split-fp16 TN kernel (hyper_tn.h): f16x3 contexts with the f64
// solve, fixed inducing inputs (their gradient needs Kbar itself), kernels whose only shape parameter is the lengthscale
inline bool hyper_tn_on(const FormShape& f) {
  return f.hyper_tn && f.split == 2 && f.ssz == 8 && !f.learn_z && !f.ard && !f.per && f.kind != F_RATIONALQUADRATIC && !f.stored_t && (f.Mp / 8) <= 256;
}

// the gate of the one-wave-per-SIMD forms of W-bar and tt (f16x3): many rows (no reduction slices), Mp in whole 64-deep blocks, at most 16 topics
inline bool w1_gate(const FormShape& f) {
  const int64_t pairs = (f.rtiles() + 1) / 2;
  return (f.Mp % 64) == 0 && f.K >= 2 && f.K <= 16 && pairs * f.nt() > 32;
}

// the K x 128 table of row factors of a wave group of the split W-bar forms; the k64 form's LDS: eight f16x3 images, two tables
inline size_t wbar_tab_bytes(int K) { return ((size_t)K * F_TILE * sizeof(float) + 15) & ~(size_t)15; }
inline size_t wbar_k64_lds(int K) { return 8 * (size_t)F_IMG_F16 * 2 + 2 * wbar_tab_bytes(K); }
// ---- W-bar.  grid / threads / lds: the split forms only (forms 1 and 2 launch on the NT core's own geometry)
struct WbarPlan { WbarForm form; int nslice, R; unsigned grid; int threads; size_t lds; bool fits; };
inline WbarPlan wbar_plan(const FormShape& f) {
  WbarPlan p{WBAR_NONE, 1, 0, 0, 0, 0, true};
  if (f.stored_t) { p.form = WBAR_GEMM_NT_T; return p; }
  if (!f.split) { p.form = WBAR_GEMM_NT; return p; }
  const int Mp = f.Mp, K = f.K, nct = f.nt();
  const bool f16 = f.split == 2;
  const size_t img = f16 ? F_IMG_F16 : F_IMG_BF16;                  // halfwords per operand image
  const size_t tabb = wbar_tab_bytes(K);
  const size_t grp = 2 * img * 2 + tabb;                            // one wave group: A and B images, its table
  const int64_t rtiles = f.rtiles(), pairs = (rtiles + 1) / 2;
  if (K >= 2 && 2 * grp <= LDS_MAX) {   // two phase-shifted wave groups per workgroup (own A images, shared double-buffered B, LDS-DMA staging)
    const size_t lds_cc = 6 * img * 2 + 2 * tabb;
    p.grid = (unsigned)round_up(pairs * nct, 8); p.threads = 512;
    if (f16 && (Mp % 64) == 0 && wbar_k64_lds(K) <= LDS_MAX) {
      if (w1_gate(f)) {
        // many rows (no slices) and at most 16 topics: one wave per SIMD, B_k fragments straight from L2 into registers
        p.form = WBAR_W1; p.threads = 256;
        p.lds = 8 * img * 2 + 2 * (size_t)(K + 1) * F_TILE * sizeof(float);
        p.R = K >= 8 ? 2 : (K >= 4 ? 4 : 8);       // W-image requests per wave and phase: the 16 of a block fit into its K phases
        return p;
      }
      // few rows (streaming mini-batches): a handful of workgroups would each walk all K x Mp / 64 chunks one after the other
      // (0.19 ms at n = 64); the reduction blocks are split over gridDim.y slices into slabs, summed in a fixed order
      const int nkb = Mp / 64;
      if (pairs * nct <= 32 && nkb >= 2) p.nslice = std::min(nkb, 8);
      if ((size_t)p.nslice * round_up(f.n, 256) * Mp > (size_t)f.nsplit_cap * (K + 1) * Mp * Mp) p.nslice = 1;   // the TN slab buffer is idle now
      p.form = WBAR_K64; p.lds = wbar_k64_lds(K);
    } else if (lds_cc <= LDS_MAX) {
      p.form = WBAR_SPLIT_CC; p.lds = lds_cc;
    } else {
      p.form = WBAR_SPLIT2; p.lds = std::max<size_t>(2 * grp, 8 * 32 * 68 * sizeof(float));      // the epilogue's transposition tiles
    }
  } else {
    p.form = WBAR_SPLIT1; p.fits = grp <= LDS_MAX;
    p.lds = std::max<size_t>(grp, 4 * 32 * 68 * sizeof(float));
    p.grid = (unsigned)round_up(rtiles * nct, 8); p.threads = 256;
  }
  return p;
}

// ---- tt.  Forms 2 and 3: grid / threads / lds.  Form 4: K / 4 * 4 topics on the quad geometry (one row tile, four topics per workgroup: half
// the W traffic per topic), the K % 4 left over on the pair geometry (two row tiles, two topics), in L2 groups of KGP pairs whose workgroups
// share the W blocks they stream
struct FwdTPlan { FwdTForm form; int KG, rt8; unsigned grid; int threads, lds; int KQ, KP, KGP, rt8_q; unsigned grid_q, grid_p; int lds_q, lds_p; };
inline FwdTPlan fwd_t_tiled_plan(const FormShape& f) {      // forms 2 and 3, whatever the gate of form 4 says (tools/fwd_t_kernel_time.hip times both)
  FwdTPlan p{};
  const int Mp = f.Mp, K = f.K, NP = f.split == 2 ? 2 : 3, img = NP == 2 ? F_IMG_F16 : F_IMG_BF16;
  // topics per group: as many lower-triangular S^T piece panels (NP x ~0.6 Mp^2 halfwords each) as fit in 2 MB
  const double panel = 0.625 * 2.0 * NP * (double)Mp * Mp;
  p.KG = std::max(1, std::min(K, (int)(2.0 * 1024 * 1024 / panel)));
  // two row tiles per 512-thread workgroup (two phase-shifted wave groups, LDS-DMA staging): 6 operand images
  const int64_t pairs = (f.rtiles() + 1) / 2;
  p.rt8 = (int)((pairs + 7) / 8);
  p.grid = (unsigned)(8 * K * p.rt8);
  if (NP == 2) {       // 256 x 256 workgroup tiles (two-piece modes: eight operand images in 128 KB)
    p.form = FWD_T_Q4; p.threads = 1024; p.lds = 8 * img * 2 + 8 * F_TILE * 4;      // + the row-sum slots
  } else {
    p.form = FWD_T_CC; p.threads = 512; p.lds = 6 * img * 2;
  }
  return p;
}
inline FwdTPlan fwd_t_plan(const FormShape& f) {
  if (!f.split) { FwdTPlan p{}; p.form = FWD_T_GEMM_NT; return p; }
  FwdTPlan p = fwd_t_tiled_plan(f);
  if (f.split == 2 && w1_gate(f)) {      // one wave per SIMD, S_k^T fragments straight from L2 into registers
    const int K = f.K;
    p.form = FWD_T_W1; p.threads = 256;
    p.KQ = K / 4 * 4; p.KP = (K - p.KQ + 1) / 2; p.KGP = std::min(p.KP, FWD_T_W1_KGP);
    p.rt8_q = (int)((f.rtiles() + 7) / 8);
    p.grid_q = (unsigned)(8 * (p.KQ / 4) * p.rt8_q); p.lds_q = 2 * F_W1_WIMG + 16 * F_TILE * 4;             // + the row-sum slots
    p.grid_p = (unsigned)(8 * p.KP * p.rt8); p.lds_p = 4 * F_W1_WIMG + 16 * F_TILE * 4;
    p.KG = p.KQ ? 4 : 2 * p.KGP;
  }
  return p;
}

// ---- A_k.  ns / rps: the tiled TN kernels (forms 1, 2); nst / rpst: form 3; ns1 / rps1: form 4; red_ns / red_qd: what reduce_slabs sums
struct AkPlan { AkForm form; int kgroups, ns; int64_t rps; int nst; int64_t rpst; int ns1; int64_t rps1; int red_ns, red_qd; };
inline AkPlan ak_plan(const FormShape& f) {
  AkPlan p{};
  const int K = f.K, BR = f.tn_br();
  const int64_t n = f.n;
  p.ns = std::min(tn_nsplit(K, f.nt(), n, BR, f.split ? 2 : 3), f.nsplit_cap);
  p.rps = round_up((n + p.ns - 1) / p.ns, BR);
  p.red_ns = p.ns; p.red_qd = F_TILE / 2;
  if (f.split == 2) {
    p.nst = std::min(tn_topics_nsplit(K, f.Mp, n), f.nsplit_cap);
    p.rpst = round_up((n + p.nst - 1) / p.nst, 32);
    p.kgroups = (K + F_TNT_KT - 1) / F_TNT_KT;
    // The one-wave forms run every stage of their 10-topic groups whatever K: with more than 40 % of the topic slots empty (K <= 5, K = 11)
    // the two-wave form, which walks the topic pairs that exist, is the faster one.
    if (10 * K >= 6 * p.kgroups * F_TNT_KT) {      // one-wave-per-SIMD form (gemm_tn_topics1.h): 128 rows per wave
      p.form = AK_W2;
      int ns1 = f.nsplit_cap < 64 ? f.nsplit_cap : 64;                            // 8 k splits: every XCD owns whole splits
      while (ns1 > 8 && (n + ns1 - 1) / ns1 < 8 * F_TN1_CH) ns1 -= 8;             // at least 8 chunks per split
      if (ns1 >= 8) ns1 &= ~7;
      p.ns1 = ns1; p.rps1 = round_up((n + ns1 - 1) / ns1, F_TN1_CH);
      p.red_ns = ns1;
    } else {
      p.form = AK_TN_TOPICS; p.red_ns = p.nst;
    }
    p.red_qd = 32;
  } else {
    p.form = f.split ? AK_TN_SPLIT : AK_GEMM_TN;      // bf16x6 (f16x3 took the branch above)
  }
  return p;
}

// ---- G^T = W^T Wbar and the hyper-TN form's Hd = dK^T Wbar, both on nt x nt tiles
struct GtPlan { GtForm form; int ns; int64_t rps; };
inline GtPlan gt_plan(const FormShape& f) {
  const int BR = f.tn_br();
  const int ns = std::min(f.split ? tn_nsplit_gt(f.K, f.nt(), f.n, BR) : tn_nsplit(f.K, f.nt(), f.n, BR, 3), f.nsplit_cap);
  return {f.split ? GT_TN_SPLIT : GT_GEMM_TN, ns, round_up((f.n + ns - 1) / ns, BR)};
}
struct HyperPlan { HyperForm form; int ns; int64_t rps; };
inline HyperPlan hyper_plan(const FormShape& f) {
  if (!(f.esz == 4 && f.ssz == 8 && hyper_tn_on(f))) return {HYPER_F64, 0, 0};
  const int BR = f.tn_br();
  const int ns = std::min(tn_nsplit_gt(f.K, f.nt(), f.n, BR), f.nsplit_cap);
  return {HYPER_TN, ns, round_up((f.n + ns - 1) / ns, BR)};
}

// ---- loc = W U^T.  Form 1: a streaming pass over W for a handful of topics, U in LDS
struct LocPlan { LocForm form; int64_t blocks; size_t lds; };
inline LocPlan loc_plan(const FormShape& f) {
  const size_t ulds = (size_t)f.K * f.Mp * f.esz;
  if (f.K <= F_LOC_KMAX && f.Mp % (16 * (F_VEC / f.esz)) == 0 && ulds <= LDS_ROWS) return {LOC_ROWS, std::min<int64_t>((f.n + 31) / 32, 256 * 8), ulds};
  const bool wide = f.esz == 8 && f.K > 64;       // f64 with K > 64 (the NT core's 64-wide column tile): two column tiles
  return {wide ? LOC_GEMM_NT_WIDE : LOC_GEMM_NT, f.rtiles(), 0};
}

// ---- ubar = locbar W: topic quads per pass, rows per block, blocks
struct UbarPlan { int kq; int64_t rpb, nb; };
inline UbarPlan ubar_plan(const FormShape& f) {
  const int64_t rpb = ubar_rows_per_block(f.n);
  return {f.K <= 16 ? (f.K + 3) / 4 : 4, rpb, (f.n + rpb - 1) / rpb};
}

// ---- the row terms
// LDS bytes of elbo_rows_mfma (rows_mfma.h): scratch 128 | phiS K V | per wave: thT 16 x (16 NKT + 1), pbT 16 x (16 NVT + 1) | per wave Phi-bar slab K V
inline size_t rows_mfma_lds(int esz, int K, int V, int nkt, int nvt, int waves) {
  return 128 + ((size_t)K * V + (size_t)waves * (16 * (16 * nkt + 1) + 16 * (16 * nvt + 1)) + (size_t)waves * K * V) * esz;
}
// elbo_rows_mfma addresses the [topic][ldk] arrays (qpart as [chunk][ldk]) and eps ([topic][lde]) by a 32-bit BYTE offset from the row group's
// first row: the largest one it forms, row max(K, nqpart) - 1 plus at most 15 rows, must not wrap
inline bool rows_mfma_offsets_fit(int esz, int K, int nqpart, int64_t ldk, int64_t lde) {
  const uint64_t lim = (uint64_t)1 << 32, grp = 16 * (uint64_t)esz;
  const uint64_t top = (uint64_t)((K > nqpart ? K : nqpart) - 1);
  return top * (uint64_t)ldk * esz + grp < lim && (uint64_t)(K - 1) * (uint64_t)lde * esz + grp < lim;
}
struct RowsPlan { RowsForm form; int nkt, nvt, RB, threads; size_t lds; int egrid; bool kreg, fits; };   // kreg: the topics of a row in registers
inline RowsPlan rows_plan(const FormShape& f) {
  RowsPlan p{ROWS_NONE, 0, 0, 0, 0, 0, 0, false, true};
  const int K = f.K, V = f.V;
  if (f.rows_form == 1 || f.csr) { p.form = ROWS_STREAMED; return p; }
  // matrix-core form (rows_mfma.h): 16 rows per wave, the three K x V products of a row block as 16x16x4 matrix instructions on
  // register-resident operands; K <= 32, V <= 64 and 32-bit offsets.  The one-thread-per-row kernel serves the other sizes
  if (K <= 32 && V <= 64 && rows_mfma_offsets_fit(f.esz, K, f.nct_solve(), f.ldk(), f.n)) {
    p.form = ROWS_MFMA; p.nkt = K <= 16 ? 1 : 2; p.nvt = V <= 32 ? 2 : 4; p.threads = 256;
    p.lds = rows_mfma_lds(f.esz, K, V, p.nkt, p.nvt, 4);
    const int64_t groups = (f.n + 15) / 16;
    p.egrid = (int)std::min<int64_t>((groups + 3) / 4, f.erows_grid_cap);
    return p;
  }
  const bool kreg = K <= F_KMAX;
  auto lds_for = [&](int rb) { return 128 + ((size_t)2 * K * V + (size_t)rb * (K + 1) * (kreg ? 1 : 2) + (size_t)rb * (V + 1)) * f.esz; };
  int RB = 128;
  while (RB > 32 && lds_for(RB) > LDS_ROWS) RB >>= 1;
  p.form = ROWS_THREAD; p.kreg = kreg; p.RB = p.threads = RB; p.lds = lds_for(RB); p.fits = p.lds <= LDS_ROWS;
  p.egrid = (int)std::min<int64_t>((f.n + RB - 1) / RB, f.erows_grid_cap);
  return p;
}

// ---- the small M x M products (Impl::mm_nt).  A single product is 16 workgroups of the NT core (45 us at M = 512 in double, four of them in a
// row in every step's Cholesky backward): its reduction is split over 8 slices into the context's ONE slab buffer, which reduce_slabs adds
// in a fixed order.  A batch is launched directly (measured SLOWER split: 160 workgroups at K = 10 already fill most CUs and the slab sum
// of K matrices costs more than the split saves).  K = 1 makes every batched product a single one, and step_finish runs Sbar_k = 2 A_k S_k
// on the side stream BESIDE the Cholesky-backward chain: a product beside the chain never takes the slab the chain's products write
// (`beside_chain`: direct; it hides behind four dependent products).
constexpr int MM_S = 8;                  // slices of a split product
constexpr int mm_bk(int esz) { return 128 / esz; }                                        // NTCfg<E>::BK: 32 (f32) / 16 (f64)
inline int mm_tiles(int Mp, int esz) { const int cw = esz == 4 ? 128 : 64; return ((Mp + F_TILE - 1) / F_TILE) * ((Mp + cw - 1) / cw); }
inline size_t mm_slab_bytes(int Mp, int ssz) { return (size_t)MM_S * Mp * Mp * ssz; }   // [slices][Mp][Mp] in the solve precision
struct MmPlan { MmForm form; int S, kw; bool split() const { return form == MM_SPLIT8; } };      // S slices of kw reduction indices each; direct: 1, 0
inline MmPlan mm_plan(int Mp, int esz, int batch, int tiles, size_t slab_bytes, bool beside_chain) {
  const int kw = Mp / MM_S;
  if (!beside_chain && batch == 1 && tiles <= 256 && Mp >= 256 && Mp % MM_S == 0 && kw % mm_bk(esz) == 0 &&
      (size_t)MM_S * Mp * Mp * esz <= slab_bytes)
    return {MM_SPLIT8, MM_S, kw};
  return {MM_DIRECT, 1, 0};
}
// step_finish's two kinds of M x M product: the Cholesky-backward chain's single products in the solve precision, and Sbar_k = 2 A_k S_k in the
// arrays' (whitened: beside the chain, on the side stream; unwhitened: on the main stream, alone)
inline MmPlan mm_chain_plan(const FormShape& f) { return mm_plan(f.Mp, f.ssz, 1, mm_tiles(f.Mp, f.ssz), mm_slab_bytes(f.Mp, f.ssz), false); }
inline MmPlan mm_sbar_plan(const FormShape& f) { return mm_plan(f.Mp, f.esz, f.K, mm_tiles(f.Mp, f.esz), mm_slab_bytes(f.Mp, f.ssz), !f.unwhitened); }

// ---- gdrf_predict modes 0-3 (mode 4 runs the step's forward: no form of its own)
struct PredictPlan { PredictForm form; int NB; size_t lds; bool fits; };
inline PredictPlan predict_plan(const FormShape& f) {
  const int M = f.M, K = f.K, V = f.V, D = f.D;
  const size_t ts = f.ssz;
  if (f.predict_mode == 4) return {PREDICT_NONE, 0, 0, true};
  if (f.rows_form == 1 || (f.predict_mode == 3 && f.csr)) {
    const size_t lds = 128 + (size_t)M * D * ts;
    return {PREDICT_STREAMED, 0, lds, lds <= LDS_ROWS};
  }
  {
    // matrix-core form (predict.h): a wave owns 16 rows, one covariance value per lane and step is the A operand of the 16x16x4
    // matrix instruction, the padded transposed coefficients CfT its B operand.  K <= 32, the scaled inducing inputs in LDS.
    const int M4 = (int)round_up(M, 4), NB = K <= 16 ? 1 : 2, DDt = D <= 2 ? 2 : F_DMAX;
    const size_t lds = 128 + ((size_t)M4 * DDt + (size_t)K * V + (size_t)4 * 16 * (16 * NB + 1)) * ts;
    if (K <= 32 && lds <= LDS_FORM) return {PREDICT_MFMA, NB, lds, true};
  }
  if (K > F_KMAX) {
    const size_t lds = 128 + ((size_t)M * D + (size_t)K * V + (size_t)128 * (V + 1)) * ts;
    return {PREDICT_ROWS_BIGK, 0, lds, lds <= LDS_ROWS};
  }
  size_t lds = 128 + ((size_t)M * D + (size_t)K * V + (size_t)K * M) * ts;
  bool in_lds = true;
  if (lds > LDS_FORM) { in_lds = false; lds -= (size_t)K * M * ts; }
  return {in_lds ? PREDICT_ROWS_LDS : PREDICT_ROWS_MEM, 0, lds, lds <= LDS_ROWS};
}

// ---- gdrf_predict_quant, the quantile mode (predict_quant.h): a workgroup pass keeps the S samples of CP components of RP rows in LDS
//   theta [256 / LG][Kp] | samples [RP][CP (P + 1) + LG],  P = S rounded up to a power of two, Kp = K rounded up to whole lanes of the group
// within QUANT_LDS = 64 KB: two workgroups on a CU (two waves per SIMD, so one group's LDS latency in the ordering network hides behind
// the other's draws) with a quarter of the LDS left over.  The draws are regenerated for each of the ceil(C / CP) passes and a row's
// draws cost more than ordering all of its components, so the plan minimises the regenerated draws per row, ceil(C / CP) / RP, over
// RP = 1 .. 256 / LG with CP the most components that fit beside RP rows (at most C); equal cost: the larger RP, which keeps more
// groups busy in the ordering.  The comparison is in integers.  The largest unit (S = 1024 in double beside K = 128) is 12.5 KB: RP = 1, CP = 1
// always fits.
constexpr size_t QUANT_LDS = 64 * 1024;
struct QuantPlan { int RP, CP, P; size_t lds; };
inline QuantPlan quant_plan(int K, int C, int S, int esz, int LG) {
  const int RPB = 256 / LG, Kp = (K + LG - 1) / LG * LG;
  int P = 1;
  while (P < S) P <<= 1;
  const size_t theta = (size_t)RPB * Kp * esz;
  auto lds_for = [&](int rp, int cp) { return theta + (size_t)rp * ((size_t)cp * (P + 1) + LG) * esz; };
  QuantPlan best{0, 0, P, 0};
  int64_t best_passes = 0;
  for (int rp = 1; rp <= RPB; ++rp) {
    if (lds_for(rp, 1) > QUANT_LDS) break;
    const int64_t room = (int64_t)((QUANT_LDS - theta) / ((size_t)rp * esz)) - LG;      // elements a row may take
    const int cp = (int)std::min<int64_t>(C, room / (P + 1));
    const int64_t passes = (C + cp - 1) / cp;
    if (!best.RP || passes * best.RP <= best_passes * rp) { best.RP = rp; best.CP = cp; best_passes = passes; }
  }
  best.lds = lds_for(best.RP, best.CP);
  return best;
}

// ---- gdrf_predict_loo / gdrf_psis_rows (predict_loo.h): a workgroup pass keeps all S log likelihoods of RP rows in LDS, in double
//   rows [RP][P + M + 3 m] double | Phi chunk [K][W] (dense) | theta [RP][Kp] | counts [RP][W] int32 (dense)
// P = S rounded up to a power of two (what the ordering network takes), M = loo_tail_len(S) the tail the fit reads and m = 30 +
// floor(sqrt(M)) its grid: beside its P samples a row keeps the M exceedances (later the smoothed tail) and the grid's b_j, L_j, w_j.
// W = min(V, 128) (GDRF_SCORE_V_CHUNK), Kp = K rounded up to whole lanes of the group.  The stage kernel is K = 0, V = 0, csr.
// What the plan optimises: the rows in flight on a compute unit, RP x (workgroups resident there: those whose LDS fits LDS_MAX, and no
// more than the registers allow - LOO_WG_CU = 2 four-wave workgroups for the fused kernel at its ~200 VGPRs, LOO_STAGE_WG_CU = 3 for the
// stage kernel) - a row's samples weigh more than its share of anything else, and the ordering network is LDS latency that only other
// rows' work hides.  The product is maximised over RP = 1 .. 256 / LG with a workgroup's LDS within LDS_ROWS; equal products: the
// larger RP, which stages Phi less often and leaves fewer groups idle.  In integers.  The largest unit, K = 128 in double at S = 1024
// (Phi 128 KB, samples and fit 1024 + 96 + 117 doubles, theta 1 KB, counts 512 B): 142504 bytes at RP = 1, which fits.
constexpr int LOO_WG_CU = 2, LOO_STAGE_WG_CU = 3;
inline int loo_tail_len(int S) { return (int)std::ceil(std::min((double)S / 5.0, 3.0 * std::sqrt((double)S))); }
inline int loo_fit_grid(int M) { return 30 + (int)std::floor(std::sqrt((double)M)); }
struct LooPlan { int RP, P, M, stride; size_t lds; };      // stride: the doubles of a row
inline LooPlan loo_plan(int K, int V, int S, int esz, int LG, bool csr) {
  const int RPB = 256 / LG, Kp = (K + LG - 1) / LG * LG, W = std::min(V, 128);
  int P = 1;
  while (P < S) P <<= 1;
  const int M = loo_tail_len(S), stride = P + M + 3 * loo_fit_grid(M);
  const size_t fixed = csr ? 0 : (size_t)K * W * esz;
  const size_t row = (size_t)stride * sizeof(double) + (size_t)Kp * esz + (csr ? 0 : (size_t)W * sizeof(int32_t));
  LooPlan best{1, P, M, stride, fixed + row};
  int64_t best_rows = 0;
  for (int rp = 1; rp <= RPB; ++rp) {
    const size_t lds = fixed + rp * row;
    if (lds > LDS_ROWS) break;
    const int64_t rows = (int64_t)rp * std::min<int64_t>(K ? LOO_WG_CU : LOO_STAGE_WG_CU, (int64_t)(LDS_MAX / lds));
    if (rows >= best_rows) { best.RP = rp; best.lds = lds; best_rows = rows; }
  }
  return best;
}

}  // namespace forms
}  // namespace gdrf
