// libgdrf_hip: C-ABI entry points (include/gdrf_hip.h) and launch sequencing.  gfx950 only.
#include "../../include/gdrf_hip.h"
#include "common.h"
#include "gemm_nt.h"
#include "gemm_tn.h"
#include "gemm_split.h"
#include "gemm_tn_topics.h"
#include "gemm_tn_topics1.h"
#include "kernels_mm.h"
#include "kernels_n.h"
#include "predict.h"
#include "predict_mc.h"
#include "predict_info.h"
#include "predict_score.h"
#include "predict_quant.h"
#include "predict_loo.h"
#include "foldin.h"
#include "sample_counts.h"
#include "predict_cov.h"
#include "select_batch.h"
#include "select_inducing.h"
#include "rows_lds.h"
#include "rows_mfma.h"
#include "rows_vstream.h"
#include "rows_csr.h"
#include "hyper_tn.h"
#include "optim.h"
#include "forms.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

using namespace gdrf;
namespace F = gdrf::forms;

// forms.h restates the constants its rules share with the kernels: each one is tied to its original here
static_assert(F::F_TILE == GDRF_TILE && F::F_MPAD == GDRF_MPAD && F::F_DMAX == GDRF_DMAX && F::F_KMAX == GDRF_KMAX && F::F_LOC_KMAX == LOC_KMAX, "forms.h");
static_assert(F::F_TNT_KT == TNT_KT && F::F_TN1_CH == TN1_CH && F::F_W1_WIMG == W1_WIMG, "forms.h");
static_assert(F::F_IMG_F16 == SplitCfg<SplitF16>::IMG && F::F_IMG_BF16 == SplitCfg<SplitBf16>::IMG, "forms.h");
static_assert(F::F_VEC == sizeof(Vec16<float>::type) && F::F_VEC == sizeof(Vec16<double>::type), "forms.h");
static_assert(F::F_RATIONALQUADRATIC == GDRF_RATIONALQUADRATIC && 128 / sizeof(float) == TNCfg<float>::BR && 128 / sizeof(double) == TNCfg<double>::BR, "forms.h");
static_assert(NTCfg<float>::CW == 128 && NTCfg<double>::CW == 64, "forms.h: FormShape::nct_solve, loc_plan");
static_assert(F::WBAR_LAST == 7 && F::AK_LAST == 4 && F::FWD_T_LAST == 4 && F::LOC_LAST == 3 && F::ROWS_LAST == 3 && F::GT_LAST == 2 && F::HYPER_LAST == 2 &&
              F::PREDICT_LAST == 5 && F::MM_LAST == 2, "the form codes of include/gdrf_hip.h");
static_assert(F::mm_bk(4) == NTCfg<float>::BK && F::mm_bk(8) == NTCfg<double>::BK, "forms.h: mm_plan");

static thread_local std::string g_err;
static int fail(int code, const char* what, const char* detail) {
  g_err = std::string(what) + ": " + detail;
  return code;
}
#define HIPCHK(x)                                                             \
  do {                                                                        \
    hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess) return fail(-(int)e_ - 1000, #x, hipGetErrorString(e_)); \
  } while (0)
#define LAUNCHCHK(name)                                                       \
  do {                                                                        \
    hipError_t e_ = hipGetLastError();                                        \
    if (e_ != hipSuccess) return fail(-(int)e_ - 1000, name, hipGetErrorString(e_)); \
  } while (0)

#define GDRF_NSLOTS 16
// dtype of a context: N-side element type T / solve element type TS
//   GDRF_F32 (0): T = float, TS = double  (default fp32 mode: K-fold contractions on f32 MFMA, the ill-conditioned
//                 pieces -- K_uu, Cholesky, L^-1, the solve W = K_nm L^-T, its backward, the M x M epilogue -- in f64)
//   GDRF_F64 (1): T = TS = double
//   GDRF_F32_PURE (2): T = TS = float (everything in fp32, as the reference's .float() casts do; for A/B comparisons)
struct gdrf_ctx {
  int dev, M, Mp, K, V, D, dtype, kind;
  int64_t ncap, ldk;          // ldk = leading dimension of the (K, n) arrays
  size_t esz, ssz;            // element sizes: N side, solve side
  int nt;                     // 128-wide tiles over Mp
  int nsplit_cap;
  // solve precision, M x M (ld Mp)
  void *mmslab; size_t mmslab_bytes;    // split-K slabs of the small M x M products: [slices][batch][Mp][Mp]
  void *Kuu, *Lw, *Lo, *L, *LT, *Linv, *LinvT, *Dinv, *t0, *t1, *t2, *Cf, *CfT, *Zs, *GTs;      // Lo: the panel-wise factorisation's output (Lw is its work matrix)
  void *Knm;                  // [ncap][Mp] K_nm in the solve precision (forward A operand, backward epilogue)
  // probe (N-side precision) scratch, only when T != TS
  void *pK, *pL;
  // N-side precision
  void *S, *ST, *Bm, *Sbar, *phi, *Upad, *qpart;
  void *W, *Wbar, *q, *loc, *tt, *vbar, *locbar, *asum, *mu;
  void *g_loc, *g_tt, *g_qpart, *g_vbar, *g_locbar, *g_asum, *g_redT; double* g_redd;   // two-point evaluation (quirk Q3), allocated on first use
  const void* mean_g; int64_t mean_g_sk, mean_g_sn;
  void* dKh;                  // pieces of dK_nm / d log ls (hyper_tn.h), allocated on first use
  gdrf_allreduce_fn allreduce; void* allreduce_user;      // the caller's collective (gdrf_set_allreduce), or null
  int hyper_tn; double* hpart;   // K_nm parts of the hyper-parameter gradients through Hd = dK^T Wbar on the TN kernel (hyper_tn.h) instead of the f64 backward GEMM
  void* vbs = nullptr;        // vbar x block scale, zero-padded to a multiple of 64 rows (gemm_tn_topics1.h)
  void *Bh, *STh, *Wh;        // 16-bit pieces of B_k, S_k^T and W (f32 contexts; split-operand MFMA forms, gemm_split.h)
  int split;                  // 0: native f32 MFMA; 1: "bf16x6" (3 bf16 pieces, 6 products); 2: "f16x3" (2 fp16 pieces, 3 products, block scales)
  int wh_pieces;              // pieces Wh has room for
  float* ssc; unsigned* smx;  // block scales (SplitLay pairs) and the maxima they come from
  void *Tst;                  // T_k = W S_k kept for the backward, or nullptr (dense W B_k form instead)
  int64_t t_bs, t_ts;         // its per-topic / per-row-tile strides in elements
  void *slab, *ubar_part, *phibar_part;
  double *dpart, *dsmall;     // dsmall: [0..2] kuu sums, [8] ll_const scratch
  double *llpart;             // per-workgroup partials of the data constant (own buffer: it may be queued beside a step)
  int64_t dpart_len, ubar_blocks_cap, erows_grid_cap;
  double* alpha_dev; double lgam_const;
  Hyper *hyp, *hyp_probe; int* flag;        // flag[0]: solve factorisation failed; flag[8..16): probe levels failed; flag[16]: a reused factorisation's inputs changed (own
                                            // 64-byte line, written only by the compare kernel and by reuse_clear below: the side stream's memset of flag[0..8) never touches it)
  void* snap; int prefact_valid; double prefact_jitter;     // the inputs of a factorisation made ahead of its step (gdrf_factorize_mode)
  hipStream_t side;           // small, tail-heavy kernels run here beside the big GEMMs (fork/join with events)
  hipEvent_t ev_fork, ev_loc, ev_fork2, ev_join, ev_fact0, ev_fact;
  int fact_pending;           // a factorisation has been queued on the side stream: consumers wait for ev_fact
  const void* mean;           // borrowed (K, n) mean_function values for the next gdrf_step_local calls, or null (zero_mean)
  int64_t mean_sk, mean_sn;
  int unwhitened;             // whiten = False: u' = L^-1 u, S' = L^-1 S (solve-precision scratch below, allocated on demand)
  void *uS, *uSb, *uSc, *uU, *uUb, *Uw;
  int learn_z; double* zpart; // learnable inducing inputs: per-row-tile partial sums [ceil(ncap/128)][M][D]
  int ard; void* Zp; double* apart;   // ARD (gdrf_set_ard): scaled inducing inputs in the N-side precision (probe, gdrf_knm); per-block sums of d / d log ls_d
  // Periodic kernel (kernel_id GDRF_PERIODIC): D = 2 Dr embedded coordinates per raw input axis pair (kernels_mm.h: prep_hyper_per_kernel), np
  // log-periods (1 or Dr; 0 in other contexts), the embedded rows of the current call (Xe, xe_cap rows), the inducing phases t_d z_d (Zph)
  int per, Dr, np; void *Xe, *Zph; int64_t xe_cap;
  // Product kernel (kernel_id GDRF_PRODUCT, gdrf_set_product): a periodic context whose embedded coordinates come from a table of nf factors
  // {kind, axis count, lengthscale count, period count, axes[4]}; nls / nper: elements of its log-lengthscale and log-period segments (the
  // nf log-variances come first).  npair: the pair coordinates of a periodic or product context (Dr in a periodic one).
  int prod, nf, pfac[GDRF_DMAX][8], nls, nper, npair;
  int64_t mean_count;         // trainable mean_function parameters (gdrf_set_mean_params): elements of their segment, 0 = none
  double* opt_part; int64_t opt_part_cap;   // gdrf_optim_step: per-workgroup sums of squares of the clip_norm pass, allocated on first use
  int rows_form;              // gdrf_set_rows_form: 0 the LDS row forms, 1 the vocabulary-streamed form (rows_vstream.h)
  void *vs_tmp, *vs_part, *vs_cpart, *vs_rs;   // form 1, allocated on first use: (K, ldk) mubar / topic_probs, Phi-bar slots [vs_gcap][K*V],
  int64_t vs_gcap;                             // link-constant slots [vs_gcap][K], row sums of Phi and their reduced constants [2][K]
  // the sparse row form (rows_csr.h): the CSR count matrix bound with gdrf_bind_counts_csr (borrowed pointers; csr_crow = null: none) ...
  const int64_t *csr_crow, *csr_ccol, *csr_cperm; const int32_t *csr_col, *csr_val; int64_t csr_n, csr_nnz;
  int csr_fresh;                               // the binding's entry rows and segment table are still to be built
  // ... its scratch of fixed size, allocated on first use: Phi^T (V, Kp), theta (n_cap, K), the link constant per row (n_cap) and per
  // workgroup [1024][K], one Phi-bar slot (K, V) ...
  void *csr_phiT, *csr_thN, *csr_cn, *csr_cpart, *csr_slot;
  // ... and the arrays that grow with nnz: pbar and the row of every entry, the column segments' table and partial sums
  void *csr_pb, *csr_parts; int32_t *csr_erow, *csr_segcol; int64_t *csr_segoff; int64_t csr_cap;
  // the joint posterior (predict_cov.h), allocated on first use and grown with the call: W (jrows, Mp), R (jnp, jnp), the Cholesky work
  // matrix (jgnp, jgnp), T_k (K, jtrows, Mp), the sampler's V (jsk, Mp) and zeta (jzel elements), all in the solve precision; its failure flag
  void *jW, *jR, *jG, *jT, *jV, *jZ; int64_t jrows, jnp, jgnp, jtrows, jsk, jzel; int* jflag;
  int64_t jlast_n, jlast_sk;  // rows and (sample, topic) pairs of the gdrf_sample_joint whose W, R, V and zeta are still in place (0: none)
  // the batch choice (select_batch.h), allocated on first use and grown with the call: the candidates and the given rows in one array
  // (sX, sxrows rows), the factor columns c[k][t][row] (sC) and the conditional variances d[k][row] (sD) in the solve precision, the picked
  // flags (sTk); of fixed size: B = (w_p, b_k) with the pivot's history and variances behind it (sB), the pass's partials and the picks (sPg, sPi)
  void *sX, *sC, *sD, *sB; int* sTk; double* sPg; long long* sPi; int64_t sxrows, sc_el, sd_el, stk_el;
  std::vector<void*> allocs;
  // optional per-kernel HIP-event timing (gdrf_set_timing): events recorded on the launch stream
  int timing;
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> tev;   // (slot, (start, stop)) pending
  std::vector<hipEvent_t> ev_pool;
  double t_ms[GDRF_NSLOTS]; int64_t t_cnt[GDRF_NSLOTS];
  int forms[GDRF_NFORMS];     // gdrf_last_forms: the form each shape-dispatched stage launched last (host bookkeeping, GDRF_FORM_* of gdrf_hip.h)
  int quant_plan[3];          // gdrf_quant_last_plan: (RP, CP, LDS bytes) of the last gdrf_predict_quant launch
  int loo_plan[2];            // gdrf_loo_last_plan: (RP, LDS bytes) of the last gdrf_predict_loo / gdrf_psis_rows launch
};

struct ScopedTimer {
  gdrf_ctx* c; int slot; hipStream_t s; hipEvent_t e0, e1; bool on;
  ScopedTimer(gdrf_ctx* c_, int slot_, hipStream_t s_) : c(c_), slot(slot_), s(s_), on(c_->timing != 0) {
    if (!on) return;
    auto get = [&]() { hipEvent_t e; if (!c->ev_pool.empty()) { e = c->ev_pool.back(); c->ev_pool.pop_back(); } else (void)hipEventCreate(&e); return e; };
    e0 = get(); e1 = get();
    (void)hipEventRecord(e0, s);
  }
  ~ScopedTimer() {
    if (!on) return;
    (void)hipEventRecord(e1, s);
    c->tev.push_back({slot, {e0, e1}});
  }
};

const char* gdrf_last_error(void) { return g_err.c_str(); }
int gdrf_version(void) { return 1; }

// Flat parameter layout: three scalars at 0, 1, 2, then the segments below, each starting on a multiple of 4 elements.  Setters change it
// after creation (ard, nf, nls, nper, np, mean_count), so it is computed on demand.
struct ParamLay { int64_t uloc, phi, S, Z, ard, pls, per, mean, total; };
static ParamLay param_lay(const gdrf_ctx* c) {
  ParamLay l;
  l.uloc = 4;
  l.phi = round_up(l.uloc + (int64_t)c->K * c->M, 4);
  l.S = round_up(l.phi + (int64_t)c->K * c->V, 4);
  l.Z = round_up(l.S + (int64_t)c->K * c->M * c->M, 4);          // unconstrained inducing inputs (M, D)
  l.ard = round_up(l.Z + (int64_t)c->M * c->Dr, 4);              // ARD contexts only: the D log-lengthscales
  // periodic contexts only: the np log-periods, right behind them.  Product contexts: the nf factor log-variances at ard, then the nls
  // log-lengthscales (pls), then the nper log-periods (per)
  l.pls = l.ard + c->nf;
  l.per = c->prod ? l.pls + c->nls : l.ard + (c->ard ? c->Dr : 0);
  l.mean = c->prod ? round_up(l.per + c->nper, 4)
                   : (c->ard || c->per) ? round_up(l.per + c->np, 4) : l.ard;   // contexts with gdrf_set_mean_params only: mean_function parameters
  l.total = c->mean_count ? round_up(l.mean + c->mean_count, 4) : l.mean;
  return l;
}
// doubles of red_d: 8 scalars, the (M, D) inducing-input sums, in ARD contexts the D sums of d / d log ls_d over the rows, then the
// caller's sums of d elbo / d theta of the mean_function parameters (gdrf_set_mean_params)
// periodic and product contexts: D embedded-coordinate sums in place of the ARD ones, then the npair sums of d / d log p
static int64_t red_nd(const gdrf_ctx* c) {
  return 8 + (int64_t)c->M * c->D + ((c->ard || c->per) ? c->D : 0) + (c->per ? c->npair : 0) + c->mean_count;
}
static int64_t red_mean_off(const gdrf_ctx* c) { return red_nd(c) - c->mean_count; }
// layout of red_T: ubar (K, Mp), phibar (K, V), A_k (K, Mp, Mp), G^T (Mp, Mp), then the tail
struct RedLay { int64_t ubar, phibar, A, GT, tail, total; };
static RedLay red_lay(const gdrf_ctx* c) {
  const int64_t mm = (int64_t)c->Mp * c->Mp;
  RedLay l;
  l.ubar = 0;
  l.phibar = round_up((int64_t)c->K * c->Mp, 4);
  l.A = round_up(l.phibar + (int64_t)c->K * c->V, 4);
  l.GT = l.A + c->K * mm;
  l.tail = l.GT + mm;
  // tail: the doubles of red_d for the step's single all-reduce (gdrf_payload_pack): as they are in f64 contexts, four float
  // pieces each in f32 ones
  const int64_t nd = red_nd(c);
  l.total = l.tail + round_up(c->esz == 8 ? nd : 4 * nd, 4);
  return l;
}

int gdrf_param_layout(const gdrf_ctx* c, int64_t out[7]) {
  const ParamLay l = param_lay(c);
  out[0] = 0; out[1] = 1; out[2] = 2; out[3] = l.uloc; out[4] = l.phi; out[5] = l.S; out[6] = l.total;
  return 0;
}
int gdrf_red_layout(const gdrf_ctx* c, int64_t out[6]) {
  const RedLay l = red_lay(c);
  out[0] = l.ubar; out[1] = l.phibar; out[2] = l.A; out[3] = l.GT; out[4] = l.total;
  out[5] = red_nd(c);          // the doubles of red_d, in the order red_nd lists them
  return 0;
}
int gdrf_inducing_layout(const gdrf_ctx* c, int64_t out[2]) { out[0] = param_lay(c).Z; out[1] = (int64_t)c->M * c->Dr; return 0; }
int gdrf_ard_layout(const gdrf_ctx* c, int64_t out[2]) { out[0] = param_lay(c).ard; out[1] = c->ard ? c->Dr : 0; return 0; }
int gdrf_periodic_layout(const gdrf_ctx* c, int64_t out[2]) { out[0] = param_lay(c).per; out[1] = c->np; return 0; }
int gdrf_product_layout(const gdrf_ctx* c, int64_t out[6]) {
  const ParamLay l = param_lay(c);
  out[0] = l.ard; out[1] = c->nf; out[2] = l.pls; out[3] = c->nls; out[4] = l.per; out[5] = c->nper;
  return 0;
}
// the parameters a factorisation depends on beyond slots 0-3 and Z, contiguous from the ard offset: the ARD log-lengthscales and the
// log-periods of a periodic context, the three segments of a product one
static int snap_extra(const gdrf_ctx* c) { return c->prod ? c->nf + c->nls + c->nper : (c->ard ? c->Dr : 0) + c->np; }
// embedded coordinates the context's buffers hold: a product context's table may change until its first step
static int dcap(const gdrf_ctx* c) { return c->prod ? GDRF_DMAX : c->D; }
// The embedded-coordinate table (kernels_mm.h: CoordTab) with absolute parameter indices.  A periodic context is one Periodic factor over all
// its raw axes; a product context lists the sources of its Periodic factors (pairs), then those of its RBF factors, each in factor order.
static CoordTab coord_tab(const gdrf_ctx* c) {
  CoordTab t{};
  const ParamLay pl = param_lay(c);
  t.dr = c->Dr;
  if (!c->prod) {
    t.D = 2 * c->Dr; t.npair = t.nsrc = c->Dr; t.nvar = 1; t.var[0] = 1;
    for (int d = 0; d < c->Dr; ++d) {
      t.ax[d] = d;
      t.ls[d] = c->ard ? pl.ard + d : 0;
      t.per[d] = pl.per + (c->np > 1 ? d : 0);
    }
    return t;
  }
  int64_t lsb[GDRF_DMAX], pb[GDRF_DMAX], ol = pl.pls, op = pl.per;
  for (int f = 0; f < c->nf; ++f) {
    lsb[f] = ol; ol += c->pfac[f][2];
    pb[f] = op; op += c->pfac[f][3];
    t.var[f] = pl.ard + f;
  }
  t.nvar = c->nf;
  int j = 0;
  for (int pass = 0; pass < 2; ++pass)
    for (int f = 0; f < c->nf; ++f) {
      const int* fa = c->pfac[f];
      if ((fa[0] == GDRF_PERIODIC) != (pass == 0)) continue;
      for (int k = 0; k < fa[1]; ++k, ++j) {
        t.ax[j] = fa[4 + k];
        t.ls[j] = lsb[f] + (fa[2] > 1 ? k : 0);
        if (pass == 0) t.per[j] = pb[f] + (fa[3] > 1 ? k : 0);
      }
      if (pass == 0) t.npair = j;
    }
  t.nsrc = j;
  t.D = 2 * t.npair + (t.nsrc - t.npair);
  return t;
}
// the covariance forms of the forward and predictive paths: ARD scales on the rows (a periodic context's embedding carries its own)
static bool ard_fwd(const gdrf_ctx* c) { return c->ard && !c->per; }
int gdrf_mean_param_layout(const gdrf_ctx* c, int64_t out[2]) { out[0] = param_lay(c).mean; out[1] = c->mean_count; return 0; }

// What the planning rules of forms.h read of the context, for a call on n rows
static F::FormShape form_shape(const gdrf_ctx* c, int64_t n, int predict_mode = 0) {
  F::FormShape f;
  f.n = n; f.n_cap = c->ncap; f.M = c->M; f.Mp = c->Mp; f.K = c->K; f.V = c->V; f.D = c->D;
  f.esz = (int)c->esz; f.ssz = (int)c->ssz; f.split = c->split; f.stored_t = c->Tst != nullptr;
  f.rows_form = c->rows_form; f.csr = c->csr_crow != nullptr;
  f.hyper_tn = c->hyper_tn; f.learn_z = c->learn_z; f.ard = c->ard; f.per = c->per; f.kind = c->kind;
  f.nsplit_cap = c->nsplit_cap; f.erows_grid_cap = c->erows_grid_cap; f.predict_mode = predict_mode; f.unwhitened = c->unwhitened;
  return f;
}
static bool hyper_tn_on(const gdrf_ctx* c) { return F::hyper_tn_on(form_shape(c, 0)); }

// Device memory the context owns until gdrf_ctx_destroy.  A block that a later call replaces (Wh, Xe, opt_part) stays owned as well: queued
// work may still read it.  `what` labels the error of a failed allocation.
template <typename P>
static int ctx_alloc(gdrf_ctx* c, P** p, size_t bytes, const char* what, bool zero = false) {
  void* q = nullptr;
  hipError_t e = hipMalloc(&q, bytes);
  if (e != hipSuccess) return fail(-(int)e - 1000, what, hipGetErrorString(e));
  c->allocs.push_back(q);
  if (zero) HIPCHK(hipMemset(q, 0, bytes));
  *p = (P*)q;
  return 0;
}

int gdrf_ctx_create(gdrf_ctx** out, int device, int64_t n_cap, int M, int K, int V, int D, int dtype, int kernel_id) {
  return gdrf_ctx_create_ex(out, device, n_cap, M, K, V, D, dtype, kernel_id, GDRF_STORE_T_OFF);
}

int gdrf_ctx_create_ex(gdrf_ctx** out, int device, int64_t n_cap, int M, int K, int V, int D, int dtype, int kernel_id, int store_t) {
  if (!out || n_cap < 1 || M < 1 || K < 1 || V < 1 || D < 1) return fail(-1, "gdrf_ctx_create", "bad size");
  if (K > GDRF_TILE) return fail(-1, "gdrf_ctx_create", "num_topic_categories > 128 not supported (loc = W U^T runs as one 128-wide column tile)");
  if (D > GDRF_DMAX) return fail(-1, "gdrf_ctx_create", "more than 4 input dimensions not supported");
  if (dtype != GDRF_F32 && dtype != GDRF_F64 && dtype != GDRF_F32_PURE) return fail(-1, "gdrf_ctx_create", "dtype");
  if (kernel_id < GDRF_RBF || kernel_id > GDRF_PRODUCT) return fail(-1, "gdrf_ctx_create", "kernel_id");
  if (kernel_id == GDRF_PERIODIC && 2 * D > GDRF_DMAX) return fail(-1, "gdrf_ctx_create", "the Periodic kernel supports at most 2 input dimensions");
  const int Dr = D;
  if (kernel_id == GDRF_PERIODIC) D = 2 * D;       // the embedded coordinates (cos, sin) of every raw axis
  if (kernel_id == GDRF_PRODUCT) D = GDRF_DMAX;    // buffers for any table; the default table is one RBF factor over every axis
  HIPCHK(hipSetDevice(device));
  gdrf_ctx* c = new gdrf_ctx();       // value-initialised (no user-provided constructor): every member not set below is zero / null / empty
  c->dev = device; c->M = M; c->Mp = (int)round_up(M, GDRF_MPAD); c->K = K; c->V = V; c->D = D; c->Dr = Dr;
  c->per = kernel_id == GDRF_PERIODIC || kernel_id == GDRF_PRODUCT; c->np = kernel_id == GDRF_PERIODIC ? 1 : 0;
  c->prod = kernel_id == GDRF_PRODUCT; c->npair = kernel_id == GDRF_PERIODIC ? Dr : 0;
  if (c->prod) {
    c->nf = 1; c->nls = 1; c->D = Dr;
    c->pfac[0][0] = GDRF_RBF; c->pfac[0][1] = Dr; c->pfac[0][2] = 1;
    for (int d = 0; d < Dr; ++d) c->pfac[0][4 + d] = d;
  }
  c->dtype = dtype; c->kind = c->per ? GDRF_RBF : kernel_id; c->ncap = n_cap; c->ldk = round_up(n_cap, 4);   // periodic: the RBF forms, embedded
  c->esz = dtype == GDRF_F64 ? 8 : 4;
  c->ssz = dtype == GDRF_F32_PURE ? 4 : 8;
  c->nt = (c->Mp + GDRF_TILE - 1) / GDRF_TILE;
  const size_t mm = (size_t)c->Mp * c->Mp * c->esz, mms = (size_t)c->Mp * c->Mp * c->ssz;
  auto A = [&](auto** p, size_t bytes) { return ctx_alloc(c, p, bytes ? bytes : 16, "hipMalloc"); };
#define AL(ptr, bytes) if (int rc = A(&(ptr), (bytes))) { gdrf_ctx_destroy(c); return rc; }
  AL(c->Kuu, mms) AL(c->Lw, mms) AL(c->Lo, mms)
  c->mmslab_bytes = F::mm_slab_bytes(c->Mp, (int)c->ssz);
  AL(c->snap, (size_t)(4 + (size_t)c->M * D + (c->prod ? 3 : 1) * GDRF_DMAX) * c->esz)
  AL(c->mmslab, c->mmslab_bytes) AL(c->L, mms) AL(c->LT, mms) AL(c->Linv, mms) AL(c->LinvT, mms)
  AL(c->Dinv, (size_t)(c->Mp / 32) * 1024 * c->ssz)
  AL(c->t0, mms) AL(c->t1, mms) AL(c->t2, mms) AL(c->GTs, mms)
  AL(c->Cf, (size_t)K * M * c->ssz) AL(c->CfT, (size_t)c->Mp * 32 * c->ssz) AL(c->Zs, (size_t)c->Mp * D * c->ssz)
  AL(c->Knm, (size_t)n_cap * c->Mp * c->ssz)
  AL(c->pK, mm) AL(c->pL, mm * 8)          // probe scratch: K_uu without jitter, 8 level copies
  AL(c->S, mm * K) AL(c->ST, mm * K) AL(c->Bm, mm * K) AL(c->Sbar, mm * K)
  if (c->esz == 4) { AL(c->Bh, (size_t)3 * K * c->Mp * c->Mp * 2) AL(c->STh, (size_t)3 * K * c->Mp * c->Mp * 2) }
  if (c->esz == 4) { AL(c->vbs, (size_t)K * round_up(n_cap, 64) * sizeof(float)) }
  AL(c->phi, (size_t)K * V * c->esz)
  AL(c->Upad, (size_t)GDRF_TILE * c->Mp * c->esz) AL(c->qpart, (size_t)((c->Mp + 63) / 64) * c->ldk * c->esz)
  AL(c->W, (size_t)n_cap * c->Mp * c->esz) AL(c->Wbar, (size_t)n_cap * c->Mp * c->esz)
  AL(c->q, (size_t)c->ldk * c->esz) AL(c->asum, (size_t)c->ldk * c->esz)
  AL(c->loc, (size_t)K * c->ldk * c->esz) AL(c->tt, (size_t)K * c->ldk * c->esz) AL(c->vbar, (size_t)K * c->ldk * c->esz)
  AL(c->locbar, (size_t)K * c->ldk * c->esz) AL(c->mu, (size_t)K * c->ldk * c->esz)
  {
    // GDRF_STORE_T_AUTO would keep T_k when it fits comfortably (<= 64 GB and <= 40 % of the free HBM); measured on
    // MI355X the stored-T form is currently SLOWER (47 vs 43 ms at the headline size: its A operand is a cold HBM
    // stream on every chunk and the register prefetch is drained by vmcnt(0) waits), so AUTO resolves to OFF.
    c->t_ts = (int64_t)GDRF_TILE * c->Mp + 1536;                                   // + 6 KB (f32): not a power of two
    c->t_bs = c->t_ts * ((n_cap + GDRF_TILE - 1) / GDRF_TILE) + 40960 + 512;
    const size_t tbytes = (size_t)K * c->t_bs * c->esz;
    if (store_t == GDRF_STORE_T_ON) { AL(c->Tst, tbytes) }
  }
  c->nsplit_cap = F::nsplit_cap_rule(K, c->Mp, n_cap, (int)c->esz);
  AL(c->slab, (size_t)c->nsplit_cap * (K + 2) * mm)          // K batches of A_k, one of G^T, one of Hd = dK^T Wbar
  AL(c->hpart, (size_t)std::max(4096, c->Mp + 2048) * sizeof(double))
  c->ubar_blocks_cap = std::min<int64_t>(1025, (n_cap + 255) / 256);     // upper bound of ubar_blocks(n) over n <= n_cap
  AL(c->ubar_part, (size_t)c->ubar_blocks_cap * K * c->Mp * c->esz)
  c->erows_grid_cap = 1024;          // phibar_part ([erows_grid_cap][K*V]) is allocated by the first LDS-form row kernel that writes it
  const int64_t rtiles = (n_cap + GDRF_TILE - 1) / GDRF_TILE;
  // users: bwd_knm 3 per workgroup, kuu_bar_reduce 3 per inducing point, elbo_rows 4 per workgroup, predict / ll_const <= 2 x 2048
  c->dpart_len = std::max<int64_t>({((rtiles + 8) * ((c->Mp + 63) / 64) + 16) * 3, (int64_t)3 * c->Mp + 16, 4 * c->erows_grid_cap, (int64_t)8192});
  AL(c->dpart, (size_t)c->dpart_len * sizeof(double))
  AL(c->dsmall, 16 * sizeof(double))
  AL(c->llpart, 2048 * sizeof(double))
  AL(c->alpha_dev, (size_t)K * V * sizeof(double))
  AL(c->hyp, sizeof(HyperPer)) AL(c->hyp_probe, sizeof(HyperPer)) AL(c->flag, 128)
  if (c->per) {
    // apart: D coordinate sums and npair period sums per backward workgroup or per inducing point
    const int npc = c->prod ? GDRF_DMAX / 2 : Dr;
    AL(c->Xe, (size_t)n_cap * D * c->esz) AL(c->Zp, (size_t)c->Mp * D * c->esz) AL(c->Zph, (size_t)c->Mp * npc * c->ssz)
    AL(c->apart, (size_t)c->dpart_len * (D + npc) * sizeof(double))
    c->xe_cap = n_cap;
  }
  AL(c->ssc, (size_t)SplitLay{K}.nfloats() * sizeof(float)) AL(c->smx, (size_t)SplitLay{K}.nmax() * sizeof(unsigned))
#undef AL
  {
    // the side stream carries the factorisation chain (small launches the step's first GEMM waits for): highest priority, so that its
    // workgroups are placed ahead of the K_nm kernel's 16 384 on the main stream
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least) {
      HIPCHK(hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, greatest));
    } else {
      HIPCHK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
    }
  }
  for (hipEvent_t* e : {&c->ev_fork, &c->ev_loc, &c->ev_fork2, &c->ev_join, &c->ev_fact0, &c->ev_fact})
    HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
  HIPCHK(hipMemset(c->flag, 0, 128));
  HIPCHK(hipMemset(c->W, 0, (size_t)n_cap * c->Mp * c->esz));
  std::vector<double> a((size_t)K * V, 1.0);
  *out = c;
  return gdrf_set_dirichlet(c, a.data());
}

void gdrf_ctx_destroy(gdrf_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->dev);
  for (void* p : c->allocs) (void)hipFree(p);
  for (auto& t : c->tev) { (void)hipEventDestroy(t.second.first); (void)hipEventDestroy(t.second.second); }
  for (auto e : c->ev_pool) (void)hipEventDestroy(e);
  for (hipEvent_t e : {c->ev_fork, c->ev_loc, c->ev_fork2, c->ev_join, c->ev_fact0, c->ev_fact}) if (e) (void)hipEventDestroy(e);
  if (c->side) (void)hipStreamDestroy(c->side);
  delete c;
}

int gdrf_set_dirichlet(gdrf_ctx* c, const double* alpha) {
  HIPCHK(hipSetDevice(c->dev));
  double lg = 0;
  for (int k = 0; k < c->K; ++k) {
    double s = 0;
    for (int v = 0; v < c->V; ++v) {
      const double a = alpha[(size_t)k * c->V + v];
      if (!(a > 0)) return fail(-1, "gdrf_set_dirichlet", "b must be positive");
      s += a; lg -= std::lgamma(a);
    }
    lg += std::lgamma(s);
  }
  c->lgam_const = lg;
  HIPCHK(hipMemcpy(c->alpha_dev, alpha, (size_t)c->K * c->V * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

// which = 0 W, 1 Wbar, 2 q, 3 loc, 4 tt, 5 vbar, 6 locbar, 7 asum, 8 Kuu, 9 L, 10 Linv, 11 S, 12 B, 13 phi, 14 mu, 15 LinvT, 16 ST, 17 Knm (solve precision),
// 18 the guide-side locbar of gdrf_step_local2 (0 elements before its first call)
static int ws_lookup(gdrf_ctx* c, int which, void** ptr, int64_t* nelem, int* esz) {
  const int64_t mm = (int64_t)c->Mp * c->Mp, kn = (int64_t)c->K * c->ldk;
  void* p = nullptr; int64_t n = 0; int e = (int)c->esz;
  switch (which) {
    case 0: p = c->W; n = c->ncap * c->Mp; break;     case 1: p = c->Wbar; n = c->ncap * c->Mp; break;
    case 2: p = c->q; n = c->ldk; break;              case 3: p = c->loc; n = kn; break;
    case 4: p = c->tt; n = kn; break;                 case 5: p = c->vbar; n = kn; break;
    case 6: p = c->locbar; n = kn; break;             case 7: p = c->asum; n = c->ldk; break;
    case 8: p = c->Kuu; n = mm; e = (int)c->ssz; break;   case 9: p = c->L; n = mm; e = (int)c->ssz; break;
    case 10: p = c->Linv; n = mm; e = (int)c->ssz; break; case 11: p = c->S; n = mm * c->K; break;
    case 12: p = c->Bm; n = mm * c->K; break;         case 13: p = c->phi; n = (int64_t)c->K * c->V; break;
    case 14: p = c->mu; n = kn; break;                case 15: p = c->LinvT; n = mm; e = (int)c->ssz; break;
    case 16: p = c->ST; n = mm * c->K; break;
    case 17: p = c->Knm; n = c->ncap * c->Mp; e = (int)c->ssz; break;
    case 18: p = c->g_locbar; n = c->g_locbar ? kn : 0; break;
    default: return fail(-1, "gdrf_ws_ptr", "unknown buffer id");
  }
  *ptr = p; *nelem = n; *esz = e;
  return 0;
}
int gdrf_ws_ptr(gdrf_ctx* c, int which, void** ptr, int64_t* nelem) { int e; return ws_lookup(c, which, ptr, nelem, &e); }
int gdrf_stores_t(const gdrf_ctx* c) { return c->Tst != nullptr; }
int gdrf_set_mfma_mode(gdrf_ctx* c, int mode) {
  if (mode < 0 || mode > 2) return fail(-1, "gdrf_set_mfma_mode", "mode");
  if (mode != 0 && (c->esz != 4 || c->Tst)) return fail(-1, "gdrf_set_mfma_mode", "the split modes need float arrays and the dense Wbar form");
  // f16x3 scales W by the bound |w| <= sqrt(variance), which the f64 solve guarantees (4x headroom); an all-fp32 solve of an ill-conditioned
  // K_uu can break it and the fp16 pieces would overflow to inf without a trace: bf16x6 (f32's exponent range) is the split mode there
  if (mode == 2 && c->ssz != 8) return fail(-1, "gdrf_set_mfma_mode", "f16x3 needs the f64 solve (GDRF_F32); use bf16x6 or f32 with GDRF_F32_PURE");
  HIPCHK(hipSetDevice(c->dev));
  const int np = mode == 1 ? 3 : (mode == 2 ? 2 : 0);
  if (np > c->wh_pieces) {            // 16-bit pieces of W: np x n_cap x Mp halfwords, allocated on first use
    if (int rc = ctx_alloc(c, &c->Wh, (size_t)np * c->ncap * c->Mp * 2, "hipMalloc(Wh)")) return rc;
    c->wh_pieces = np;
  }
  c->split = mode;
  return 0;
}
int gdrf_set_mean(gdrf_ctx* c, const void* mean, int64_t stride_k, int64_t stride_n) {
  if (stride_k < 0 || stride_n < 0) return fail(-1, "gdrf_set_mean", "strides must be >= 0 (0 broadcasts)");
  c->mean = mean; c->mean_sk = stride_k; c->mean_sn = stride_n;
  return 0;
}

int gdrf_set_mean_guide(gdrf_ctx* c, const void* mean, int64_t stride_k, int64_t stride_n) {
  if (stride_k < 0 || stride_n < 0) return fail(-1, "gdrf_set_mean_guide", "strides must be >= 0 (0 broadcasts)");
  c->mean_g = mean; c->mean_g_sk = stride_k; c->mean_g_sn = stride_n;
  return 0;
}

int gdrf_set_whiten(gdrf_ctx* c, int whiten) {
  if (whiten != 0 && whiten != 1) return fail(-1, "gdrf_set_whiten", "whiten must be 0 or 1");
  if (!whiten && c->Tst) return fail(-1, "gdrf_set_whiten", "whiten = 0 needs the dense Wbar form (GDRF_STORE_T_OFF)");
  HIPCHK(hipSetDevice(c->dev));
  if (!whiten && !c->uS) {
    const size_t kmm = (size_t)c->K * c->Mp * c->Mp * c->ssz, kv = (size_t)c->K * c->Mp * c->ssz;
    void** ps[] = {&c->uS, &c->uSb, &c->uSc, &c->uU, &c->uUb, &c->Uw};
    const size_t sz[] = {kmm, kmm, kmm, kv, kv, (size_t)c->K * c->M * c->esz};
    for (int i = 0; i < 6; ++i)
      if (int rc = ctx_alloc(c, ps[i], sz[i], "hipMalloc(unwhitened scratch)", true)) return rc;
  }
  c->unwhitened = !whiten;
  return 0;
}
int gdrf_set_learn_inducing(gdrf_ctx* c, int on) {
  if (on != 0 && on != 1) return fail(-1, "gdrf_set_learn_inducing", "on must be 0 or 1");
  HIPCHK(hipSetDevice(c->dev));
  if (on && !c->zpart) {
    const size_t bytes = (size_t)((c->ncap + GDRF_TILE - 1) / GDRF_TILE) * c->M * dcap(c) * sizeof(double);
    if (int rc = ctx_alloc(c, &c->zpart, bytes, "hipMalloc(zpart)")) return rc;
  }
  c->learn_z = on;
  return 0;
}
int gdrf_set_ard(gdrf_ctx* c, int on) {
  if (on != 0 && on != 1) return fail(-1, "gdrf_set_ard", "on must be 0 or 1");
  if (c->prod) return fail(-1, "gdrf_set_ard", "a product context takes its lengthscale counts from gdrf_set_product");
  HIPCHK(hipSetDevice(c->dev));
  if (on && !c->Zp) {
    // apart: D per backward workgroup (at most dpart_len / 3 of them, gdrf_step_local checks) or per inducing point (M < dpart_len)
    if (int rc = ctx_alloc(c, &c->Zp, (size_t)c->Mp * c->D * c->esz, "hipMalloc(ARD scratch)")) return rc;
    if (int rc = ctx_alloc(c, &c->apart, (size_t)c->dpart_len * c->D * sizeof(double), "hipMalloc(ARD scratch)")) return rc;
  }
  c->ard = on;
  c->prefact_valid = 0;
  return 0;
}
int gdrf_set_period_count(gdrf_ctx* c, int count) {
  if (!c->per || c->prod) return fail(-1, "gdrf_set_period_count", "not a periodic context (kernel_id GDRF_PERIODIC)");
  if (count != 1 && count != c->Dr) return fail(-1, "gdrf_set_period_count", "count must be 1 or the number of input dimensions");
  if (c->g_loc) return fail(-1, "gdrf_set_period_count", "call it before the first gdrf_step_local2");
  c->np = count;
  c->prefact_valid = 0;
  return 0;
}
int gdrf_set_product(gdrf_ctx* c, int nfactors, const int* table) {
  if (!c->prod) return fail(-1, "gdrf_set_product", "not a product context (kernel_id GDRF_PRODUCT)");
  if (c->g_loc) return fail(-1, "gdrf_set_product", "call it before the first gdrf_step_local2");
  if (nfactors < 1 || nfactors > GDRF_DMAX || !table) return fail(-1, "gdrf_set_product", "1 to 4 factors");
  int coords = 0, nls = 0, nper = 0, npair = 0;
  for (int f = 0; f < nfactors; ++f) {
    const int* fa = table + 8 * f;
    const int kind = fa[0], na = fa[1];
    if (kind != GDRF_RBF && kind != GDRF_PERIODIC) return fail(-1, "gdrf_set_product", "a factor's kind must be GDRF_RBF or GDRF_PERIODIC");
    if (na < 1 || na > GDRF_DMAX) return fail(-1, "gdrf_set_product", "a factor reads 1 to 4 axes");
    for (int k = 0; k < na; ++k) {
      if (fa[4 + k] < 0 || fa[4 + k] >= c->Dr) return fail(-1, "gdrf_set_product", "an active axis is not < D");
      for (int q = 0; q < k; ++q)
        if (fa[4 + q] == fa[4 + k]) return fail(-1, "gdrf_set_product", "a factor lists an axis twice");
    }
    if (fa[2] != 1 && fa[2] != na) return fail(-1, "gdrf_set_product", "a factor's lengthscale count must be 1 or its axis count");
    if (kind == GDRF_RBF && fa[3] != 0) return fail(-1, "gdrf_set_product", "an RBF factor has no period");
    if (kind == GDRF_PERIODIC && fa[3] != 1 && fa[3] != na)
      return fail(-1, "gdrf_set_product", "a Periodic factor's period count must be 1 or its axis count");
    coords += kind == GDRF_PERIODIC ? 2 * na : na;
    npair += kind == GDRF_PERIODIC ? na : 0;
    nls += fa[2]; nper += fa[3];
  }
  if (coords > GDRF_DMAX) return fail(-1, "gdrf_set_product", "more than 4 embedded coordinates (an RBF axis takes 1, a Periodic axis 2)");
  for (int f = 0; f < GDRF_DMAX; ++f)
    for (int k = 0; k < 8; ++k) c->pfac[f][k] = f < nfactors ? table[8 * f + k] : 0;
  c->nf = nfactors; c->nls = nls; c->nper = nper; c->npair = npair; c->D = coords;
  c->prefact_valid = 0;
  return 0;
}
int gdrf_set_mean_params(gdrf_ctx* c, int64_t count) {
  if (count < 0) return fail(-1, "gdrf_set_mean_params", "count must be >= 0");
  // the two-point scratch (gdrf_step_local2) holds a copy of red_d sized on its first use
  if (c->g_loc && count != c->mean_count) return fail(-1, "gdrf_set_mean_params", "call it before the first gdrf_step_local2");
  c->mean_count = count;
  return 0;
}
int gdrf_get_mfma_mode(const gdrf_ctx* c) { return c->split; }
int gdrf_set_hyper_backward(gdrf_ctx* c, int mode) {
  if (mode != 0 && mode != 1) return fail(-1, "gdrf_set_hyper_backward", "mode must be 0 (f64 backward GEMM) or 1 (Hd = dK^T Wbar on the TN kernel)");
  c->hyper_tn = mode;
  return 0;
}
int gdrf_get_hyper_backward(const gdrf_ctx* c) { return hyper_tn_on(c) ? 1 : 0; }
int gdrf_set_rows_form(gdrf_ctx* c, int form) {
  if (form != 0 && form != 1) return fail(-1, "gdrf_set_rows_form", "form must be 0 (the LDS row forms) or 1 (vocabulary-streamed)");
  c->rows_form = form;
  return 0;
}
int gdrf_get_rows_form(const gdrf_ctx* c) { return c->rows_form; }
int gdrf_last_forms(const gdrf_ctx* c, int* out, int n) {
  if (!c || (n > 0 && !out)) return fail(-1, "gdrf_last_forms", "null argument");
  for (int i = 0; i < n; ++i) out[i] = i < GDRF_NFORMS ? c->forms[i] : 0;
  return 0;
}
int gdrf_quant_last_plan(const gdrf_ctx* c, int out[3]) {
  if (!c || !out) return fail(-1, "gdrf_quant_last_plan", "null argument");
  for (int i = 0; i < 3; ++i) out[i] = c->quant_plan[i];
  return 0;
}

int gdrf_loo_last_plan(const gdrf_ctx* c, int out[2]) {
  if (!c || !out) return fail(-1, "gdrf_loo_last_plan", "null argument");
  for (int i = 0; i < 2; ++i) out[i] = c->loo_plan[i];
  return 0;
}

// the LDS row forms' Phi-bar partials, [erows_grid_cap][K*V]: allocated on the first launch that writes them
static int phibar_part_ensure(gdrf_ctx* c) {
  if (c->phibar_part) return 0;
  return ctx_alloc(c, &c->phibar_part, (size_t)c->erows_grid_cap * c->K * c->V * c->esz, "hipMalloc(phibar_part)");
}
// form 1 scratch on first use.  The grid of the streamed kernels is capped so that its Phi-bar slots take at most
// max(256 MiB, 16 K V elements), never 1024 K V: vs_gcap = min(1024, max(16, 256 MiB / (K V esz)), ceil(n_cap / 64))
static int csr_ensure(gdrf_ctx* c);
// (`counts`: the call reads counts; with a bound CSR matrix it then takes the sparse form's scratch instead)
static int vs_ensure(gdrf_ctx* c, bool counts = true) {
  if (c->csr_crow && counts) return csr_ensure(c);
  if (c->vs_part) return 0;
  const size_t kv = (size_t)c->K * c->V * c->esz;
  c->vs_gcap = std::min<int64_t>({(int64_t)1024, std::max<int64_t>(16, (int64_t)((size_t)256 << 20) / (int64_t)kv), (c->ncap + 63) / 64});
  void** ps[] = {&c->vs_tmp, &c->vs_cpart, &c->vs_rs, &c->vs_part};
  const size_t sz[] = {(size_t)c->K * c->ldk * c->esz, (size_t)c->vs_gcap * c->K * c->esz, (size_t)2 * c->K * c->esz, (size_t)c->vs_gcap * kv};
  for (int i = 0; i < 4; ++i)
    if (!*ps[i])
      if (int rc = ctx_alloc(c, ps[i], sz[i], "hipMalloc(streamed row form scratch)")) return rc;
  return 0;
}
// the sparse row form's scratch that does not depend on nnz, on first use; a context that never binds a CSR matrix holds none of it.  The
// (K, ldk) array and the row sums are the streamed form's (vs_ensure allocates whichever of its own are still missing).
static int csr_ensure(gdrf_ctx* c) {
  if (c->csr_slot) return 0;
  const size_t kv = (size_t)c->K * c->V * c->esz;
  void** ps[] = {&c->vs_tmp, &c->vs_rs, &c->csr_phiT, &c->csr_thN, &c->csr_cn, &c->csr_cpart, &c->csr_slot};
  const size_t sz[] = {(size_t)c->K * c->ldk * c->esz, (size_t)2 * c->K * c->esz, (size_t)c->V * round_up(c->K, 16) * c->esz,
                       (size_t)c->ncap * c->K * c->esz, (size_t)c->ncap * c->esz, (size_t)1024 * c->K * c->esz, kv};
  for (int i = 0; i < 7; ++i)
    if (!*ps[i])
      if (int rc = ctx_alloc(c, ps[i], sz[i], "hipMalloc(sparse row form scratch)")) return rc;
  return 0;
}
// the arrays of the sparse row form that grow with nnz (in steps of a quarter, so that mini-batches of varying size settle quickly).  The
// blocks they replace are released: hipFree waits for the work that may still read them.
static int csr_grow(gdrf_ctx* c, int64_t nnz) {
  if (c->csr_pb && nnz <= c->csr_cap) return 0;
  const int64_t cap = std::max<int64_t>(nnz + nnz / 4, 1024), nseg = c->V + cap / CSR_SEG + 1;
  void** ps[] = {&c->csr_pb, (void**)&c->csr_erow, (void**)&c->csr_segcol, (void**)&c->csr_segoff, &c->csr_parts};
  const size_t sz[] = {(size_t)cap * c->esz, (size_t)cap * sizeof(int32_t), (size_t)nseg * sizeof(int32_t), (size_t)(c->V + 1) * sizeof(int64_t),
                       (size_t)nseg * c->K * c->esz};
  for (int i = 0; i < 5; ++i) {
    if (*ps[i]) {
      c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), *ps[i]), c->allocs.end());
      HIPCHK(hipFree(*ps[i]));
      *ps[i] = nullptr;
    }
    if (int rc = ctx_alloc(c, ps[i], sz[i], "hipMalloc(sparse row form scratch)")) return rc;
  }
  c->csr_cap = cap;
  c->csr_fresh = 1;
  return 0;
}
int gdrf_bind_counts_csr(gdrf_ctx* c, const int64_t* crow, const int32_t* col, const int32_t* val, int64_t n, int64_t nnz, const int64_t* ccol,
                         const int64_t* cperm) {
  if (!c) return fail(-1, "gdrf_bind_counts_csr", "null context");
  if (!crow) {
    c->csr_crow = c->csr_ccol = c->csr_cperm = nullptr; c->csr_col = c->csr_val = nullptr; c->csr_n = c->csr_nnz = 0;
    return 0;
  }
  if (n < 1 || nnz < 0) return fail(-1, "gdrf_bind_counts_csr", "n must be >= 1 and nnz >= 0");
  if (nnz > 0 && (!col || !val)) return fail(-1, "gdrf_bind_counts_csr", "col_dev and val_dev are required when nnz > 0");
  if ((ccol == nullptr) != (cperm == nullptr) && nnz > 0) return fail(-1, "gdrf_bind_counts_csr", "ccol_dev and cperm_dev come together");
  c->csr_crow = crow; c->csr_col = col; c->csr_val = val; c->csr_n = n; c->csr_nnz = nnz; c->csr_ccol = ccol; c->csr_cperm = cperm;
  c->csr_fresh = 1;
  return 0;
}
// With a bound CSR matrix the calls that read counts take ws_dev = NULL and the bound matrix's row count
static int counts_check(const gdrf_ctx* c, const int32_t* ws, int64_t n, const char* fn) {
  if (!c->csr_crow) return 0;
  if (ws) return fail(-1, fn, "a CSR count matrix is bound (gdrf_bind_counts_csr): ws_dev must be NULL");
  if (n != c->csr_n) return fail(-1, fn, "n differs from the row count of the bound CSR count matrix");
  return 0;
}
int gdrf_ws_elem_size(gdrf_ctx* c, int which) { void* p; int64_t n; int e; return ws_lookup(c, which, &p, &n, &e) ? -1 : e; }

int gdrf_set_timing(gdrf_ctx* c, int enable) {
  c->timing = enable;
  for (int i = 0; i < GDRF_NSLOTS; ++i) { c->t_ms[i] = 0; c->t_cnt[i] = 0; }
  return 0;
}
int gdrf_get_timing(gdrf_ctx* c, double* ms_out, int64_t* cnt_out, int nslots) {
  HIPCHK(hipSetDevice(c->dev));
  for (auto& t : c->tev) {
    HIPCHK(hipEventSynchronize(t.second.second));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, t.second.first, t.second.second));
    c->t_ms[t.first] += ms; c->t_cnt[t.first] += 1;
    c->ev_pool.push_back(t.second.first); c->ev_pool.push_back(t.second.second);
  }
  c->tev.clear();
  for (int i = 0; i < nslots && i < GDRF_NSLOTS; ++i) { ms_out[i] = c->t_ms[i]; cnt_out[i] = c->t_cnt[i]; }
  return 0;
}

// make stream s wait for the factorisation queued on the side stream (no-op before the first gdrf_factorize)
static int join_fact(gdrf_ctx* c, hipStream_t s) {
  if (c->fact_pending) HIPCHK(hipStreamWaitEvent(s, c->ev_fact, 0));
  return 0;
}

int gdrf_ws_copy(gdrf_ctx* c, int which, void* dst, int64_t nelem, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  void* p; int64_t n; int e;
  int rc = ws_lookup(c, which, &p, &n, &e);
  if (rc) return rc;
  if (nelem > n) return fail(-1, "gdrf_ws_copy", "nelem exceeds the buffer");
  if ((rc = join_fact(c, (hipStream_t)stream))) return rc;
  HIPCHK(hipMemcpyAsync(dst, p, (size_t)nelem * e, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

// A launch with `lds` bytes of dynamic LDS: more than the 48 KB default needs the kernel's limit raised first
template <typename... KA, typename... A>
static int launch_lds(void (*kern)(KA...), dim3 grid, dim3 block, size_t lds, hipStream_t s, A... args) {
  if (lds > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, grid, block, lds, s, args...);
  return 0;
}

// fn<SP>(...) of Impl for the context's split mode: 2 = f16x3 (SplitF16), 1 = bf16x6 (SplitBf16)
#define BY_SPLIT(c, fn, ...) ((c)->split == 2 ? fn<SplitF16>(__VA_ARGS__) : fn<SplitBf16>(__VA_ARGS__))

#define GDRF_STREAMED_HINT "the vocabulary-streamed row form (gdrf_set_rows_form(ctx, 1), rows_form=\"streamed\") has no such limit"
static int rows_lds_fail(const char* fn) {
  return fail(-1, fn, "num_topic_categories x num_observation_categories too large for the row kernel's LDS; " GDRF_STREAMED_HINT);
}

// The (LG, KJ) forms of the lane-group row kernels (lane_group.h: LG lanes own a row, KJ topics per lane, LG x KJ >= K), by K:
//   K <=          8        16        32        64       128
//   predictive  (8, 1)   (16, 1)   (32, 1)   (64, 1)   (64, 2)     predict_mc_kernel, predict_info_kernel, predict_score_kernel, foldin_kernel
//   sparse      (8, 1)   (16, 2)   (16, 2)   (16, 8)   (16, 8)     rows_csr_kernel, csr_phibar_seg_kernel
// They differ and are kept: the sparse kernels pay a butterfly over the group (and LG entries fetched) per stored entry, so their groups
// stop at 16 lanes and more topics go into a lane's registers; the predictive kernels reduce over the group per row and sample only and
// spread the words over the same lanes, so they widen the group with K first.  Each dispatcher hands the pair to f as the compile-time
// constants F::LG, F::KJ of its argument's type F.
template <int LG_, int KJ_> struct LaneForm { static constexpr int LG = LG_, KJ = KJ_; };
template <typename F> static int predictive_form(int K, F&& f) {
  return K <= 8 ? f(LaneForm<8, 1>()) : K <= 16 ? f(LaneForm<16, 1>()) : K <= 32 ? f(LaneForm<32, 1>()) : K <= 64 ? f(LaneForm<64, 1>()) : f(LaneForm<64, 2>());
}
template <typename F> static int sparse_form(int K, F&& f) {
  return K <= 8 ? f(LaneForm<8, 1>()) : K <= 32 ? f(LaneForm<16, 2>()) : f(LaneForm<16, 8>());
}
// the grid of the predictive lane-group kernels: 256 / LG rows per workgroup pass, at most 1024 workgroups striding over the rows
static int lane_group_grid(int64_t n, int LG) {
  const int64_t nblk = (n + 256 / LG - 1) / (256 / LG);
  return (int)std::max<int64_t>(1, std::min<int64_t>(nblk, 1024));
}

// ------------------------------------------------------------------------------------------------
// T = N-side element type, TS = solve element type
template <typename T, typename TS> struct Impl {
  using C = NTCfg<T>;
  using CS = NTCfg<TS>;
  static constexpr bool kSame = std::is_same<T, TS>::value;
  static T* P(void* p) { return reinterpret_cast<T*>(p); }
  static const T* P(const void* p) { return reinterpret_cast<const T*>(p); }
  static TS* Q(void* p) { return reinterpret_cast<TS*>(p); }

  // column tiles of the NT core for element type E (128 wide for f32, 64 for f64); row tiles are always 128
  template <typename E> static int nct(const gdrf_ctx* c) { return (c->Mp + NTCfg<E>::CW - 1) / NTCfg<E>::CW; }

  // C = alpha A B^T on M x M operands, `batch` of them.  The plan (forms.h: mm_plan) splits the reduction of a single product over slices
  // into the context's one slab buffer, added in a fixed order; `beside_chain`: the product runs on the side stream while the Cholesky-backward
  // chain uses that buffer on the main one, and is launched directly.  `slot`: the slot of gdrf_last_forms that reports the form, or -1.
  template <typename E>
  static int mm_nt(gdrf_ctx* c, const E* A, int64_t abs_, const E* Bt, int64_t bbs, E* Cm, int64_t cbs, E alpha, int batch,
                   hipStream_t s, bool beside_chain = false, int slot = -1) {
    const int64_t mm = (int64_t)c->Mp * c->Mp;
    const int tiles = c->nt * nct<E>(c);
    const F::MmPlan pl = F::mm_plan(c->Mp, (int)sizeof(E), batch, tiles, c->mmslab ? c->mmslab_bytes : 0, beside_chain);
    if (slot >= 0) c->forms[slot] = pl.form;
    if (pl.split()) {
      MMProb<E> p{{}, {}, {}, A, abs_, Bt, bbs, (E*)c->mmslab, mm, c->Mp, alpha, pl.kw, batch};
      dim3 grid(tiles, pl.S * batch);
      hipLaunchKernelGGL((gemm_nt_kernel<E, MMProb<E>>), grid, dim3(256), NTCfg<E>::LDS_BYTES, s, p);
      hipLaunchKernelGGL(reduce_slabs_kernel<E>, dim3((c->Mp + 255) / 256, c->Mp, batch), dim3(256), 0, s, (const E*)c->mmslab, pl.S, batch, c->Mp, 0, Cm, GDRF_TILE / 2);
      LAUNCHCHK("mm_nt split-K");
      return 0;
    }
    MMProb<E> p{{}, {}, {}, A, abs_, Bt, bbs, Cm, cbs, c->Mp, alpha, 0, 1};
    dim3 grid(c->nt * nct<E>(c), batch);
    hipLaunchKernelGGL((gemm_nt_kernel<E, MMProb<E>>), grid, dim3(256), NTCfg<E>::LDS_BYTES, s, p);
    LAUNCHCHK("mm_nt");
    return 0;
  }

  // What the covariance kernels read, refreshed from the parameters: the hyper-parameter block h, and the inducing inputs in precision TO,
  // which are returned.  Periodic and product contexts: the embedded inducing inputs (M, D) in zout, with the phases of their pairs
  // (M, npair) when ph is given.  ARD contexts: the scaled inducing inputs z_d / ls_d in zout; ls = 1 in the hyper-parameter block.
  // Otherwise Z itself, or with `copy` its cast into zout.
  template <typename TO>
  static const TO* cov_inputs(gdrf_ctx* c, const T* Z, const T* params, Hyper* h, TO* zout, TO* ph, bool copy, hipStream_t s) {
    const int64_t nz = (int64_t)c->M * c->D;
    if (c->per) {
      const CoordTab tb = coord_tab(c);
      const int64_t nzr = (int64_t)c->M * tb.nsrc;
      hipLaunchKernelGGL(prep_hyper_per_kernel<T>, dim3(1), dim3(64), 0, s, params, tb, (HyperPer*)h);
      hipLaunchKernelGGL((embed_per_kernel<T, TO>), dim3((unsigned)((nzr + 255) / 256)), dim3(256), 0, s, (int64_t)c->M, tb, Z, params, zout, ph);
    } else if (c->ard) {
      const T* ls = params + param_lay(c).ard;
      hipLaunchKernelGGL(prep_hyper_ard_kernel<T>, dim3(1), dim3(64), 0, s, params, ls, c->D, h);
      hipLaunchKernelGGL((scale_z_kernel<T, TO>), dim3((unsigned)((nz + 255) / 256)), dim3(256), 0, s, nz, c->D, Z, ls, zout);
    } else {
      hipLaunchKernelGGL(prep_hyper_kernel<T>, dim3(1), dim3(64), 0, s, params, h);
      if constexpr (std::is_same<T, TO>::value) {
        if (!copy) return Z;
      }
      hipLaunchKernelGGL((cast_kernel<T, TO>), dim3((unsigned)((nz + 255) / 256)), dim3(256), 0, s, nz, Z, zout);
    }
    return zout;
  }
  // The rows of one call: X is what K_nm is evaluated at, Xr the caller's raw rows (the period sums of the backward).  They differ in periodic
  // and product contexts only, where step_inputs writes the embedded rows (n, D) into c->Xe.  More rows than it holds (gdrf_knm, gdrf_predict)
  // grow it; the old buffer stays allocated until gdrf_ctx_destroy, since work queued before may still read it.
  struct StepRows { const T* X; const T* Xr; };
  static int step_inputs(gdrf_ctx* c, const T* X, int64_t n, const T* params, hipStream_t s, StepRows* r) {
    *r = {X, X};
    if (!c->per) return 0;
    if (n > c->xe_cap) {
      if (int rc = ctx_alloc(c, &c->Xe, (size_t)n * c->D * c->esz, "hipMalloc(embedded rows)")) return rc;
      c->xe_cap = n;
    }
    const CoordTab tb = coord_tab(c);
    const int64_t nx = n * tb.nsrc;
    if (nx > 0)
      hipLaunchKernelGGL((embed_per_kernel<T, T>), dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, s, n, tb, X, params, (T*)c->Xe, (T*)nullptr);
    LAUNCHCHK("embed rows (periodic)");
    r->X = (const T*)c->Xe;
    return 0;
  }
  // nlev (<= 8) Cholesky attempts in ONE launch, in the N-side precision (what the reference's fp32
  // torch.linalg.cholesky would see): K_uu built once, one workgroup per cumulative jitter; flags in c->flag[8..8+nlev)
  // (slot 0 is the solve factorisation's, so a probe may run on another stream beside gdrf_factorize)
  static int probe(gdrf_ctx* c, const T* Z, const T* params, const double* jitters, int nlev, hipStream_t s) {
    const int Mp = c->Mp, M = c->M;
    ScopedTimer tm(c, 0, s);
    HIPCHK(hipMemsetAsync(c->flag + 8, 0, 32, s));
    dim3 g2((Mp + 255) / 256, Mp);
    Z = cov_inputs<T>(c, Z, params, c->hyp_probe, P(c->Zp), nullptr, false, s);
    hipLaunchKernelGGL(kuu_kernel<T>, g2, dim3(256), 0, s, Z, M, Mp, c->D, c->kind, c->hyp_probe, 0.0, P(c->pK));
    JitterLevels jl;
    for (int l = 0; l < 8; ++l) jl.v[l] = l < nlev ? jitters[l] : 0.0;
    dim3 g3((Mp + 255) / 256, Mp, nlev);
    hipLaunchKernelGGL(level_copies_kernel<T>, g3, dim3(256), 0, s, (const T*)P(c->pK), M, Mp, jl, P(c->pL));
    if (int rc = launch_lds(chol_kernel<T>, dim3(nlev), dim3(1024), chol_lds_bytes<T>(M), s, P(c->pL), M, Mp, c->flag + 8, (int64_t)Mp * Mp))
      return rc;
    LAUNCHCHK("probe");
    return 0;
  }

  // K_uu(+jitter) -> Cholesky(flag) -> L, LT -> Linv, LinvT in the solve precision.  The hyper-parameters and the cast of Z
  // are refreshed on the caller's stream; the factorisation chain (one workgroup for most of its 1.7 ms) runs on the
  // context's side stream so that what follows on the caller's stream and does not need L (the S / B_k transforms and the
  // solve-precision K_nm of gdrf_step_local) overlaps it.  Every consumer of L calls join_fact() first.
  // mode 0: factorise.  mode 1: factorise AHEAD of the step that will use it (right behind the optimizer update, so that the chain runs while
  // the host reads the loss and enqueues the next step) and keep a copy of its inputs.  mode 2: the step's own call - if a mode-1
  // factorisation with this jitter is waiting, only compare its inputs with the current ones on the device (flag[16], read with the
  // failure flag by gdrf_chol_failed: a mismatch makes the caller redo the step, like a wrong jitter guess); otherwise as mode 0.
  static int factorize(gdrf_ctx* c, const T* Z, const T* params, double jitter, hipStream_t s, int mode = 0) {
    const int Mp = c->Mp, M = c->M;
    const int64_t nzs = (int64_t)M * c->Dr;
    if (mode == 2 && c->prefact_valid && jitter == c->prefact_jitter) {
      hipLaunchKernelGGL(fact_snapshot_kernel<T>, dim3(1), dim3(256), 0, s, params, Z, nzs, P(c->snap), 1, c->flag + 16, params + param_lay(c).ard,
                         snap_extra(c));
      // the factorisation stays valid for further calls with the same inputs (a predictive evaluation between two steps): every reuse
      // compares again, and any fresh factorisation below invalidates it first
      LAUNCHCHK("factorize (reuse)");
      return 0;
    }
    c->prefact_valid = 0;
    if (mode != 1) HIPCHK(hipMemsetAsync(c->flag + 16, 0, sizeof(int), s));     // this stream's own factorisation: nothing reused, no mismatch to report
    dim3 g2((Mp + 255) / 256, Mp);
    cov_inputs<TS>(c, Z, params, c->hyp, Q(c->Zs), Q(c->Zph), true, s);      // the inducing inputs (and phases) in the solve precision: c->Zs, c->Zph
    HIPCHK(hipEventRecord(c->ev_fact0, s));
    hipStream_t f = c->side;
    HIPCHK(hipStreamWaitEvent(f, c->ev_fact0, 0));
    {
      ScopedTimer tm(c, 15, f);
      HIPCHK(hipMemsetAsync(c->flag, 0, 32, f));
      hipLaunchKernelGGL(kuu_kernel<TS>, g2, dim3(256), 0, f, (const TS*)Q(c->Zs), M, Mp, c->D, c->kind, c->hyp, jitter, Q(c->Kuu));
      HIPCHK(hipMemcpyAsync(c->Lw, c->Kuu, (size_t)Mp * Mp * sizeof(TS), hipMemcpyDeviceToDevice, f));
      // one launch per 32-column panel, one small workgroup per trailing tile (kernels_mm.h: chol_panel_kernel); the inverses of the
      // diagonal blocks come out of the panel launches
      const int nt = (M + 31) / 32;
      for (int k = 0; k < nt; ++k) {
        const int n = nt - k - 1, wgs = n > 0 ? n * (n + 1) / 2 : 1;
        hipLaunchKernelGGL(chol_panel_kernel<TS>, dim3((unsigned)wgs), dim3(128), 0, f, Q(c->Lw), Q(c->Lo), Q(c->Dinv), M, Mp, k, c->flag);
      }
      hipLaunchKernelGGL(finalize_l_kernel<TS>, g2, dim3(256), 0, f, (const TS*)Q(c->Lo), M, Mp, Q(c->L), Q(c->LT));
      hipLaunchKernelGGL(trinv_cols_kernel<TS>, dim3(Mp / 32), dim3(1024), 0, f, (const TS*)Q(c->L), (const TS*)Q(c->Dinv), M, Mp, Q(c->Linv),
                         Q(c->LinvT));
    }
    HIPCHK(hipEventRecord(c->ev_fact, f));
    c->fact_pending = 1;
    if (mode == 1) {
      hipLaunchKernelGGL(fact_snapshot_kernel<T>, dim3(1), dim3(256), 0, s, params, Z, nzs, P(c->snap), 0, (int*)nullptr, params + param_lay(c).ard,
                         snap_extra(c));
      c->prefact_valid = 1; c->prefact_jitter = jitter;
    }
    LAUNCHCHK("factorize");
    return 0;
  }

  static int knm(gdrf_ctx* c, const T* X, int64_t n, const T* Z, const T* params, T* out, int64_t ldo, hipStream_t s) {
    Z = cov_inputs<T>(c, Z, params, c->hyp, P(c->Zp), nullptr, false, s);
    StepRows r;
    if (int rc = step_inputs(c, X, n, params, s, &r)) return rc;
    X = r.X;
    ScopedTimer tm(c, 1, s);
    const int VE = Vec16<T>::N;
    const int vpr = (c->M + VE - 1) / VE, rpp = vpr <= 256 ? 256 / vpr : 1;
    int64_t blocks = (n + 4 * rpp - 1) / (4 * rpp);
    const int64_t cap = 256 * 64;          // swept on MI355X: 2048 blocks 0.60-0.65 of HBM peak, 16384 0.67-0.79
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    if (ard_fwd(c))
      hipLaunchKernelGGL((knm_kernel<T, T, true, true, true>), dim3((unsigned)blocks), dim3(256), 0, s, X, n, Z, c->M, c->D, c->kind, c->hyp, out, ldo);
    else
      hipLaunchKernelGGL((knm_kernel<T, T, true, true>), dim3((unsigned)blocks), dim3(256), 0, s, X, n, Z, c->M, c->D, c->kind, c->hyp, out, ldo);
    LAUNCHCHK("knm");
    return 0;
  }

  // block scales of the split modes (gemm_split.h): `what` = SPLIT_SC_* groups to refresh from hyp / the maxima
  static void split_scales(gdrf_ctx* c, int what, hipStream_t s) {
    hipLaunchKernelGGL(split_scales_kernel, dim3(1), dim3(64), 0, s, c->split == 2 ? 1 : 0, (const Hyper*)c->hyp, (const unsigned*)c->smx, c->ssc, c->K, what);
  }

  // pieces of S_k^T (and of W in the all-fp32 mode), then tt on the 16-bit matrix path (f32 contexts only)
  template <class SP>
  static int fwd_t_split(gdrf_ctx* c, int64_t n, hipStream_t s) {
    if constexpr (std::is_same<T, float>::value) {
      using E = typename SP::E;
      const int Mp = c->Mp, K = c->K;
      const SplitLay SL{K};
      const int64_t nb = (int64_t)K * Mp * Mp, nw = n * Mp;
      {
        ScopedTimer tm(c, 2, s);
        hipLaunchKernelGGL(split_blocked_kernel<SP>, dim3((unsigned)((nb / 4 + 255) / 256)), dim3(256), 0, s, (const float*)c->ST, nb, Mp, Mp, (E*)c->STh, nb,
                           (const float*)c->ssc + SL.st(0));
        if (c->ssz != 8)       // with the f64 solve, fwd_w's epilogue has already written the pieces of W
          hipLaunchKernelGGL(split_kernel<SP>, dim3((unsigned)((nw / 4 + 255) / 256)), dim3(256), 0, s, (const float*)c->W, nw, (E*)c->Wh,
                             (int64_t)c->ncap * Mp, (const float*)c->ssc + SL.w());
      }
      ScopedTimer tm(c, 5, s);
      const F::FwdTPlan pl = F::fwd_t_plan(form_shape(c, n));
      c->forms[GDRF_FORM_FWD_T] = pl.form; c->forms[GDRF_FORM_FWD_T_KG] = pl.KG;
      FwdTSplitArgs<SP> a{(const E*)c->Wh, (int64_t)c->ncap * Mp, n, Mp, K, pl.KG, pl.rt8, (const E*)c->STh, nb, (float*)c->tt, c->ldk, (const float*)c->ssc};
      auto launch = [&](auto kern, unsigned grid, int threads, int lds) {
        HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, s, a);
        return 0;
      };
      int rc = 0;
      switch (pl.form) {
        case F::FWD_T_W1:
          if constexpr (std::is_same<SP, SplitF16>::value) {
            if (pl.KQ) {
              a.k_lo = 0; a.k_n = pl.KQ; a.KG = 1; a.rt8 = pl.rt8_q;
              if ((rc = launch(fwd_t_f16_w1_kernel<true>, pl.grid_q, pl.threads, pl.lds_q))) return rc;
            }
            if (pl.KP) {
              a.k_lo = pl.KQ; a.k_n = K - pl.KQ; a.KG = pl.KGP; a.rt8 = pl.rt8;
              if ((rc = launch(fwd_t_f16_w1_kernel<false>, pl.grid_p, pl.threads, pl.lds_p))) return rc;
            }
          }
          break;
        case F::FWD_T_Q4:
          if constexpr (SP::NP == 2) rc = launch(fwd_t_split_q4_kernel<SP>, pl.grid, pl.threads, pl.lds);
          break;
        default:
          if constexpr (SP::NP != 2) rc = launch(fwd_t_split_cc_kernel<SP>, pl.grid, pl.threads, pl.lds);
          break;
      }
      if (rc) return rc;
      LAUNCHCHK("fwd_t_split");
      return 0;
    } else {
      return fail(-1, "fwd_t_split", "float arrays only");
    }
  }

  // C = Wh^T diag(scale) B over the observations on the 16-bit matrix path (f32 contexts only); A side = the pieces of W.
  // sidx_b / sidx_b_stride: SplitLay pair index of the block scale of the row-scaled B operand (per batch)
  template <class SP>
  static int tn_split(gdrf_ctx* c, const float* B, const float* scale, int64_t scale_bs, int64_t n, int64_t rps, int sym, float* slab,
                      int nbatch, int ns, int ntiles, int sidx_b, int sidx_b_stride, hipStream_t s, const void* Ah = nullptr, int sidx_a = -1) {
    if constexpr (std::is_same<T, float>::value) {
      using E = typename SP::E;
      // stored (pre-split) operand: the pieces of W unless the caller names another [piece][row][Mp] array and its block scale
      TNSplitArgs<SP> a{(const E*)(Ah ? Ah : c->Wh), (int64_t)c->ncap * c->Mp, c->Mp, B, c->Mp, scale, scale_bs, n, rps, c->Mp, sym, slab, nbatch, ns,
                        (const float*)c->ssc, sidx_a >= 0 ? sidx_a : SplitLay{c->K}.w(), sidx_b, sidx_b_stride};
      constexpr int lds = 3 * SP::NP * 32 * 128 * 2;            // double-buffered A image + B image
      HIPCHK(hipFuncSetAttribute((const void*)gemm_tn_split_kernel<SP>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      hipLaunchKernelGGL(gemm_tn_split_kernel<SP>, dim3((unsigned)(ntiles * nbatch * ns)), dim3(256), lds, s, a);
      return 0;
    } else {
      return fail(-1, "tn_split", "float arrays only");
    }
  }

  // Wbar on the 16-bit matrix path (f32 contexts only)
  template <class SP>
  static int wbar_split(gdrf_ctx* c, int64_t n, const T* U, hipStream_t s) {
    if constexpr (std::is_same<T, float>::value) {
      using E = typename SP::E;
      const int Mp = c->Mp, K = c->K;
      const SplitLay SL{K};
      const int64_t nb = (int64_t)K * Mp * Mp;
      hipLaunchKernelGGL(split_blocked_kernel<SP>, dim3((unsigned)((nb / 4 + 255) / 256)), dim3(256), 0, s, (const float*)c->Bm, nb, Mp, Mp, (E*)c->Bh, nb,
                         (const float*)c->ssc + SL.b(0));
      BwdWbarSplitArgs<SP> a{(const float*)c->W, (const E*)c->Wh, (int64_t)c->ncap * Mp, n, c->M, Mp, K, (const E*)c->Bh, nb,
                             (const float*)c->vbar, (const float*)c->locbar, c->ldk, (const float*)c->asum, (const float*)U, (float*)c->Wbar,
                             (const float*)c->ssc, c->smx + SL.mx_wbar()};
      const F::WbarPlan pl = F::wbar_plan(form_shape(c, n));
      if (!pl.fits) return fail(-1, "wbar_split", "too many topics for the LDS scale table");
      auto launch = [&](auto kern) {
        HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds));
        hipLaunchKernelGGL(kern, dim3(pl.grid, (unsigned)pl.nslice), dim3(pl.threads), pl.lds, s, a);
        return 0;
      };
      int rc = 0;
      switch (pl.form) {
        case F::WBAR_W1:
          if constexpr (std::is_same<SP, SplitF16>::value)
            rc = pl.R == 2 ? launch(bwd_wbar_f16_w1_kernel<2>) : (pl.R == 4 ? launch(bwd_wbar_f16_w1_kernel<4>) : launch(bwd_wbar_f16_w1_kernel<8>));
          break;
        case F::WBAR_K64:
          if constexpr (std::is_same<SP, SplitF16>::value) {
            if (pl.nslice > 1) { a.slab = (float*)c->slab; a.slab_stride = (int64_t)round_up(n, 256) * Mp; a.nslice = pl.nslice; }
            if ((rc = launch(bwd_wbar_f16_k64_kernel))) return rc;
            if (pl.nslice > 1) {
              const int64_t n4 = n * Mp / 4;
              hipLaunchKernelGGL(wbar_slab_sum_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, (const float*)a.slab, a.slab_stride, pl.nslice, n4,
                                 (float*)c->Wbar, a.wbar_max);
            }
          }
          break;
        case F::WBAR_SPLIT_CC: rc = launch(bwd_wbar_split_cc_kernel<SP>); break;
        case F::WBAR_SPLIT2: rc = launch(bwd_wbar_split_kernel<SP, 2>); break;
        default: rc = launch(bwd_wbar_split_kernel<SP, 1>); break;
      }
      if (rc) return rc;
      c->forms[GDRF_FORM_WBAR] = pl.form; c->forms[GDRF_FORM_WBAR_NSLICE] = pl.nslice;
      LAUNCHCHK("wbar_split");
      return 0;
    } else {
      return fail(-1, "wbar_split", "float arrays only");
    }
  }

  // K_nm in the solve precision with the exact exponential, zero-padded to Mp columns
  static int knm_solve(gdrf_ctx* c, const T* X, int64_t n, hipStream_t s) {
    ScopedTimer tm(c, 1, s);
    const int VE = Vec16<TS>::N;
    const int vpr = (c->Mp + VE - 1) / VE, rpp = vpr <= 256 ? 256 / vpr : 1;
    int64_t blocks = (n + 4 * rpp - 1) / (4 * rpp);
    const int64_t kcap = 256 * 64;
    if (blocks > kcap) blocks = kcap;
    if (blocks < 1) blocks = 1;
    if constexpr (sizeof(TS) == 8) {
      if (c->kind == 0 && vpr <= 256) {
        auto go = [&](auto kern) {
          hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, s, X, n, (const double*)Q(c->Zs), c->M, c->D, c->hyp, (double*)Q(c->Knm),
                             (int64_t)c->Mp);
        };
        if (ard_fwd(c)) { if (c->D <= 2) go(knm_rbf_f64_kernel<T, 2, true, true>); else go(knm_rbf_f64_kernel<T, GDRF_DMAX, true, true>); }
        else { if (c->D <= 2) go(knm_rbf_f64_kernel<T, 2>); else go(knm_rbf_f64_kernel<T, GDRF_DMAX>); }
        LAUNCHCHK("knm_solve");
        return 0;
      }
    }
    if (ard_fwd(c))
      hipLaunchKernelGGL((knm_kernel<TS, T, false, true, true>), dim3((unsigned)blocks), dim3(256), 0, s, X, n, (const TS*)Q(c->Zs), c->M, c->D, c->kind,
                         c->hyp, Q(c->Knm), (int64_t)c->Mp);
    else
      hipLaunchKernelGGL((knm_kernel<TS, T, false>), dim3((unsigned)blocks), dim3(256), 0, s, X, n, (const TS*)Q(c->Zs), c->M, c->D, c->kind,
                         c->hyp, Q(c->Knm), (int64_t)c->Mp);
    LAUNCHCHK("knm_solve");
    return 0;
  }

  // whiten = False: S' = L^-1 S (into c->S / c->ST, and kept in the solve precision in c->uS), u' = L^-1 u (c->Uw, c->uU)
  static int unwhiten_forward(gdrf_ctx* c, const T* U, hipStream_t s) {
    const int Mp = c->Mp, M = c->M, K = c->K;
    const int64_t mm = (int64_t)Mp * Mp;
    int rc;
    if ((rc = join_fact(c, s))) return rc;
    hipLaunchKernelGGL((cast_kernel<T, TS>), dim3((unsigned)((K * mm + 255) / 256)), dim3(256), 0, s, K * mm, (const T*)P(c->ST), Q(c->uSb));
    if ((rc = mm_nt<TS>(c, Q(c->Linv), 0, Q(c->uSb), mm, Q(c->uS), mm, TS(1), K, s))) return rc;        // S'[i][j] = sum_q Linv[i][q] S[q][j]
    dim3 g3((Mp + 255) / 256, Mp, K);
    hipLaunchKernelGGL((cast_with_transpose_kernel<TS, T>), g3, dim3(256), 0, s, (const TS*)Q(c->uS), Mp, P(c->S), P(c->ST));
    hipLaunchKernelGGL((lower_matvec_kernel<TS, T>), dim3((M + 127) / 128, K), dim3(128), 0, s, (const TS*)Q(c->Linv), U, M, Mp, Q(c->uU),
                       (T*)c->Uw);
    return 0;
  }

  // the tail of the per-row ELBO stage: `grid` workgroups' Phi-bar partials -> the phibar block of red_T; with their four scalars -> red_d[0..4)
  static void phibar_reduce(gdrf_ctx* c, const T* parts, int64_t grid, T* redT, hipStream_t s) {
    const int64_t kv = (int64_t)c->K * c->V;
    hipLaunchKernelGGL(reduce_parts_kernel<T>, dim3((unsigned)((kv + 255) / 256)), dim3(256), 0, s, parts, grid, kv, redT + red_lay(c).phibar);
  }
  static void rows_reduce(gdrf_ctx* c, const T* parts, int64_t grid, T* redT, double* redd, hipStream_t s, int64_t nparts = -1) {
    hipLaunchKernelGGL(reduce_dparts_kernel, dim3(1), dim3(1024), 0, s, c->dpart, grid, 4, redd);
    phibar_reduce(c, parts, nparts < 0 ? grid : nparts, redT, s);
  }

  // ---- the vocabulary-streamed row form (gdrf_set_rows_form(ctx, 1), rows_vstream.h) ----
  // (with a bound CSR matrix the Phi-bar slots do not bound the grid: up to 1024 workgroups)
  static int vs_grid(const gdrf_ctx* c, int64_t n, bool counts = true) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((n + 63) / 64, c->csr_crow && counts ? 1024 : c->vs_gcap));
  }
  // where the streamed call sites find the Phi-bar partials and the link constants: the streamed kernel's `grid` slots, or the sparse form's one
  static const T* vs_parts(const gdrf_ctx* c) { return (const T*)(c->csr_crow ? c->csr_slot : c->vs_part); }
  static int64_t vs_nparts(const gdrf_ctx* c, int64_t grid) { return c->csr_crow ? 1 : grid; }
  static const T* vs_cparts(const gdrf_ctx* c) { return (const T*)(c->csr_crow ? c->csr_cpart : c->vs_cpart); }

  // ---- the sparse row form (rows_csr.h): rows [row_off, row_off + n) of the bound CSR matrix in place of rows_vstream_kernel ----
  template <int MODE>
  static int csr_launch(gdrf_ctx* c, int64_t n, int grid, const T* src, int64_t sk, int64_t sn, int64_t row_off, T* dst, int64_t dld,
                        double* dpart, int dacc, hipStream_t s, bool new_phi) {
    constexpr bool ELBO = MODE == VS_SOFTMAX || MODE == VS_LINK;
    const int K = c->K, V = c->V, Kp = (int)round_up(K, K <= 8 ? 8 : 16);      // Phi^T rows padded to sparse_form's LG
    const int64_t nnz = c->csr_nnz;
    if (row_off < 0 || row_off + n > c->csr_n) return fail(-1, "rows_csr", "rows outside the bound CSR count matrix");
    if (ELBO && nnz > 0 && !c->csr_ccol) return fail(-1, "rows_csr", "a step needs the column grouping (ccol_dev, cperm_dev) of the bound CSR count matrix");
    if (int rc = csr_ensure(c)) return rc;
    if (ELBO) {
      if (int rc = csr_grow(c, nnz)) return rc;
      if (c->csr_fresh) {            // once per binding: the row of every entry, the column segments
        hipLaunchKernelGGL(csr_entry_rows_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 15) / 16, 4096))), dim3(256), 0, s, c->csr_crow, n,
                           nnz, c->csr_erow);
        if (nnz > 0) hipLaunchKernelGGL(csr_segscan_kernel, dim3(1), dim3(1024), 0, s, c->csr_ccol, V, c->csr_segoff, c->csr_segcol);
        c->csr_fresh = 0;
      }
    }
    const int64_t nt = (int64_t)V * Kp;
    if (new_phi) {                   // Phi^T of this call's Phi; the later pieces of a gdrf_predict call reuse it
      hipLaunchKernelGGL(csr_transpose_phi_kernel<T>, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, (const T*)P(c->phi), K, Kp, V, (T*)c->csr_phiT);
    }
    sparse_form(K, [&](auto fm) {
      using F = decltype(fm);
      hipLaunchKernelGGL((rows_csr_kernel<T, MODE, F::LG, F::KJ>), dim3(grid), dim3(256), 0, s, n, K, Kp, V, nnz, src, sk, sn, c->csr_crow + row_off,
                         c->csr_col, c->csr_val, (const T*)c->csr_phiT, (const T*)c->vs_rs, dst, dld, dpart, dacc, (T*)c->csr_thN, (T*)c->csr_pb,
                         (T*)c->csr_cn);
      return 0;
    });
    if constexpr (MODE == VS_LINK)
      hipLaunchKernelGGL(csr_link_const_kernel<T>, dim3(grid), dim3(128), 0, s, n, K, (const T*)c->csr_thN, (const T*)c->csr_cn, (T*)c->csr_cpart);
    if constexpr (ELBO) {
      if (nnz > 0) {
        const int64_t nseg = V + nnz / CSR_SEG + 1;         // an upper bound of the table's length; the kernel reads the length itself
        sparse_form(K, [&](auto fm) {
          using F = decltype(fm);
          hipLaunchKernelGGL((csr_phibar_seg_kernel<T, F::LG, F::KJ>), dim3((unsigned)((nseg * F::LG + 255) / 256)), dim3(256), 0, s, K, V, nnz, n,
                             c->csr_ccol, c->csr_cperm, (const int64_t*)c->csr_segoff, (const int32_t*)c->csr_segcol, (const int32_t*)c->csr_erow,
                             (const T*)c->csr_pb, (const T*)c->csr_thN, (T*)c->csr_parts);
          return 0;
        });
        hipLaunchKernelGGL(csr_phibar_combine_kernel<T>, dim3((unsigned)(((int64_t)K * V + 255) / 256)), dim3(256), 0, s, K, V,
                           (const int64_t*)c->csr_segoff, (const T*)c->csr_parts, (T*)c->csr_slot);
      } else {
        HIPCHK(hipMemsetAsync(c->csr_slot, 0, (size_t)K * V * c->esz, s));
      }
    }
    LAUNCHCHK("rows_csr");
    return 0;
  }

  template <int MODE>
  static int vs_launch(gdrf_ctx* c, int64_t n, int grid, const T* src, int64_t sk, int64_t sn, const int32_t* ws, T* dst, int64_t dld,
                       double* dpart, int dacc, hipStream_t s, int64_t row_off = 0) {
    if constexpr (MODE != VS_WORDP) {
      if (c->csr_crow) return csr_launch<MODE>(c, n, grid, src, sk, sn, row_off, dst, dld, dpart, dacc, s, row_off == 0);
    }
    const size_t lds = vs_lds<T>(c->K);
    auto go = [&](auto kern) {
      return launch_lds(kern, dim3(grid), dim3(256), lds, s, n, c->K, c->V, src, sk, sn, ws, (const T*)P(c->phi), (const T*)c->vs_rs, dst, dld, dpart, dacc,
                        (T*)c->vs_part, (T*)c->vs_cpart);
    };
    int rc;
    if constexpr (MODE == VS_SOFTMAX || MODE == VS_LINK) rc = c->K <= 32 ? go(rows_vstream_kernel<T, MODE, 8>) : go(rows_vstream_kernel<T, MODE, 32>);
    else rc = go(rows_vstream_kernel<T, MODE, 1>);
    if (rc) return rc;
    LAUNCHCHK("rows_vstream");
    return 0;
  }
  // the V-free head and tail of the row stage (rows_lds.h) on the streamed form's grid: q and mu from one side's (qpart, loc, tt, mean);
  // the Normal sites and the row-local backward from mub = mubar (K, mub_ld)
  static void rows_mu(gdrf_ctx* c, int64_t n, int grid, const T* eps, const T* qpart, const T* loc, const T* tt, const T* mean, int64_t msk,
                      int64_t msn, hipStream_t s) {
    hipLaunchKernelGGL(rows_mu_kernel<T>, dim3(grid), dim3(64), 0, s, n, c->K, c->hyp, qpart, nct<TS>(c), loc, tt, eps, c->ldk, n, mean, msk, msn,
                       P(c->q), P(c->mu));
  }
  static void rows_sites(gdrf_ctx* c, int64_t n, int grid, const T* eps, const T* mub, int64_t mub_ld, hipStream_t s) {
    hipLaunchKernelGGL(rows_sites_kernel<T>, dim3(grid), dim3(64), 0, s, n, c->K, c->hyp, (const T*)P(c->qpart), nct<TS>(c), (const T*)P(c->tt), eps,
                       c->ldk, n, mub, mub_ld, P(c->vbar), P(c->locbar), P(c->asum), c->dpart);
  }
  // gdrf_step_local's row terms in form 1: q, mu ; Phi row sums ; theta = softmax(mu) through the streamed likelihood -> mubar ; the
  // Normal sites and the row-local backward ; reductions
  static int rows_streamed(gdrf_ctx* c, const int32_t* ws, const T* eps, int64_t n, T* redT, double* redd, hipStream_t s) {
    const int K = c->K, V = c->V;
    if (int rc = vs_ensure(c)) return rc;
    const int G = vs_grid(c, n);
    rows_mu(c, n, G, eps, P(c->qpart), P(c->loc), P(c->tt), (const T*)c->mean, c->mean_sk, c->mean_sn, s);
    hipLaunchKernelGGL(vs_rowsum_kernel<T>, dim3(K), dim3(256), 0, s, P(c->phi), K, V, (T*)c->vs_rs);
    if (int rc = vs_launch<VS_SOFTMAX>(c, n, G, P(c->mu), c->ldk, 1, ws, (T*)c->vs_tmp, c->ldk, c->dpart, 0, s)) return rc;
    rows_sites(c, n, G, eps, (const T*)c->vs_tmp, c->ldk, s);
    LAUNCHCHK("elbo_rows (streamed)");
    rows_reduce(c, vs_parts(c), G, redT, redd, s, vs_nparts(c, G));
    return 0;
  }

  // The backward through K_nm (kernels_n.h: BwdKnmProb) on `nb` workgroups: the three hyper-parameter partials per workgroup into c->dpart, with
  // LZ the inducing-input partials (c->zpart), with ARD the per-axis ones (c->apart), with PER the period ones behind them.
  template <bool LZ, bool ARD, bool PER>
  static void bwd_knm(gdrf_ctx* c, const T* X, const T* Xr, int64_t n, int64_t nb, hipStream_t s) {
    using Prob = BwdKnmProb<TS, T, LZ, ARD, PER>;
    Prob p{{}, {}, P(c->Wbar), n, c->M, c->Mp, c->D, c->kind, (const TS*)Q(c->LinvT), (const TS*)Q(c->Knm), X, (const TS*)Q(c->Zs), c->hyp, c->dpart,
           LZ ? c->zpart : nullptr, ARD ? c->apart : nullptr, PER ? Xr : nullptr, PER ? (const TS*)Q(c->Zph) : nullptr};
    // capped at 160 registers where the LDS-transposed f64 epilogue runs: two of its waves then share a SIMD with one wave of
    // G^T's TN contraction on the side stream (192 registers), which fills this kernel's stalls instead of queueing behind it
    if constexpr (!LZ) {
      if (sizeof(TS) == 8) { hipLaunchKernelGGL((gemm_nt_kernel_v160<TS, Prob>), dim3((unsigned)nb), dim3(256), CS::LDS_BYTES, s, p); return; }
    }
    hipLaunchKernelGGL((gemm_nt_kernel<TS, Prob>), dim3((unsigned)nb), dim3(256), CS::LDS_BYTES, s, p);
  }

  // ---- the stages of one evaluation: step_inputs, the parameter transforms, the forward over the rows (K_nm, W, loc, tt),
  // the per-row terms, the backward over the rows.  step_local runs them in that order; step_local2, step_local_link and the predictive
  // entry points compose the ones they need.
  // u_loc as the stages behind step_transforms read it: whitened contexts keep it in the parameters, unwhitened ones in c->Uw (u' = L^-1 u)
  static const T* step_u(const gdrf_ctx* c, const T* params) { return c->unwhitened ? (const T*)c->Uw : params + param_lay(c).uloc; }
  static int64_t row_tiles(int64_t n) { return (n + GDRF_TILE - 1) / GDRF_TILE; }

  // S_k, S_k^T, Phi, the padded u_loc, B_k = S_k S_k^T and the block scales of the split modes.  Caller's stream.
  static int step_transforms(gdrf_ctx* c, const T* params, hipStream_t s) {
    const int Mp = c->Mp, M = c->M, K = c->K, V = c->V;
    const int64_t mm = (int64_t)Mp * Mp;
    const ParamLay pl = param_lay(c);
    int rc;
    ScopedTimer tm(c, 2, s);
    dim3 g3((Mp + 255) / 256, Mp, K);
    hipLaunchKernelGGL(build_s_kernel<T>, g3, dim3(256), 0, s, params + pl.S, M, Mp, P(c->S), P(c->ST));
    hipLaunchKernelGGL(build_phi_kernel<T>, dim3(K), dim3(64), 0, s, params + pl.phi, K, V, P(c->phi));
    if (c->unwhitened && (rc = unwhiten_forward(c, params + pl.uloc, s))) return rc;     // S, ST now hold S' = L^-1 S; c->Uw holds u' = L^-1 u
    hipLaunchKernelGGL(build_upad_kernel<T>, dim3((Mp + 255) / 256, GDRF_TILE), dim3(256), 0, s, step_u(c, params), K, M, Mp, P(c->Upad));
    if (!c->Tst && (rc = mm_nt<T>(c, P(c->S), mm, P(c->S), mm, P(c->Bm), mm, T(1), K, s))) return rc;      // B_k = S_k S_k^T
    if constexpr (std::is_same<T, float>::value) {
      if (c->split) {            // block scales of W (from the variance), B_k and S_k^T (from their maxima)
        const SplitLay SL{K};
        HIPCHK(hipMemsetAsync(c->smx, 0, (size_t)SL.nmax() * sizeof(unsigned), s));
        if (c->split == 2) {
          hipLaunchKernelGGL(absmax_batched_kernel, dim3(64, K), dim3(256), 0, s, (const float*)c->Bm, mm, mm, c->smx + SL.mx_b(0));
          hipLaunchKernelGGL(absmax_batched_kernel, dim3(64, K), dim3(256), 0, s, (const float*)c->ST, mm, mm, c->smx + SL.mx_st(0));
        }
        split_scales(c, SPLIT_SC_W | SPLIT_SC_BST, s);
      }
    }
    return 0;
  }

  // K_nm, W, loc and tt at the rows r.X.  W and tt on the caller's stream; loc (and, with want_dk, the dK_nm pieces of the hyper-TN
  // backward) on the side stream behind ev_fork; the caller's stream waits for loc (ev_loc) before it returns, not for the pieces.
  static int step_forward(gdrf_ctx* c, const StepRows& r, int64_t n, hipStream_t s, bool want_dk) {
    const int Mp = c->Mp, M = c->M, K = c->K;
    const int64_t ldk = c->ldk, rtiles = row_tiles(n);
    int rc;
    // (1) W = Knm Linv^T in the solve precision, stored in the N-side precision
    {
      if ((rc = knm_solve(c, r.X, n, s))) return rc;
      if ((rc = join_fact(c, s))) return rc;          // W needs L^-1
      ScopedTimer tm(c, 3, s);
      FwdWProb<TS, T> p{{}, {}, (const TS*)Q(c->Knm), n, Mp, (const TS*)Q(c->Linv), P(c->W), P(c->qpart), ldk};
      if (c->split && sizeof(TS) == 8 && sizeof(T) == 4) {      // pieces of W from the same epilogue
        p.Wh = c->Wh; p.wh_stride = (int64_t)c->ncap * Mp; p.wh_mode = c->split; p.wh_scale = c->ssc + SplitLay{K}.w();
      }
      hipLaunchKernelGGL((gemm_nt_kernel<TS, FwdWProb<TS, T>>), dim3(nt_xcd_row_grid(rtiles, nct<TS>(c))), dim3(256), CS::LDS_BYTES, s, p);
    }
    // loc = W U^T, on the side stream beside fwd_t (both only read W)
    HIPCHK(hipEventRecord(c->ev_fork, s));
    HIPCHK(hipStreamWaitEvent(c->side, c->ev_fork, 0));
    {
      ScopedTimer tm(c, 4, c->side);
      const F::LocPlan pl = F::loc_plan(form_shape(c, n));
      switch (pl.form) {
        case F::LOC_ROWS:
          if ((rc = launch_lds(loc_rows_kernel<T>, dim3((unsigned)pl.blocks), dim3(256), pl.lds, c->side, (const T*)P(c->W), n, Mp, K, (const T*)P(c->Upad),
                               P(c->loc), ldk))) return rc;
          break;
        case F::LOC_GEMM_NT_WIDE:       // f64 with K > 64: two column tiles
          if constexpr (sizeof(T) == 8) {
            LocProb<T, true> p{{}, {}, {}, P(c->W), n, Mp, K, P(c->Upad), P(c->loc), ldk};
            hipLaunchKernelGGL((gemm_nt_kernel<T, LocProb<T, true>>), dim3((unsigned)pl.blocks), dim3(256), C::LDS_BYTES, c->side, p);
          }
          break;
        default: {
          LocProb<T> p{{}, {}, {}, P(c->W), n, Mp, K, P(c->Upad), P(c->loc), ldk};
          hipLaunchKernelGGL((gemm_nt_kernel<T, LocProb<T>>), dim3((unsigned)pl.blocks), dim3(256), C::LDS_BYTES, c->side, p);
        }
      }
      c->forms[GDRF_FORM_LOC] = pl.form;
    }
    HIPCHK(hipEventRecord(c->ev_loc, c->side));
    if constexpr (std::is_same<T, float>::value && sizeof(TS) == 8) {
      if (hyper_tn_on(c) && want_dk) {
        // pieces of dK_nm / d log(lengthscale) for the backward's Hd = dK^T Wbar; on the side stream behind loc: the main stream does not wait for it
        const int vpr = Mp / 8, rpp = 256 / vpr;
        const int64_t blocks = std::min<int64_t>((n + rpp - 1) / rpp, 256 * 16);
        if (!c->dKh && (rc = ctx_alloc(c, &c->dKh, (size_t)2 * c->ncap * Mp * 2, "hipMalloc(dKh)"))) return rc;
        _Float16* dkh = (_Float16*)c->dKh;
        const float* dsc = (const float*)c->ssc + SplitLay{K}.dk();
        hipLaunchKernelGGL((c->D <= 2 ? dk_pieces_kernel<T, 2> : dk_pieces_kernel<T, GDRF_DMAX>), dim3((unsigned)blocks), dim3(256), 0, c->side, r.X, n,
                           (const double*)c->Zs, M, c->D, c->kind, c->hyp, dkh, (int64_t)c->ncap * Mp, Mp, dsc);
        LAUNCHCHK("dk_pieces");
      }
    }
    // (2) tt_kn = ||S_k^T w_n||^2
    if (c->split) {
      if ((rc = BY_SPLIT(c, fwd_t_split, c, n, s))) return rc;
    } else {
      ScopedTimer tm(c, 5, s);
      FwdTProb<T> p{{K}, {}, {}, P(c->W), n, Mp, P(c->ST), P(c->tt), ldk, P(c->Tst), c->t_bs, c->t_ts};
      hipLaunchKernelGGL((gemm_nt_kernel<T, FwdTProb<T>>), dim3((unsigned)(8 * K * ((rtiles + 7) / 8))), dim3(256), C::LDS_BYTES, s, p);
      c->forms[GDRF_FORM_FWD_T] = F::FWD_T_GEMM_NT; c->forms[GDRF_FORM_FWD_T_KG] = 0;
    }
    LAUNCHCHK("forward");
    HIPCHK(hipStreamWaitEvent(s, c->ev_loc, 0));
    return 0;
  }

  // per-row ELBO terms and row-local backward: the streamed or sparse route, or one of the two forms with Phi in LDS.  Caller's stream.
  static int step_rows(gdrf_ctx* c, const int32_t* ws, const T* eps, int64_t n, T* redT, double* redd, hipStream_t s) {
    const int K = c->K, V = c->V;
    const int64_t ldk = c->ldk;
    int rc;
    ScopedTimer tm(c, 6, s);
    const F::RowsPlan pl = F::rows_plan(form_shape(c, n));
    if (pl.form == F::ROWS_STREAMED) {
      if ((rc = rows_streamed(c, ws, eps, n, redT, redd, s))) return rc;
    } else {
      if ((rc = phibar_part_ensure(c))) return rc;
      if (!pl.fits)
        return fail(-1, "gdrf_step_local", "num_topic_categories x num_observation_categories too large: the row kernel keeps the "
                                           "(K, V) word-topic matrix and its gradient in LDS (2*K*V + 32*(2K + V + 3) elements <= 150 KB); "
                                           GDRF_STREAMED_HINT);
      auto rows = [&](auto kern) {         // the LDS row forms take the same arguments
        return launch_lds(kern, dim3(pl.egrid), dim3(pl.threads), pl.lds, s, n, K, V, c->hyp, P(c->qpart), nct<TS>(c), P(c->loc), P(c->tt), eps, ldk, n, ws,
                          P(c->phi), (const T*)c->mean, c->mean_sk, c->mean_sn, P(c->q), P(c->vbar), P(c->locbar), P(c->asum), P(c->mu), c->dpart,
                          P(c->phibar_part));
      };
      if (pl.form == F::ROWS_MFMA) {       // 16 rows per wave (rows_mfma.h)
        if ((rc = rows(pl.nkt == 1 ? (pl.nvt == 2 ? elbo_rows_mfma_kernel<T, 1, 2> : elbo_rows_mfma_kernel<T, 1, 4>)
                                   : (pl.nvt == 2 ? elbo_rows_mfma_kernel<T, 2, 2> : elbo_rows_mfma_kernel<T, 2, 4>)))) return rc;
        LAUNCHCHK("elbo_rows (mfma)");
      } else {                             // one thread per row, K <= GDRF_KMAX topics in registers
        if ((rc = rows(pl.kreg ? elbo_rows_kernel<T, true> : elbo_rows_kernel<T, false>))) return rc;
        LAUNCHCHK("elbo_rows");
      }
      rows_reduce(c, P(c->phibar_part), pl.egrid, redT, redd, s);
    }
    c->forms[GDRF_FORM_ROWS] = pl.form; c->forms[GDRF_FORM_ROWS_KT] = pl.nkt; c->forms[GDRF_FORM_ROWS_VT] = pl.nvt;
    return 0;
  }

  // ---- the pieces of step_backward, in its order.  None of them records or awaits an event: step_backward does.
  // block scale of diag(vbar_k) W, the scaled operand of the A_k contraction.  Stream s (main), no event.
  static int bwd_vscale(gdrf_ctx* c, int64_t n, hipStream_t s) {
    if constexpr (std::is_same<T, float>::value) {
      if (c->split) {
        const SplitLay SL{c->K};
        if (c->split == 2) {
          HIPCHK(hipMemsetAsync(c->smx + SL.mx_v(0), 0, (size_t)c->K * sizeof(unsigned), s));
          HIPCHK(hipMemsetAsync(c->smx + SL.mx_wbar(), 0, sizeof(unsigned), s));
          hipLaunchKernelGGL(absmax_batched_kernel, dim3(64, c->K), dim3(256), 0, s, (const float*)c->vbar, n, c->ldk, c->smx + SL.mx_v(0));
        }
        split_scales(c, SPLIT_SC_V, s);
      }
    }
    return 0;
  }
  // ubar = locbar W needs only the row kernel's locbar: BESIDE the Wbar contraction (a vector / HBM pass next to a matrix-pipe kernel that
  // leaves half of each SIMD's registers free) instead of inside bwd_knm with G^T.  Stream ss (side), behind ev_fork.
  static int bwd_ubar(gdrf_ctx* c, int64_t n, T* redT, hipStream_t ss) {
    const int Mp = c->Mp, K = c->K;
    ScopedTimer tm(c, 12, ss);
    const auto [kq, rpb, nb] = F::ubar_plan(form_shape(c, n));
    if (nb > c->ubar_blocks_cap) return fail(-1, "gdrf_step_local", "ubar partial buffer too small");
    c->forms[GDRF_FORM_UBAR_Q4] = kq;
    hipLaunchKernelGGL((kq == 1 ? ubar_part_kernel<T, 1> : kq == 2 ? ubar_part_kernel<T, 2> : kq == 3 ? ubar_part_kernel<T, 3> : ubar_part_kernel<T, 4>),
                       dim3((unsigned)nb, (Mp + 255) / 256), dim3(256), 0, ss, P(c->W), n, Mp, K, P(c->locbar), c->ldk, rpb, P(c->ubar_part));
    hipLaunchKernelGGL(reduce_parts_kernel<T>, dim3((K * Mp + 255) / 256), dim3(256), 0, ss, P(c->ubar_part), nb, (int64_t)K * Mp, redT + red_lay(c).ubar);
    return 0;
  }
  // (3) Wbar.  Stream s (main), no event: the side stream's G^T and hyper-TN wait for it through ev_fork2.
  static int bwd_wbar(gdrf_ctx* c, int64_t n, const T* U, hipStream_t s) {
    const int Mp = c->Mp, M = c->M, K = c->K;
    const int64_t ldk = c->ldk, rtiles = row_tiles(n);
    int rc;
    ScopedTimer tm(c, 7, s);
    const size_t lds = C::LDS_BYTES + (size_t)K * GDRF_TILE * sizeof(T);
    const dim3 grid(c->Tst ? nt_xcd_pair_grid(rtiles, nct<T>(c)) : (unsigned)round_up(rtiles * nct<T>(c), 8));
    if (c->Tst) {
      BwdWbarTProb<T> p{{}, {}, P(c->Tst), c->t_bs, c->t_ts, P(c->W), n, M, Mp, K, P(c->S), P(c->vbar), P(c->locbar), ldk,
                        P(c->asum), U, P(c->Wbar)};
      if ((rc = launch_lds(gemm_nt_kernel<T, BwdWbarTProb<T>>, grid, dim3(256), lds, s, p))) return rc;
      c->forms[GDRF_FORM_WBAR] = F::WBAR_GEMM_NT_T; c->forms[GDRF_FORM_WBAR_NSLICE] = 1;
    } else if (c->split) {
      if ((rc = BY_SPLIT(c, wbar_split, c, n, U, s))) return rc;
      split_scales(c, SPLIT_SC_WBAR, s);           // max |Wbar| came out of the epilogue: scale of the G^T contraction's operand
    } else {
      BwdWbarProb<T> p{{}, {}, P(c->W), n, M, Mp, K, P(c->Bm), P(c->vbar), P(c->locbar), ldk, P(c->asum), U, P(c->Wbar)};
      if ((rc = launch_lds(gemm_nt_kernel<T, BwdWbarProb<T>>, grid, dim3(256), lds, s, p))) return rc;
      c->forms[GDRF_FORM_WBAR] = F::WBAR_GEMM_NT; c->forms[GDRF_FORM_WBAR_NSLICE] = 1;
    }
    return 0;
  }
  // G^T = W^T Wbar, where it fills the last-round tails of bwd_knm and the A_k contraction on the main stream.  Stream ss (side), behind ev_fork2.
  static int bwd_gt(gdrf_ctx* c, int64_t n, T* redT, hipStream_t ss) {
    const int Mp = c->Mp, K = c->K;
    const auto [form, ns, rps] = F::gt_plan(form_shape(c, n));
    T* slab_gt = P(c->slab) + (int64_t)c->nsplit_cap * K * Mp * Mp;           // the (K+1)-th batch region of the slab buffer
    TNArgs<T> b{P(c->W), Mp, P(c->Wbar), Mp, nullptr, 0, n, rps, Mp, 0, slab_gt, 1, ns};
    { ScopedTimer tm(c, 10, ss);
      c->forms[GDRF_FORM_GT] = form;
      if (form == F::GT_TN_SPLIT) {
        const int ib = SplitLay{K}.wbar();
        if (int rc = BY_SPLIT(c, tn_split, c, (const float*)c->Wbar, nullptr, 0, n, rps, 0, (float*)slab_gt, 1, ns, c->nt * c->nt, ib, 0, ss)) return rc;
      } else {
        hipLaunchKernelGGL(gemm_tn_kernel<T>, dim3((unsigned)(c->nt * c->nt * ns)), dim3(256), TNCfg<T>::LDS_BYTES, ss, b);
      } }
    { ScopedTimer tm(c, 11, ss);
      dim3 gr1((Mp + 255) / 256, Mp, 1);
      hipLaunchKernelGGL(reduce_slabs_kernel<T>, gr1, dim3(256), 0, ss, (const T*)slab_gt, ns, 1, Mp, 0, redT + red_lay(c).GT); }
    return 0;
  }
  // (4) kernel hyper-parameter partials through K_nm, in one of two forms.
  // Hyper-TN (hyper_tn.h): stream ss (side), behind G^T: Hd = dK^T Wbar on the same TN kernel (slab batch K + 1), its contraction with L^-1
  // in double -> red_d[5]; sum Wbar o W -> red_d[4]; red_d[6] = 0.  No backward solve GEMM.
  // Otherwise the bwd_knm fan and its reductions: stream s (main), no event.
  static int bwd_hyper(gdrf_ctx* c, const StepRows& r, int64_t n, double* redd, hipStream_t s, hipStream_t ss) {
    const int Mp = c->Mp, M = c->M;
    const auto [form, ns, rps] = F::hyper_plan(form_shape(c, n));
    c->forms[GDRF_FORM_HYPER] = form;
    if constexpr (std::is_same<T, float>::value && sizeof(TS) == 8) {
      if (form == F::HYPER_TN) {
        ScopedTimer tm(c, 8, ss);
        float* slab_hd = (float*)c->slab + (int64_t)c->nsplit_cap * (c->K + 1) * Mp * Mp;
        const SplitLay SL{c->K};
        if (int rc = tn_split<SplitF16>(c, (const float*)c->Wbar, nullptr, 0, n, rps, 0, slab_hd, 1, ns, c->nt * c->nt, SL.wbar(), 0, ss, c->dKh, SL.dk())) return rc;
        hipLaunchKernelGGL(slab_linvt_dot_kernel<TS>, dim3((unsigned)M), dim3(256), 0, ss, (const float*)slab_hd, ns, Mp, M, (const TS*)Q(c->LinvT), c->hpart);
        hipLaunchKernelGGL(reduce_dparts_kernel, dim3(1), dim3(1024), 0, ss, c->hpart, (int64_t)M, 1, redd + 5);
        hipLaunchKernelGGL(wbar_w_dot_kernel<T>, dim3(2048), dim3(256), 0, ss, (const T*)P(c->Wbar), (const T*)P(c->W), n, Mp, c->hpart + Mp);
        hipLaunchKernelGGL(reduce_dparts_kernel, dim3(1), dim3(1024), 0, ss, c->hpart + Mp, (int64_t)2048, 1, redd + 4);
        HIPCHK(hipMemsetAsync(redd + 6, 0, sizeof(double), ss));
        LAUNCHCHK("hyper_tn");
        return 0;
      }
    }
    ScopedTimer tm(c, 8, s);
    const int64_t rtiles = row_tiles(n), nb = nt_xcd_row_grid(rtiles, nct<TS>(c));
    if (3 * nb > c->dpart_len) return fail(-1, "gdrf_step_local", "n_local exceeds the context capacity");
    const T *X = r.X, *Xr = r.Xr;
    if (c->per) { if (c->learn_z) bwd_knm<true, true, true>(c, X, Xr, n, nb, s); else bwd_knm<false, true, true>(c, X, Xr, n, nb, s); }
    else if (c->ard) { if (c->learn_z) bwd_knm<true, true, false>(c, X, Xr, n, nb, s); else bwd_knm<false, true, false>(c, X, Xr, n, nb, s); }
    else if (c->learn_z) bwd_knm<true, false, false>(c, X, Xr, n, nb, s);
    else bwd_knm<false, false, false>(c, X, Xr, n, nb, s);
    if (c->learn_z)
      hipLaunchKernelGGL(reduce_parts_kernel<double>, dim3((unsigned)((M * c->D + 255) / 256)), dim3(256), 0, s, (const double*)c->zpart, rtiles,
                         (int64_t)M * c->D, redd + 8);
    // red_d[8 + M D ..): the ARD tail; periodic and product contexts: the coordinate sums, then the period sums
    if (c->per || c->ard)
      hipLaunchKernelGGL(reduce_dparts_kernel, dim3(1), dim3(1024), 0, s, c->apart, nb, c->D + (c->per ? c->npair : 0), redd + 8 + (int64_t)M * c->D);
    hipLaunchKernelGGL(reduce_dparts_kernel, dim3(1), dim3(1024), 0, s, c->dpart, nb, 3, redd + 4);      // red_d[4..6]
    return 0;
  }
  // (5) A_k = W^T diag(vbar_k) W.  It needs W and vbar only - not Wbar - but stays on stream s (main), no event: beside the f64 backward GEMM
  // the two kernels time-slice the CUs instead of filling each other's stalls
  static int bwd_ak(gdrf_ctx* c, int64_t n, T* redT, hipStream_t s) {
    const int Mp = c->Mp, K = c->K;
    const int64_t ldk = c->ldk;
    int rc;
    const F::AkPlan pl = F::ak_plan(form_shape(c, n));
    c->forms[GDRF_FORM_AK] = pl.form; c->forms[GDRF_FORM_AK_KGROUPS] = pl.kgroups;
    { ScopedTimer tm(c, 9, s);
      switch (pl.form) {
        case F::AK_W2:           // one-wave-per-SIMD form (gemm_tn_topics1.h): 128 rows per wave
          if constexpr (std::is_same<T, float>::value) {
            const SplitLay SL{K};
            const int ntl = tnt_ntiles(Mp), kgroups = pl.kgroups, ns1 = pl.ns1;
            const int64_t lds64 = round_up(c->ncap, 64);
            hipLaunchKernelGGL(tn1_scale_rows_kernel, dim3(256, K), dim3(256), 0, s, (const float*)c->vbar, ldk, n, (float*)c->vbs, lds64,
                               (const float*)c->ssc, SL.v(0));
            TNTopicsArgs t1{(const _Float16*)c->Wh, (int64_t)c->ncap * Mp, Mp, (const float*)c->W, Mp, (const float*)c->vbs, lds64, n, pl.rps1, Mp,
                            (float*)c->slab, K, ns1, ntl, (const float*)c->ssc, SL.w(), SL.v(0)};
            // two launches: the tiles whose upper 64 rows lie above the diagonal (J = 2 I + 1) multiply half the A tiles (gemm_tn_topics1.h)
            const int nth = tn2_ntiles_half(Mp);
            TNTopicsArgs t0 = t1, t4 = t1;
            t0.ntiles = ntl - nth; t4.ntiles = nth;
            HIPCHK(hipFuncSetAttribute((const void*)tn_topics_w2_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, tn2_lds_bytes()));
            HIPCHK(hipFuncSetAttribute((const void*)tn_topics_w2_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, tn2_lds_bytes()));
            if (t0.ntiles > 0) hipLaunchKernelGGL(tn_topics_w2_kernel<0>, dim3((unsigned)(t0.ntiles * kgroups * ns1)), dim3(256), tn2_lds_bytes(), s, t0);
            if (t4.ntiles > 0) hipLaunchKernelGGL(tn_topics_w2_kernel<4>, dim3((unsigned)(t4.ntiles * kgroups * ns1)), dim3(256), tn2_lds_bytes(), s, t4);
            LAUNCHCHK("tn_topics_w2");
          }
          break;
        case F::AK_TN_TOPICS:    // two waves per SIMD (gemm_tn_topics.h)
          if constexpr (std::is_same<T, float>::value) {
            const SplitLay SL{K};
            const int ntl = tnt_ntiles(Mp);
            TNTopicsArgs ta{(const _Float16*)c->Wh, (int64_t)c->ncap * Mp, Mp, (const float*)c->W, Mp, (const float*)c->vbar, ldk, n, pl.rpst, Mp,
                            (float*)c->slab, K, pl.nst, ntl, (const float*)c->ssc, SL.w(), SL.v(0)};
            HIPCHK(hipFuncSetAttribute((const void*)tn_topics_f16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, tnt_lds_bytes()));
            hipLaunchKernelGGL(tn_topics_f16_kernel, dim3((unsigned)(ntl * pl.kgroups * pl.nst)), dim3(512), tnt_lds_bytes(), s, ta);
            LAUNCHCHK("tn_topics");
          }
          break;
        case F::AK_TN_SPLIT: {   // bf16x6
          const int ib = SplitLay{K}.v(0), ntl = c->nt * (c->nt + 1) / 2;
          if ((rc = tn_split<SplitBf16>(c, (const float*)c->W, (const float*)c->vbar, ldk, n, pl.rps, 1, (float*)c->slab, K, pl.ns, ntl, ib, 2, s))) return rc;
          break;
        }
        default: {
          TNArgs<T> a{P(c->W), Mp, P(c->W), Mp, P(c->vbar), ldk, n, pl.rps, Mp, 1, P(c->slab), K, pl.ns};
          hipLaunchKernelGGL(gemm_tn_kernel<T>, dim3((unsigned)(c->nt * (c->nt + 1) / 2 * K * pl.ns)), dim3(256), TNCfg<T>::LDS_BYTES, s, a);
        }
      } }
    const int red_ns = pl.red_ns, red_qd = pl.red_qd;
    { ScopedTimer tm(c, 11, s);
      dim3 gr((Mp + 255) / 256, Mp, K);
      hipLaunchKernelGGL(reduce_slabs_kernel<T>, gr, dim3(256), 0, s, P(c->slab), red_ns, K, Mp, 1, redT + red_lay(c).A, red_qd); }
    return 0;
  }

  // The backward over the rows: ubar, A_k, G^T into redT and the K_nm hyper-parameter partials into redd, from the row stage's vbar, locbar
  // and asum and the forward's W.  Every event of the backward is recorded and awaited here:
  //   main s : vscale | fork ------- wbar | fork2 ---------- (hyper: bwd_knm fan) - ak ----- wait(join)
  //   side   :         wait(fork) ubar     wait(fork2) gt - (hyper: TN form) ----- join
  static int step_backward(gdrf_ctx* c, const StepRows& r, int64_t n, const T* params, T* redT, double* redd, hipStream_t s) {
    int rc;
    if ((rc = bwd_vscale(c, n, s))) return rc;
    HIPCHK(hipEventRecord(c->ev_fork, s));
    HIPCHK(hipStreamWaitEvent(c->side, c->ev_fork, 0));
    if ((rc = bwd_ubar(c, n, redT, c->side))) return rc;
    if ((rc = bwd_wbar(c, n, step_u(c, params), s))) return rc;
    HIPCHK(hipEventRecord(c->ev_fork2, s));
    HIPCHK(hipStreamWaitEvent(c->side, c->ev_fork2, 0));
    if ((rc = bwd_gt(c, n, redT, c->side))) return rc;
    if ((rc = bwd_hyper(c, r, n, redd, s, c->side))) return rc;
    HIPCHK(hipEventRecord(c->ev_join, c->side));         // behind everything the side stream took: ubar, G^T and the hyper-TN form
    LAUNCHCHK("backward");
    if ((rc = bwd_ak(c, n, redT, s))) return rc;
    HIPCHK(hipStreamWaitEvent(s, c->ev_join, 0));
    LAUNCHCHK("reductions");
    return 0;
  }

  // the forward of the predictive entry points (mode 4 of predict, predict_mc, fold_in, the joint posterior): no backward follows, so no dK_nm pieces
  static int predictive_forward(gdrf_ctx* c, const T* X, int64_t n, const T* params, hipStream_t s) {
    StepRows r;
    if (int rc = step_inputs(c, X, n, params, s, &r)) return rc;
    if (int rc = step_transforms(c, params, s)) return rc;
    return step_forward(c, r, n, s, false);
  }

  static int step_local(gdrf_ctx* c, const T* X, const int32_t* ws, const T* eps, int64_t n, const T* Z, const T* params,
                        T* redT, double* redd, hipStream_t s) {
    StepRows r;
    int rc;
    if ((rc = step_inputs(c, X, n, params, s, &r))) return rc;
    if ((rc = step_transforms(c, params, s))) return rc;
    if ((rc = step_forward(c, r, n, s, true))) return rc;
    if ((rc = step_rows(c, ws, eps, n, redT, redd, s))) return rc;
    return step_backward(c, r, n, params, redT, redd, s);
  }

  // Guide and model evaluated at DIFFERENT inputs (the reference's quirk Q3, sparse_gdrf.py:376-380): forward at the guide's inputs,
  // keep its (loc, tt, q); forward at the model's; two-point row terms; backward through the model-side predictive; forward at the
  // guide's inputs again (the N x M intermediates are not kept twice) and backward through the guide-side predictive; the two
  // payloads add.  ~2.5 x the cost of a step - this path exists for parity with the reference on non-unit worlds, not for speed.
  static int step_local2(gdrf_ctx* c, const T* Xm, const T* Xg, const int32_t* ws, const T* eps, int64_t n, const T* Z, const T* params,
                         T* redT, double* redd, hipStream_t s) {
    const int K = c->K, V = c->V;
    const int64_t ldk = c->ldk, kn = (int64_t)K * ldk, nq = (int64_t)((c->Mp + 63) / 64) * ldk;
    const RedLay rl = red_lay(c);
    const int64_t nT = rl.total, nd = red_nd(c);
    StepRows rg, rm;
    int rc;
    if (!c->g_loc) {
      void** ps[] = {&c->g_loc, &c->g_tt, &c->g_qpart, &c->g_vbar, &c->g_locbar, &c->g_asum, &c->g_redT, (void**)&c->g_redd};
      const size_t sz[] = {(size_t)kn * c->esz, (size_t)kn * c->esz, (size_t)nq * c->esz, (size_t)kn * c->esz, (size_t)kn * c->esz,
                           (size_t)ldk * c->esz, (size_t)nT * c->esz, (size_t)nd * sizeof(double)};
      for (int i = 0; i < 8; ++i)
        if ((rc = ctx_alloc(c, ps[i], sz[i], "hipMalloc(two-point scratch)"))) return rc;
    }
    if ((rc = step_inputs(c, Xg, n, params, s, &rg)) || (rc = step_transforms(c, params, s)) || (rc = step_forward(c, rg, n, s, true))) return rc;
    HIPCHK(hipMemcpyAsync(c->g_loc, c->loc, (size_t)kn * c->esz, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(c->g_tt, c->tt, (size_t)kn * c->esz, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(c->g_qpart, c->qpart, (size_t)nq * c->esz, hipMemcpyDeviceToDevice, s));
    if ((rc = step_inputs(c, Xm, n, params, s, &rm)) || (rc = step_forward(c, rm, n, s, true))) return rc;
    {
      // the guide-side mu (its q is rewritten below), the streamed or sparse likelihood -> mubar, the two-point sites (V-free)
      ScopedTimer tm(c, 6, s);
      if ((rc = vs_ensure(c))) return rc;
      const int G = vs_grid(c, n);
      rows_mu(c, n, G, eps, (const T*)c->g_qpart, (const T*)c->g_loc, (const T*)c->g_tt, (const T*)c->mean_g, c->mean_g_sk, c->mean_g_sn, s);
      hipLaunchKernelGGL(vs_rowsum_kernel<T>, dim3(K), dim3(256), 0, s, P(c->phi), K, V, (T*)c->vs_rs);
      if ((rc = vs_launch<VS_SOFTMAX>(c, n, G, P(c->mu), ldk, 1, ws, (T*)c->vs_tmp, ldk, c->dpart, 0, s))) return rc;
      hipLaunchKernelGGL(elbo_rows2_sites_kernel<T>, dim3(G), dim3(64), 0, s, n, K, c->hyp, nct<TS>(c), P(c->qpart), P(c->loc), P(c->tt),
                         (const T*)c->g_qpart, (const T*)c->g_loc, (const T*)c->g_tt, eps, ldk, n, (const T*)c->vs_tmp, (const T*)c->mean,
                         c->mean_sk, c->mean_sn, (const T*)c->mean_g, c->mean_g_sk, c->mean_g_sn, P(c->q), P(c->vbar), P(c->locbar), P(c->asum),
                         (T*)c->g_vbar, (T*)c->g_locbar, (T*)c->g_asum, P(c->mu), c->dpart);
      LAUNCHCHK("elbo_rows2");
      rows_reduce(c, vs_parts(c), G, redT, redd, s, vs_nparts(c, G));
    }
    // backward through the model-side predictive (the buffers hold its W), payload aside
    if ((rc = step_inputs(c, Xm, n, params, s, &rm)) || (rc = step_backward(c, rm, n, params, redT, redd, s))) return rc;
    HIPCHK(hipMemcpyAsync(c->g_redT, redT, (size_t)nT * c->esz, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(c->g_redd, redd, (size_t)nd * sizeof(double), hipMemcpyDeviceToDevice, s));
    // the guide side: its forward again, its row-local gradients in place of the model's
    if ((rc = step_inputs(c, Xg, n, params, s, &rg)) || (rc = step_forward(c, rg, n, s, true))) return rc;
    std::swap(c->vbar, c->g_vbar); std::swap(c->locbar, c->g_locbar); std::swap(c->asum, c->g_asum);
    if (!(rc = step_inputs(c, Xg, n, params, s, &rg))) rc = step_backward(c, rg, n, params, redT, redd, s);
    std::swap(c->vbar, c->g_vbar); std::swap(c->locbar, c->g_locbar); std::swap(c->asum, c->g_asum);
    if (rc) return rc;
    // payload = model side + guide side: ubar, A_k, G^T (not the phibar block, which the row kernel wrote once) and red_d[4..]
    auto add = [&](int64_t off, int64_t len) {
      hipLaunchKernelGGL(add_into_kernel<T>, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s, len, (const T*)c->g_redT + off, redT + off);
    };
    add(rl.ubar, rl.phibar - rl.ubar);
    add(rl.A, rl.tail - rl.A);
    const int64_t ndk = nd - 4 - c->mean_count;      // the mean segment is the caller's to write (gdrf_set_mean_params)
    hipLaunchKernelGGL(add_into_kernel<double>, dim3((unsigned)((ndk + 255) / 256)), dim3(256), 0, s, ndk, (const double*)c->g_redd + 4, redd + 4);
    LAUNCHCHK("step_local2");
    return 0;
  }

  // one svi.step around a caller-supplied link function, in three calls:
  //   phase 0: transforms + forward + mu (rows_mu_kernel) -> workspace 14;  phase 1: ext = theta (K, ext_ld) through the streamed or sparse
  //   likelihood -> thetabar in workspace 6 (locbar), Phi-bar (its constant part subtracted after the reduction), the log-likelihood sum;
  //   phase 2: ext = mubar (K, ext_ld) -> the Normal sites, the row-local backward (rows_sites_kernel) and the rest of gdrf_step_local
  static int step_local_link(gdrf_ctx* c, const T* X, const int32_t* ws, const T* eps, int64_t n, const T* Z, const T* params,
                             T* redT, double* redd, hipStream_t s, int phase, const T* ext, int64_t ext_ld) {
    const int K = c->K, V = c->V;
    StepRows r;
    int rc;
    if (phase == 0 && ((rc = step_inputs(c, X, n, params, s, &r)) || (rc = step_transforms(c, params, s)) || (rc = step_forward(c, r, n, s, true)))) return rc;
    if ((rc = vs_ensure(c))) return rc;
    const int G = vs_grid(c, n);
    if (phase == 0) {
      rows_mu(c, n, G, eps, P(c->qpart), P(c->loc), P(c->tt), (const T*)c->mean, c->mean_sk, c->mean_sn, s);
    } else if (phase == 1) {
      T* rs = (T*)c->vs_rs;
      hipLaunchKernelGGL(vs_rowsum_kernel<T>, dim3(K), dim3(256), 0, s, P(c->phi), K, V, rs);
      if ((rc = vs_launch<VS_LINK>(c, n, G, ext, ext_ld, 1, ws, P(c->locbar), c->ldk, c->dpart, 0, s))) return rc;
      phibar_reduce(c, vs_parts(c), vs_nparts(c, G), redT, s);
      hipLaunchKernelGGL(reduce_parts_kernel<T>, dim3((K + 255) / 256), dim3(256), 0, s, vs_cparts(c), (int64_t)G, (int64_t)K, rs + K);
      hipLaunchKernelGGL(vs_sub_rows_kernel<T>, dim3((unsigned)(((int64_t)K * V + 255) / 256)), dim3(256), 0, s, K, V, (const T*)(rs + K),
                         redT + red_lay(c).phibar);
    } else {
      rows_sites(c, n, G, eps, ext, ext_ld, s);
      hipLaunchKernelGGL(reduce_dparts_kernel, dim3(1), dim3(1024), 0, s, c->dpart, (int64_t)G, 4, redd);
    }
    LAUNCHCHK("elbo_rows_link");
    if (phase != 2) return 0;
    if ((rc = step_inputs(c, X, n, params, s, &r))) return rc;
    return step_backward(c, r, n, params, redT, redd, s);
  }

  static int step_finish(gdrf_ctx* c, const T* Z, const T* params, const T* redT, const double* redd, double n_global,
                         double ll_const, T* grads, double* out_d, hipStream_t s) {
    const int Mp = c->Mp, M = c->M, K = c->K, V = c->V;
    const int64_t mm = (int64_t)Mp * Mp;
    int rc;
    const ParamLay pl = param_lay(c);
    const RedLay rl = red_lay(c);
    const T* ubar = redT + rl.ubar;
    const T* phib = redT + rl.phibar;
    const T* Ak = redT + rl.A;
    const T* GT = redT + rl.GT;
    if ((rc = join_fact(c, s))) return rc;
    ScopedTimer tm(c, 13, s);
    dim3 g2((Mp + 255) / 256, Mp);
    dim3 g3((M + 255) / 256, M, K);
    // Sbar_k = 2 A_k S_k and the u_scale_tril gradient do not depend on the Cholesky backward below (a chain of four dependent M x M
    // products): they run beside it on the side stream (whitened form; the unwhitened one chains them through L^-T further down)
    const bool sbar_aside = !c->unwhitened;
    if (sbar_aside) {
      HIPCHK(hipEventRecord(c->ev_fork, s));
      HIPCHK(hipStreamWaitEvent(c->side, c->ev_fork, 0));
      if ((rc = mm_nt<T>(c, Ak, mm, P(c->ST), mm, P(c->Sbar), mm, T(2), K, c->side, true, GDRF_FORM_MM_SBAR))) return rc;
      hipLaunchKernelGGL(grad_s_kernel<T>, g3, dim3(256), 0, c->side, P(c->Sbar), P(c->S), M, Mp, -1.0 / n_global, grads + pl.S);
      HIPCHK(hipEventRecord(c->ev_join, c->side));
    }
    // Cholesky / inverse backward in the solve precision
    hipLaunchKernelGGL((cast_kernel<T, TS>), dim3((unsigned)((mm + 255) / 256)), dim3(256), 0, s, mm, GT, Q(c->GTs));
    // HT = GT Linv ; LbarT = -triu(HT)
    if ((rc = mm_nt<TS>(c, Q(c->GTs), 0, Q(c->LinvT), 0, Q(c->t0), 0, TS(1), 1, s, false, GDRF_FORM_MM_CHAIN))) return rc;
    if (c->unwhitened) {
      // Sbar'^T = 2 S'^T A_k (A_k symmetric) -> Sbar = L^-T Sbar' -> P_k = S'_k Sbar_k^T ; ubar = L^-T ubar' ; HT += sum_k (P_k + u'_k ubar_k^T)
      if ((rc = mm_nt<T>(c, P(c->ST), mm, Ak, mm, P(c->Sbar), mm, T(2), K, s))) return rc;
      hipLaunchKernelGGL((cast_kernel<T, TS>), dim3((unsigned)((K * mm + 255) / 256)), dim3(256), 0, s, K * mm, (const T*)P(c->Sbar), Q(c->uSb));
      if ((rc = mm_nt<TS>(c, Q(c->LinvT), 0, Q(c->uSb), mm, Q(c->uSc), mm, TS(1), K, s))) return rc;   // Sbar[q][j] = sum_i LinvT[q][i] Sbar'[i][j]
      if ((rc = mm_nt<TS>(c, Q(c->uS), mm, Q(c->uSc), mm, Q(c->uSb), mm, TS(1), K, s))) return rc;      // P_k[i][j] = sum_q S'[i][q] Sbar[j][q]
      hipLaunchKernelGGL((upper_matvec_kernel<TS, T>), dim3((M + 127) / 128, K), dim3(128), 0, s, (const TS*)Q(c->Linv), ubar, M, Mp, Q(c->uUb));
      hipLaunchKernelGGL(add_et_kernel<TS>, dim3((M + 255) / 256, M), dim3(256), 0, s, (const TS*)Q(c->uSb), (const TS*)Q(c->uU),
                         (const TS*)Q(c->uUb), K, M, Mp, Q(c->t0));
    }
    hipLaunchKernelGGL(lbar_t_kernel<TS>, g2, dim3(256), 0, s, (const TS*)Q(c->t0), Mp, Q(c->t1));
    // Q = L^T Lbar ; P = Phi(Q)
    if ((rc = mm_nt<TS>(c, Q(c->LT), 0, Q(c->t1), 0, Q(c->t0), 0, TS(1), 1, s))) return rc;
    hipLaunchKernelGGL(phi_tril_kernel<TS>, g2, dim3(256), 0, s, (const TS*)Q(c->t0), Mp, Q(c->t2));
    // YT = Linv^T P^T ; S' = Linv^T Y
    if ((rc = mm_nt<TS>(c, Q(c->LinvT), 0, Q(c->t2), 0, Q(c->t0), 0, TS(1), 1, s))) return rc;
    if ((rc = mm_nt<TS>(c, Q(c->LinvT), 0, Q(c->t0), 0, Q(c->t1), 0, TS(1), 1, s))) return rc;
    if (c->per) {          // K_uu coordinate and period sums -> dsmall[9..9+D+npair) (dsmall[8] is the ll_const scratch)
      hipLaunchKernelGGL((kuu_bar_reduce_kernel<TS, true, true>), dim3(M), dim3(256), 0, s, (const TS*)Q(c->t1), (const TS*)Q(c->Zs), M, Mp, c->D,
                         c->kind, c->hyp, c->dpart, c->apart, (const TS*)Q(c->Zph));
      hipLaunchKernelGGL(reduce_dparts_kernel, dim3(1), dim3(1024), 0, s, c->apart, (int64_t)M, c->D + c->npair, c->dsmall + 9);
    } else if (c->ard) {          // K_uu sums of d / d log ls_d -> dsmall[3..3+D)
      hipLaunchKernelGGL((kuu_bar_reduce_kernel<TS, true>), dim3(M), dim3(256), 0, s, (const TS*)Q(c->t1), (const TS*)Q(c->Zs), M, Mp, c->D, c->kind,
                         c->hyp, c->dpart, c->apart);
      hipLaunchKernelGGL(reduce_dparts_kernel, dim3(1), dim3(1024), 0, s, c->apart, (int64_t)M, c->D, c->dsmall + 3);
    } else {
      hipLaunchKernelGGL(kuu_bar_reduce_kernel<TS>, dim3(M), dim3(256), 0, s, (const TS*)Q(c->t1), (const TS*)Q(c->Zs), M, Mp, c->D, c->kind,
                         c->hyp, c->dpart);
    }
    hipLaunchKernelGGL(reduce_dparts_kernel, dim3(1), dim3(1024), 0, s, c->dpart, (int64_t)M, 3, c->dsmall);
    if (c->learn_z && c->per)
      hipLaunchKernelGGL((grad_z_kernel<TS, T, true, true>), dim3(M), dim3(256), 0, s, (const TS*)Q(c->t1), (const TS*)Q(c->Zs), M, Mp, c->D, c->kind,
                         c->hyp, redd + 8, -1.0 / n_global, grads + pl.Z, Z);
    else if (c->learn_z && c->ard)
      hipLaunchKernelGGL((grad_z_kernel<TS, T, true>), dim3(M), dim3(256), 0, s, (const TS*)Q(c->t1), (const TS*)Q(c->Zs), M, Mp, c->D, c->kind, c->hyp,
                         redd + 8, -1.0 / n_global, grads + pl.Z, Z);
    else if (c->learn_z)
      hipLaunchKernelGGL((grad_z_kernel<TS, T>), dim3(M), dim3(256), 0, s, (const TS*)Q(c->t1), (const TS*)Q(c->Zs), M, Mp, c->D, c->kind, c->hyp,
                         redd + 8, -1.0 / n_global, grads + pl.Z);
    // Sbar_k = 2 A_k S_k (N-side precision: well conditioned)
    if (sbar_aside) {
      HIPCHK(hipStreamWaitEvent(s, c->ev_join, 0));
    } else {
      if ((rc = mm_nt<T>(c, Ak, mm, P(c->ST), mm, P(c->Sbar), mm, T(2), K, s, false, GDRF_FORM_MM_SBAR))) return rc;
      hipLaunchKernelGGL(grad_s_kernel<T>, g3, dim3(256), 0, s, P(c->Sbar), P(c->S), M, Mp, -1.0 / n_global, grads + pl.S);
    }
    hipLaunchKernelGGL(grad_small_kernel<T>, dim3(1), dim3(256), 0, s, M, Mp, K, V, c->hyp, redd, c->dsmall, ubar, phib, P(c->phi),
                       c->alpha_dev, c->lgam_const, ll_const, n_global, grads, grads + pl.uloc, grads + pl.phi, c->flag, out_d);
    if (c->per)
      hipLaunchKernelGGL(grad_per_kernel<T>, dim3(1), dim3(64), 0, s, coord_tab(c), (const double*)redd + 8 + (int64_t)M * c->D,
                         (const double*)c->dsmall + 9, n_global, grads);
    else if (c->ard)
      hipLaunchKernelGGL(grad_ard_kernel<T>, dim3(1), dim3(64), 0, s, c->D, (const double*)redd + 8 + (int64_t)M * c->D, (const double*)c->dsmall + 3,
                         n_global, grads, grads + pl.ard);
    if (c->mean_count)
      hipLaunchKernelGGL(grad_mean_kernel<T>, dim3((unsigned)((c->mean_count + 255) / 256)), dim3(256), 0, s, c->mean_count,
                         (const double*)redd + red_mean_off(c), n_global, grads + pl.mean);
    if (c->unwhitened)       // overwrite the u_loc / u_scale_tril blocks with the gradients chained through L^-T
      hipLaunchKernelGGL((grad_unwhitened_kernel<TS, T>), g3, dim3(256), 0, s, (const TS*)Q(c->uSc), (const TS*)Q(c->uUb), params + pl.S, K, M,
                         Mp, -1.0 / n_global, grads + pl.S, grads + pl.uloc);
    LAUNCHCHK("step_finish");
    return 0;
  }

  static int predict(gdrf_ctx* c, const T* X, int64_t n, const T* Z, const T* params, const int32_t* ws, int mode,
                     T* out, double* out_d, hipStream_t s) {
    const int Mp = c->Mp, M = c->M, K = c->K, V = c->V;
    const T* U = params + param_lay(c).uloc;
    if (int rcj = join_fact(c, s)) return rcj;
    if (c->unwhitened) {       // loc = K_nm L^-T (L^-1 u)
      hipLaunchKernelGGL((lower_matvec_kernel<TS, T>), dim3((M + 127) / 128, K), dim3(128), 0, s, (const TS*)Q(c->Linv), U, M, Mp, Q(c->uU),
                         (T*)c->Uw);
      U = (const T*)c->Uw;
    }
    if (mode == 4) {
      // (f_loc, f_var) of gp.util.conditional(full_cov=False) (gdrf/models/sparse_gdrf.py:277-319): the step's own forward - transforms,
      // K_nm, W = K_nm L^-T with its row norms, loc = W U^T, tt = |S_k^T w|^2 - and one pass that assembles the variance
      if (n > c->ncap) return fail(-1, "gdrf_predict", "mode 4 (loc, var) needs n <= n_cap");
      if (int rc = predictive_forward(c, X, n, params, s)) return rc;
      hipLaunchKernelGGL(predict_var_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, K, c->hyp, (const T*)P(c->qpart), nct<TS>(c),
                         (const T*)P(c->loc), (const T*)P(c->tt), c->ldk, out);
      LAUNCHCHK("predict (loc, var)");
      return 0;
    }
    StepRows r;
    if (int rc = step_inputs(c, X, n, params, s, &r)) return rc;
    X = r.X;
    if (mode >= 2) hipLaunchKernelGGL(build_phi_kernel<T>, dim3(K), dim3(64), 0, s, params + param_lay(c).phi, K, V, P(c->phi));
    const F::PredictPlan pl = F::predict_plan(form_shape(c, n, mode));
    const size_t lds = pl.lds;
    const int64_t ldo = mode == 0 ? n : (mode == 1 ? K : V);
    int64_t blocks = (n + 127) / 128; if (blocks > 2048) blocks = 2048; if (blocks < 1) blocks = 1;
    if (pl.form != F::PREDICT_MFMA)      // the row forms read the coefficients Cf = L^-T u
      hipLaunchKernelGGL((predict_coeff_kernel<TS, T>), dim3((M + 127) / 128, K), dim3(128), 0, s, (const TS*)Q(c->Linv), U, M, Mp, K, Q(c->Cf));
    if (!pl.fits)
      return fail(-1, "gdrf_predict", pl.form == F::PREDICT_STREAMED    ? "M*D solve-precision elements exceed the LDS budget (150 KB)"
                                      : pl.form == F::PREDICT_ROWS_BIGK ? "M*D + K*V + 128*(V+1) solve-precision elements exceed the LDS budget (150 KB)"
                                                                        : "M*D + K*V solve-precision elements exceed the LDS budget (150 KB)");
    c->forms[GDRF_FORM_PREDICT] = pl.form; c->forms[GDRF_FORM_PREDICT_NB] = pl.NB;
    switch (pl.form) {
      case F::PREDICT_STREAMED: {
        // form 1: the any-K row kernel without Phi in LDS gives f_loc / topic_probs; for word_probs and perplexity it writes topic_probs of
        // up to n_cap rows at a time into the form's scratch and the streamed product over Phi tiles (rows_vstream.h) finishes them
        auto kfn = ard_fwd(c) ? predict_rows_bigk_kernel<TS, T, true> : predict_rows_bigk_kernel<TS, T>;
        if (lds > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        auto rows = [&](const T* Xc, int64_t m, int md, T* o, int64_t ldo) {
          int64_t blocks = (m + 127) / 128; if (blocks > 2048) blocks = 2048; if (blocks < 1) blocks = 1;
          hipLaunchKernelGGL(kfn, dim3((unsigned)blocks), dim3(128), lds, s, Xc, m, (const TS*)Q(c->Zs), M, c->D, c->kind, c->hyp, (const TS*)Q(c->Cf),
                             K, V, (const T*)P(c->phi), ws, md, o, ldo, c->dpart);
        };
        if (mode <= 1) {
          rows(X, n, mode, out, mode == 0 ? n : K);
          LAUNCHCHK("predict (streamed form)");
          return 0;
        }
        if (int rc = vs_ensure(c, mode == 3)) return rc;
        const int G = vs_grid(c, std::min<int64_t>(n, c->ncap), mode == 3);
        for (int64_t off = 0; off < n; off += c->ncap) {
          const int64_t m = std::min<int64_t>(c->ncap, n - off);
          rows(X + off * c->D, m, 1, (T*)c->vs_tmp, K);
          int rc;
          if (mode == 2) rc = vs_launch<VS_WORDP>(c, m, G, (const T*)c->vs_tmp, 1, K, nullptr, out + off * V, V, nullptr, 0, s);
          else rc = vs_launch<VS_PERP>(c, m, G, (const T*)c->vs_tmp, 1, K, ws ? ws + off * V : nullptr, nullptr, 0, c->dpart, off > 0, s, off);
          if (rc) return rc;
        }
        if (mode == 3) hipLaunchKernelGGL(reduce_dparts_kernel, dim3(1), dim3(1024), 0, s, c->dpart, (int64_t)G, 2, out_d);
        LAUNCHCHK("predict (streamed form)");
        return 0;
      }
      case F::PREDICT_MFMA: {
        // matrix-core form (predict.h): a wave owns 16 rows, one covariance value per lane and step is the A operand of the 16x16x4
        // matrix instruction, the padded transposed coefficients CfT its B operand.  K <= 32, the scaled inducing inputs in LDS.
        const int M4 = (int)round_up(M, 4), NB = pl.NB, DDt = c->D <= 2 ? 2 : GDRF_DMAX;
        const int ldc = 16 * NB;
        hipLaunchKernelGGL((predict_coeff_t_kernel<TS, T>), dim3(M4), dim3(64), 0, s, (const TS*)Q(c->LinvT), U, M, Mp, M4, K, ldc, Q(c->CfT));
        const int64_t groups = (n + 15) / 16;
        blocks = (groups + 3) / 4; if (blocks > 2048) blocks = 2048; if (blocks < 1) blocks = 1;
        auto go = [&](auto kern) {
          return launch_lds(kern, dim3((unsigned)blocks), dim3(256), lds, s, X, n, (const TS*)Q(c->Zs), M, M4, c->D, c->kind, c->hyp, (const TS*)Q(c->CfT), K, V,
                            (const T*)P(c->phi), ws, mode, out, ldo, c->dpart);
        };
        constexpr int DM = GDRF_DMAX;
        const int rc = ard_fwd(c) ? (DDt == 2 ? (NB == 1 ? go(predict_mfma_kernel<TS, T, 2, 1, true>) : go(predict_mfma_kernel<TS, T, 2, 2, true>))
                                              : (NB == 1 ? go(predict_mfma_kernel<TS, T, DM, 1, true>) : go(predict_mfma_kernel<TS, T, DM, 2, true>)))
                                  : (DDt == 2 ? (NB == 1 ? go(predict_mfma_kernel<TS, T, 2, 1, false>) : go(predict_mfma_kernel<TS, T, 2, 2, false>))
                                              : (NB == 1 ? go(predict_mfma_kernel<TS, T, DM, 1, false>) : go(predict_mfma_kernel<TS, T, DM, 2, false>)));
        if (rc) return rc;
        if (mode == 3) hipLaunchKernelGGL(reduce_dparts_kernel, dim3(1), dim3(1024), 0, s, c->dpart, blocks, 2, out_d);
        LAUNCHCHK("predict (mfma)");
        return 0;
      }
      case F::PREDICT_ROWS_BIGK: {
        auto kfn = ard_fwd(c) ? predict_rows_bigk_kernel<TS, T, true> : predict_rows_bigk_kernel<TS, T>;
        if (int rc = launch_lds(kfn, dim3((unsigned)blocks), dim3(128), lds, s, X, n, (const TS*)Q(c->Zs), M, c->D, c->kind, c->hyp, (const TS*)Q(c->Cf), K, V,
                                (const T*)P(c->phi), ws, mode, out, ldo, c->dpart)) return rc;
        break;
      }
      default: {                  // predict_rows, the coefficients in LDS or read from memory
        auto kfn = ard_fwd(c) ? predict_rows_kernel<TS, T, true> : predict_rows_kernel<TS, T>;
        const int in_lds = pl.form == F::PREDICT_ROWS_LDS;
        if (int rc = launch_lds(kfn, dim3((unsigned)blocks), dim3(128), lds, s, X, n, (const TS*)Q(c->Zs), M, c->D, c->kind, c->hyp, (const TS*)Q(c->Cf), K, V,
                                (const T*)P(c->phi), ws, mode, out, ldo, c->dpart, in_lds)) return rc;
      }
    }
    if (mode == 3) hipLaunchKernelGGL(reduce_dparts_kernel, dim3(1), dim3(1024), 0, s, c->dpart, blocks, 2, out_d);
    LAUNCHCHK("predict");
    return 0;
  }

  // Monte-Carlo integration over q(mu) at new inputs (predict_mc.h): the step's forward as in mode 4 of predict, then one kernel over the
  // rows that draws (or reads) eps and reduces the samples; mode 2 ends in the per-workgroup partials' sum
  static int predict_mc(gdrf_ctx* c, const T* X, int64_t n, const T* Z, const T* params, const int32_t* ws, int mode, int S, uint64_t seed,
                        int64_t row_offset, const T* eps, T* out, double* out_d, hipStream_t s) {
    const int K = c->K, V = c->V;
    return predictive_form(K, [&](auto fm) -> int {
      using F = decltype(fm);
      const size_t lds = mode == MC_SCORE ? mc_score_lds<T>(K, V, F::LG, F::KJ) : 0;
      if (128 + lds > 150 * 1024) return rows_lds_fail("gdrf_predict_mc");      // the LDS budget of the default row forms
      if (int rc = predictive_forward(c, X, n, params, s)) return rc;
      const int grid = lane_group_grid(n, F::LG);
      if (int rc = launch_lds(predict_mc_kernel<T, F::LG, F::KJ>, dim3(grid), dim3(256), lds, s, mode, n, K, V, S, (const Hyper*)c->hyp,
                              (const T*)P(c->qpart), nct<TS>(c), (const T*)P(c->loc), (const T*)P(c->tt), c->ldk, (const T*)c->mean, c->mean_sk,
                              c->mean_sn, eps, seed, row_offset, (const T*)P(c->phi), ws, out, c->dpart)) return rc;
      if (mode == MC_SCORE) hipLaunchKernelGGL(reduce_dparts_kernel, dim3(1), dim3(1024), 0, s, c->dpart, (int64_t)grid, 2, out_d);
      LAUNCHCHK("predict_mc");
      return 0;
    });
  }

  // Entropy and information-gain maps (predict_info.h): the step's forward as in mode 4 of predict, then one kernel over the rows that
  // integrates the entropies over the draws; Phi goes through LDS in chunks of GDRF_INFO_V_CHUNK words, so no V is too large
  static int predict_info(gdrf_ctx* c, const T* X, int64_t n, const T* Z, const T* params, int S, uint64_t seed, int64_t row_offset,
                          const T* eps, double* out, hipStream_t s) {
    const int K = c->K, V = c->V;
    return predictive_form(K, [&](auto fm) -> int {
      using F = decltype(fm);
      if (int rc = predictive_forward(c, X, n, params, s)) return rc;
      if (int rc = launch_lds(predict_info_kernel<T, F::LG, F::KJ>, dim3(lane_group_grid(n, F::LG)), dim3(256), info_lds<T>(K, V, F::LG, F::KJ), s,
                              n, K, V, S, (const Hyper*)c->hyp, (const T*)P(c->qpart), nct<TS>(c), (const T*)P(c->loc), (const T*)P(c->tt), c->ldk,
                              (const T*)c->mean, c->mean_sk, c->mean_sn, eps, seed, row_offset, (const T*)P(c->phi), out)) return rc;
      LAUNCHCHK("predict_info");
      return 0;
    });
  }

  // Per-row log predictive densities (predict_score.h): the step's forward as in mode 4 of predict, then one kernel over the rows that
  // scores each row's counts under the draws - dense (Phi through LDS in chunks of GDRF_SCORE_V_CHUNK words, the samples in tiles of
  // GDRF_SCORE_S_TILE) or CSR (the stored entries only, Phi from global memory); no V and no S is too large
  static int predict_score(gdrf_ctx* c, const T* X, int64_t n, const T* Z, const T* params, const int32_t* ws, const int64_t* crow,
                           const int32_t* col, const int32_t* val, int S, uint64_t seed, int64_t row_offset, const T* eps, double* out,
                           hipStream_t s) {
    const int K = c->K, V = c->V;
    const bool csr = crow != nullptr;
    return predictive_form(K, [&](auto fm) -> int {
      using F = decltype(fm);
      const size_t lds = csr ? score_csr_lds<T>(F::LG, F::KJ) : score_dense_lds<T>(K, V, F::LG, F::KJ);
      if (int rc = predictive_forward(c, X, n, params, s)) return rc;
      auto go = [&](auto kern) {
        return launch_lds(kern, dim3(lane_group_grid(n, F::LG)), dim3(256), lds, s, n, K, V, S, (const Hyper*)c->hyp, (const T*)P(c->qpart), nct<TS>(c),
                          (const T*)P(c->loc), (const T*)P(c->tt), c->ldk, (const T*)c->mean, c->mean_sk, c->mean_sn, eps, seed, row_offset,
                          (const T*)P(c->phi), ws, crow, col, val, out);
      };
      if (int rc = csr ? go(predict_score_kernel<T, F::LG, F::KJ, true>) : go(predict_score_kernel<T, F::LG, F::KJ, false>)) return rc;
      LAUNCHCHK("predict_score");
      return 0;
    });
  }

  // PSIS leave-one-out (predict_loo.h): the step's forward as in mode 4 of predict, then one kernel over the rows that forms each row's
  // a_s as predict_score does, keeps all S of them in LDS and runs the tail fit and the smoothing on them; RP rows per workgroup pass
  // (forms.h::loo_plan)
  static int predict_loo(gdrf_ctx* c, const T* X, int64_t n, const T* Z, const T* params, const int32_t* ws, const int64_t* crow,
                         const int32_t* col, const int32_t* val, int S, uint64_t seed, int64_t row_offset, const T* eps, double* out,
                         double* a_out, hipStream_t s) {
    const int K = c->K, V = c->V;
    const bool csr = crow != nullptr;
    return predictive_form(K, [&](auto fm) -> int {
      using F = decltype(fm);
      const forms::LooPlan pl = forms::loo_plan(K, V, S, (int)sizeof(T), F::LG, csr);
      if (pl.lds > forms::LDS_ROWS) return rows_lds_fail("gdrf_predict_loo");      // loo_plan's worst case fits: not reached
      c->loo_plan[0] = pl.RP; c->loo_plan[1] = (int)pl.lds;
      if (int rc = predictive_forward(c, X, n, params, s)) return rc;
      const int64_t nblk = (n + pl.RP - 1) / pl.RP;
      const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(nblk, 1024));
      auto go = [&](auto kern) {
        return launch_lds(kern, dim3(grid), dim3(256), pl.lds, s, n, K, V, S, pl.RP, pl.P, pl.M, pl.stride, (const Hyper*)c->hyp, (const T*)P(c->qpart),
                          nct<TS>(c), (const T*)P(c->loc), (const T*)P(c->tt), c->ldk, (const T*)c->mean, c->mean_sk, c->mean_sn, eps, seed, row_offset,
                          (const T*)P(c->phi), ws, crow, col, val, out, a_out);
      };
      if (int rc = csr ? go(predict_loo_kernel<T, F::LG, F::KJ, true>) : go(predict_loo_kernel<T, F::LG, F::KJ, false>)) return rc;
      LAUNCHCHK("predict_loo");
      return 0;
    });
  }

  // Quantile, exceedance and dominant-topic maps (predict_quant.h): the step's forward as in mode 4 of predict, then one kernel over the
  // rows.  The quantile mode keeps the samples of CP components of RP rows in LDS per workgroup pass (forms.h::quant_plan); the counter
  // modes take 256 / LG rows per pass and only the theta slots
  static int predict_quant(gdrf_ctx* c, const T* X, int64_t n, const T* Z, const T* params, int mode, int S, uint64_t seed, int64_t row_offset,
                           const T* eps, const QuantLevels& lev, int nlev, const int32_t* words, int nwords, double* out, hipStream_t s) {
    const int K = c->K, V = c->V;
    const bool use_words = nwords > 0;
    const int C = use_words ? nwords : K;
    return predictive_form(K, [&](auto fm) -> int {
      using F = decltype(fm);
      constexpr int RPB = 256 / F::LG;
      int RP = RPB, CP = use_words ? std::min(C, F::LG * QUANT_WJ) : K, P = 1;
      size_t lds = quant_theta_lds<T>(F::LG, F::KJ);
      if (mode == QUANT_Q) {
        const forms::QuantPlan pl = forms::quant_plan(K, C, S, (int)sizeof(T), F::LG);
        RP = pl.RP; CP = pl.CP; P = pl.P; lds = pl.lds;
      }
      c->quant_plan[0] = RP; c->quant_plan[1] = CP; c->quant_plan[2] = (int)lds;
      if (int rc = predictive_forward(c, X, n, params, s)) return rc;
      const int64_t nblk = (n + RP - 1) / RP;
      const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(nblk, 1024));
      if (int rc = launch_lds(predict_quant_kernel<T, F::LG, F::KJ>, dim3(grid), dim3(256), lds, s, mode, n, K, V, S, (const Hyper*)c->hyp,
                              (const T*)Impl::P(c->qpart), nct<TS>(c), (const T*)Impl::P(c->loc), (const T*)Impl::P(c->tt), c->ldk, (const T*)c->mean, c->mean_sk,
                              c->mean_sn, eps, seed, row_offset, (const T*)Impl::P(c->phi), words, C, use_words, nlev, lev, RP, CP, P, out)) return rc;
      LAUNCHCHK("predict_quant");
      return 0;
    });
  }

  // Fold-in (foldin.h): the step's forward as in mode 4 of predict, then one kernel that runs the per-row MAP from the rows' own counts -
  // dense (Phi, the counts and c in LDS) or CSR (the stored entries only, Phi from global memory); mode 3 ends in the partials' sum
  static int fold_in(gdrf_ctx* c, const T* X, int64_t n, const T* Z, const T* params, const int32_t* ws, const int64_t* crow, const int32_t* col,
                     const int32_t* val, const int32_t* ws2, const int64_t* crow2, const int32_t* col2, const int32_t* val2, int mode,
                     int num_iters, double tol, T* out, double* diag, double* out_d, hipStream_t s) {
    const int K = c->K, V = c->V;
    const bool csr = crow != nullptr;
    return predictive_form(K, [&](auto fm) -> int {
      using F = decltype(fm);
      const size_t lds = csr ? fi_csr_lds<T>(F::LG, F::KJ) : fi_dense_lds<T>(K, V, F::LG, F::KJ);
      if (!csr && 128 + lds > 150 * 1024) return rows_lds_fail("gdrf_fold_in");      // the LDS budget of the default row forms
      if (int rc = predictive_forward(c, X, n, params, s)) return rc;
      const int grid = lane_group_grid(n, F::LG);
      auto go = [&](auto kern) {
        return launch_lds(kern, dim3(grid), dim3(256), lds, s, mode, n, K, V, num_iters, tol, (const Hyper*)c->hyp, (const T*)P(c->qpart), nct<TS>(c),
                          (const T*)P(c->loc), (const T*)P(c->tt), c->ldk, (const T*)c->mean, c->mean_sk, c->mean_sn, (const T*)P(c->phi), ws, crow,
                          col, val, ws2, crow2, col2, val2, out, diag, c->dpart);
      };
      if (int rc = csr ? go(foldin_kernel<T, F::LG, F::KJ, true>) : go(foldin_kernel<T, F::LG, F::KJ, false>)) return rc;
      if (mode == FI_SCORE) hipLaunchKernelGGL(reduce_dparts_kernel, dim3(1), dim3(1024), 0, s, c->dpart, (int64_t)grid, 2, out_d);
      LAUNCHCHK("fold_in");
      return 0;
    });
  }

  // Posterior-predictive count samples (sample_counts.h): Phi from the parameters, then one kernel in which a wave or a workgroup owns a
  // (row, sample) pair; SC_STATS ends in the per-sample sums of the per-workgroup partials.  No GP quantity is read: no factorisation is needed.
  static int sample_counts(gdrf_ctx* c, const T* theta, int64_t n, const T* params, const int32_t* totals, int tmax, const int32_t* ws, int mode,
                           int S, uint64_t seed, int64_t row_offset, const double* u, int32_t* out, double* dev, int64_t* zeros, hipStream_t s) {
    const int K = c->K, V = c->V;
    // up to GDRF_SC_WAVE_V words four waves share a workgroup, each with a pair of its own, and Phi joins them in LDS while four such
    // workgroups still fit a CU (40 KB each); above it the workgroup owns one pair and Phi is read from global memory (L2)
    const bool blk = V > GDRF_SC_WAVE_V;
    const int units = blk ? 1 : 4;
    const bool phi_lds = !blk && sc_lds<T>(K, V, mode, units, true) <= 40 * 1024;
    const size_t lds = sc_lds<T>(K, V, mode, units, phi_lds);
    if (128 + lds > 150 * 1024) return rows_lds_fail("gdrf_sample_counts");      // the LDS budget of the default row forms
    int64_t grid = std::min<int64_t>((n + units - 1) / units, 1024);
    if (mode == SC_STATS) {
      if (2 * (int64_t)S > c->dpart_len) return fail(-1, "gdrf_sample_counts", "num_samples exceeds the context's partial-sum scratch");
      grid = std::min<int64_t>(grid, c->dpart_len / (2 * (int64_t)S));
      HIPCHK(hipMemsetAsync(zeros, 0, (size_t)S * V * sizeof(int64_t), s));
    }
    hipLaunchKernelGGL(build_phi_kernel<T>, dim3(K), dim3(64), 0, s, params + param_lay(c).phi, K, V, P(c->phi));
    auto go = [&](auto kern) {
      return launch_lds(kern, dim3((unsigned)grid, (unsigned)S), dim3(256), lds, s, mode, n, K, V, theta, (const T*)P(c->phi), totals, tmax, ws, seed,
                        row_offset, u, out, c->dpart, (unsigned long long*)zeros);
    };
    if (int rc = blk ? go(sample_counts_kernel<T, SC_BLOCK>) : phi_lds ? go(sample_counts_kernel<T, SC_WAVE_PHI>) : go(sample_counts_kernel<T, SC_WAVE>))
      return rc;
    if (mode == SC_STATS) hipLaunchKernelGGL(sc_reduce_kernel, dim3(S), dim3(256), 0, s, c->dpart, (int)grid, S, dev);
    LAUNCHCHK("sample_counts");
    return 0;
  }

  // ---- the joint posterior at new inputs (predict_cov.h)
  // a joint buffer of at least `bytes`: a larger request replaces it.  Only the joint calls read these blocks, so the replaced one is
  // freed here, once the device has finished whatever was queued on it (a growth is rare: the wait costs one call, not every call)
  static int joint_buf(gdrf_ctx* c, void** p, int64_t* have, int64_t want, size_t bytes) {
    if (want <= *have && *p) return 0;
    if (*p) {
      HIPCHK(hipDeviceSynchronize());
      c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), *p), c->allocs.end());
      HIPCHK(hipFree(*p));
      *p = nullptr; *have = 0;
    }
    if (int rc = ctx_alloc(c, p, bytes, "hipMalloc(joint posterior)")) return rc;
    *have = want;
    return 0;
  }
  template <int EPI, typename TB, typename TO>
  static void joint_nt(gdrf_ctx* c, const JointNT<TS, TB, T, TO>& p, int batch, hipStream_t s) {
    const dim3 grid((unsigned)((p.nj + GDRF_JT - 1) / GDRF_JT), (unsigned)((p.ni + GDRF_JT - 1) / GDRF_JT), (unsigned)batch);
    if (EPI == JT_RESID && ard_fwd(c)) hipLaunchKernelGGL((joint_nt_kernel<TS, TB, T, TO, EPI, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((joint_nt_kernel<TS, TB, T, TO, EPI, false>), grid, dim3(256), 0, s, p);
  }
  // the step's forward as mode 4 of predict runs it, then W = K_nm L^-T in the solve precision (c->jW): none of the n x n buffers
  static int joint_w(gdrf_ctx* c, const T* X, int64_t n, const T* params, hipStream_t s) {
    const int Mp = c->Mp;
    if (int rc = joint_buf(c, &c->jW, &c->jrows, n, (size_t)n * Mp * sizeof(TS))) return rc;
    if (int rc = predictive_forward(c, X, n, params, s)) return rc;
    JointNT<TS, TS, T, TS> w{(const TS*)Q(c->Knm), Mp, 0, n, (const TS*)Q(c->Linv), Mp, 0, Mp, Mp, Q(c->jW), Mp, 0, nullptr, 0, nullptr, 0, 0, nullptr};
    joint_nt<JT_PLAIN>(c, w, 1, s);
    return 0;
  }
  // joint_w, then R = K_** - W W^T (c->jR, leading dimension *np_out = round_up(n, 32))
  static int joint_forward(gdrf_ctx* c, const T* X, int64_t n, const T* Z, const T* params, int64_t* np_out, hipStream_t s) {
    const int Mp = c->Mp;
    const int64_t np = round_up(n, 32);
    if (int rc = joint_buf(c, &c->jR, &c->jnp, np, (size_t)np * np * sizeof(TS))) return rc;
    if (!c->jflag)
      if (int rc = ctx_alloc(c, &c->jflag, 64, "hipMalloc(joint posterior)", true)) return rc;
    if (int rc = joint_w(c, X, n, params, s)) return rc;
    const T* Xc = c->per ? (const T*)c->Xe : X;               // periodic and product contexts: the embedded rows the forward just wrote
    JointNT<TS, TS, T, TS> r{(const TS*)Q(c->jW), Mp, 0, n, (const TS*)Q(c->jW), Mp, 0, n, Mp, Q(c->jR), np, 0, nullptr, 0, Xc, c->D, c->kind, c->hyp};
    joint_nt<JT_RESID>(c, r, 1, s);
    LAUNCHCHK("joint posterior (W, R)");
    *np_out = np;
    return 0;
  }

  static int predict_cov(gdrf_ctx* c, const T* X, int64_t n, const T* Z, const T* params, int which, T* out, hipStream_t s) {
    const int Mp = c->Mp, K = c->K;
    int64_t np = 0;
    c->jlast_n = c->jlast_sk = 0;              // W and R are about to be rewritten: no gdrf_sample_joint_retry on the old ones
    if (which == COV_FULL)
      if (int rc = joint_buf(c, &c->jT, &c->jtrows, n, (size_t)K * n * Mp * sizeof(TS))) return rc;
    if (int rc = joint_forward(c, X, n, Z, params, &np, s)) return rc;
    if (which == COV_RESID) {
      hipLaunchKernelGGL((joint_copy_out_kernel<TS, T>), dim3((unsigned)((n + 255) / 256), (unsigned)n), dim3(256), 0, s, (const TS*)Q(c->jR), n, np, out);
    } else {
      // T_k = W S_k (S_k^T in the array precision, as the step's tt reads it), then C_k = R + T_k T_k^T
      JointNT<TS, T, T, TS> t{(const TS*)Q(c->jW), Mp, 0, n, (const T*)P(c->ST), Mp, (int64_t)Mp * Mp, Mp, Mp, Q(c->jT), Mp, n * Mp, nullptr, 0, nullptr, 0, 0,
                              nullptr};
      joint_nt<JT_PLAIN>(c, t, K, s);
      JointNT<TS, TS, T, T> f{(const TS*)Q(c->jT), Mp, n * Mp, n, (const TS*)Q(c->jT), Mp, n * Mp, n, Mp, out, n, n * n, (const TS*)Q(c->jR), np, nullptr, 0, 0,
                              nullptr};
      joint_nt<JT_FULL>(c, f, K, s);
    }
    LAUNCHCHK("predict_cov");
    return 0;
  }

  static int sample_joint(gdrf_ctx* c, const T* X, int64_t n, const T* Z, const T* params, int S, uint64_t seed, const T* xi, const T* zeta,
                          double jitter, T* out, hipStream_t s) {
    const int Mp = c->Mp, M = c->M, K = c->K;
    const int64_t nsk = (int64_t)S * K;
    int64_t np = 0;
    if ((size_t)M * sizeof(T) > 64 * 1024) return fail(-1, "gdrf_sample_joint", "M array-precision elements exceed the LDS budget (64 KB)");
    if (int rc = joint_buf(c, &c->jV, &c->jsk, nsk, (size_t)nsk * Mp * sizeof(TS))) return rc;
    if (int rc = joint_buf(c, &c->jZ, &c->jzel, nsk * round_up(n, 32), (size_t)nsk * round_up(n, 32) * sizeof(TS))) return rc;
    if (int rc = joint_buf(c, &c->jG, &c->jgnp, round_up(n, 32), (size_t)round_up(n, 32) * round_up(n, 32) * sizeof(TS))) return rc;   // the sampler's alone
    c->jlast_n = c->jlast_sk = 0;
    if (int rc = joint_forward(c, X, n, Z, params, &np, s)) return rc;
    const T* U = c->unwhitened ? (const T*)c->Uw : params + param_lay(c).uloc;      // the forward's transforms left L^-1 u in c->Uw
    if (int rc = launch_lds((joint_v_kernel<TS, T>), dim3((unsigned)((Mp + 255) / 256), (unsigned)nsk), dim3(256), (size_t)M * sizeof(T), s, U, (const T*)P(c->ST), M,
                            Mp, K, xi, seed, Q(c->jV))) return rc;
    hipLaunchKernelGGL((joint_zeta_kernel<TS, T>), dim3((unsigned)((np + 255) / 256), (unsigned)nsk), dim3(256), 0, s, n, np, K, zeta, seed, Q(c->jZ));
    LAUNCHCHK("sample_joint");
    c->jlast_n = n; c->jlast_sk = nsk;
    return joint_draw(c, n, S, jitter, out, s);
  }
  // the part of sample_joint that depends on the jitter: G G^T = R + jitter I by the one-workgroup Cholesky on a buffer of its own, its
  // failure flag in c->jflag (gdrf_joint_failed), then the two sample products from the W, R, V and zeta the last sample_joint left
  static int joint_draw(gdrf_ctx* c, int64_t n, int S, double jitter, T* out, hipStream_t s) {
    const int Mp = c->Mp, K = c->K;
    const int64_t nsk = (int64_t)S * K, np = round_up(n, 32);
    HIPCHK(hipMemsetAsync(c->jflag, 0, sizeof(int), s));
    hipLaunchKernelGGL(joint_chol_in_kernel<TS>, dim3((unsigned)((np + 255) / 256), (unsigned)np), dim3(256), 0, s, (const TS*)Q(c->jR), n, np, jitter, Q(c->jG));
    if (int rc = launch_lds(chol_kernel<TS>, dim3(1), dim3(1024), chol_lds_bytes<TS>((int)n), s, Q(c->jG), (int)n, (int)np, c->jflag, (int64_t)0)) return rc;
    const dim3 grid((unsigned)((n + GDRF_JT - 1) / GDRF_JT), (unsigned)((nsk + GDRF_JT - 1) / GDRF_JT));
    hipLaunchKernelGGL((joint_sample_kernel<TS, T>), grid, dim3(256), 0, s, (const TS*)Q(c->jV), nsk, K, (const TS*)Q(c->jW), Mp, (const TS*)Q(c->jZ),
                       (const TS*)Q(c->jG), n, np, (const T*)c->mean, c->mean_sk, c->mean_sn, out);
    LAUNCHCHK("sample_joint (draw)");
    return 0;
  }

  // ---- the greedy choice of a non-redundant batch of rows (select_batch.h): the forward over the n candidates and the G given rows in one
  // array, W in the solve precision, then per pick the preparation and the pass over the rows; nothing is read back in between
  static int select_batch(gdrf_ctx* c, const T* X, int64_t n, const T* Z, const T* params, const T* given, int G, int count, double noise,
                          int64_t* idx_out, double* gains_out, double* var_out, hipStream_t s) {
    const int Mp = c->Mp, M = c->M, K = c->K, Tm = G + count;
    const int64_t nt = n + G;
    const size_t pass_lds = sel_pass_lds<TS>(Mp);
    if (pass_lds > 150 * 1024) return fail(-1, "gdrf_select_batch", "16 right-hand sides of M solve-precision elements exceed the LDS budget (150 KB)");
    if (int rc = joint_buf(c, &c->sC, &c->sc_el, (int64_t)K * Tm * nt, (size_t)K * Tm * nt * sizeof(TS))) return rc;
    if (int rc = joint_buf(c, &c->sD, &c->sd_el, (int64_t)K * nt, (size_t)K * nt * sizeof(TS))) return rc;
    if (int rc = joint_buf(c, (void**)&c->sTk, &c->stk_el, nt, (size_t)nt * sizeof(int))) return rc;
    if (!c->sB) {
      // B (K + 1, Mp), the pivot's history (K, GDRF_SELECT_MAX_PICKS) and its variances (K); the partials; their indices and the picks
      const size_t nb = (size_t)(K + 1) * Mp + (size_t)K * GDRF_SELECT_MAX_PICKS + K;
      if (int rc = ctx_alloc(c, &c->sB, nb * sizeof(TS), "hipMalloc(batch choice)")) return rc;
      if (int rc = ctx_alloc(c, &c->sPg, (size_t)GDRF_SEL_PARTS * sizeof(double), "hipMalloc(batch choice)")) return rc;
      if (int rc = ctx_alloc(c, &c->sPi, (size_t)(GDRF_SEL_PARTS + GDRF_SELECT_MAX_PICKS) * sizeof(long long), "hipMalloc(batch choice)")) return rc;
    }
    const T* Xa = X;
    if (G > 0) {
      const size_t row = (size_t)c->Dr * c->esz;
      if (int rc = joint_buf(c, &c->sX, &c->sxrows, nt, (size_t)nt * row)) return rc;
      HIPCHK(hipMemcpyAsync(c->sX, X, (size_t)n * row, hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemcpyAsync((char*)c->sX + (size_t)n * row, given, (size_t)G * row, hipMemcpyDeviceToDevice, s));
      Xa = (const T*)c->sX;
    }
    c->jlast_n = c->jlast_sk = 0;              // W is about to be rewritten: no gdrf_sample_joint_retry on the old one
    if (int rc = joint_w(c, Xa, nt, params, s)) return rc;
    const T* Xc = c->per ? (const T*)c->Xe : Xa;
    TS* B = Q(c->sB);
    TS* hp = B + (size_t)(K + 1) * Mp;
    TS* dp = hp + (size_t)K * GDRF_SELECT_MAX_PICKS;
    long long* picks = c->sPi + GDRF_SEL_PARTS;
    const int nparts = (int)std::min<int64_t>((nt + GDRF_SEL_ROWS - 1) / GDRF_SEL_ROWS, GDRF_SEL_PARTS);
    hipLaunchKernelGGL((select_init_kernel<TS, T>), dim3((unsigned)nparts), dim3(256), 0, s, n, nt, K, (const Hyper*)c->hyp, (const T*)P(c->qpart), nct<TS>(c),
                       (const T*)P(c->tt), c->ldk, noise, Q(c->sD), c->sTk, c->sPg, c->sPi);
    SelPrep<TS, T> pr{0, G, K, M, Mp, Tm, nparts, n, nt, c->sPg, c->sPi, (const TS*)Q(c->jW), (const T*)P(c->S), (const T*)P(c->ST), (const TS*)Q(c->sC),
                      (const TS*)Q(c->sD), B, hp, dp, picks, c->sTk, (long long*)idx_out, gains_out};
    SelPass<TS, T> ps{0, K, Mp, Tm, c->D, c->kind, n, nt, noise, (const Hyper*)c->hyp, Xc, (const TS*)Q(c->jW), (const TS*)B, (const TS*)hp,
                      (const TS*)dp, Q(c->sC), Q(c->sD), picks, c->sTk, c->sPg, c->sPi};
    for (int t = 0; t < Tm; ++t) {
      pr.t = ps.t = t;
      if (int rc = launch_lds((select_prep_kernel<TS, T>), dim3((unsigned)K), dim3(256), (size_t)2 * Mp * sizeof(TS), s, pr)) return rc;
      if (int rc = ard_fwd(c) ? launch_lds((select_pass_kernel<TS, T, true>), dim3((unsigned)nparts), dim3(256), pass_lds, s, ps)
                              : launch_lds((select_pass_kernel<TS, T, false>), dim3((unsigned)nparts), dim3(256), pass_lds, s, ps)) return rc;
    }
    if (var_out)
      hipLaunchKernelGGL(select_var_out_kernel<TS>, dim3((unsigned)((n + 255) / 256), (unsigned)K), dim3(256), 0, s, (const TS*)Q(c->sD), n, nt, var_out);
    LAUNCHCHK("select_batch");
    return 0;
  }

  // ---- the greedy conditional-variance choice of inducing points (select_inducing.h): no factorisation, no forward.  The hyper-parameter block
  // and, in periodic and product contexts, the embedded rows are the call's own: the context's (c->hyp, c->Xe) belong to its factorisation and
  // its steps.  Everything the call needs is one block of device memory, released before it returns: (G + count + 1)(n + G) solve-precision
  // elements and the small pieces behind them.
  static int select_inducing(gdrf_ctx* c, const T* X, int64_t n, const T* params, const T* given, int G, int count, double floor, int64_t* idx_out,
                             double* pivots_out, double* trace_out, double* resid_out, int* rank_out, hipStream_t s) {
    const int Tm = G + count;
    const int64_t nt = n + G, ntiles = (nt + GDRF_IND_ROWS - 1) / GDRF_IND_ROWS;
    const int nparts = (int)std::min<int64_t>(ntiles, GDRF_IND_PARTS);
    const size_t row = (size_t)c->Dr * c->esz;
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t o = off; off = (size_t)round_up((int64_t)(off + bytes), 256); return o; };
    const size_t oC = take((size_t)Tm * nt * sizeof(TS)), oD = take((size_t)nt * sizeof(TS)), oTk = take((size_t)nt * sizeof(int));
    const size_t oX = take(G > 0 ? (size_t)nt * row : 0), oXe = take(c->per ? (size_t)nt * c->D * c->esz : 0);
    const size_t oHp = take((size_t)GDRF_INDUCING_MAX_PICKS * sizeof(TS)), oPg = take((size_t)nparts * sizeof(double));
    const size_t oPi = take((size_t)nparts * sizeof(long long)), oTr = take((size_t)ntiles * sizeof(double));
    const size_t oPk = take(sizeof(IndPick)), oH = take(sizeof(HyperPer));
    struct Block {            // released on every way out, once the stream has finished with it
      char* p = nullptr; hipStream_t s;
      ~Block() { if (p) { (void)hipStreamSynchronize(s); (void)hipFree(p); } }
    } blk;
    blk.s = s;
    {
      hipError_t e = hipMalloc((void**)&blk.p, off);
      if (e != hipSuccess) { blk.p = nullptr; return fail(-(int)e - 1000, "hipMalloc(inducing choice)", hipGetErrorString(e)); }
    }
    char* b = blk.p;
    TS* cbuf = Q(b + oC);
    TS* d = Q(b + oD);
    int* taken = (int*)(b + oTk);
    TS* hp = Q(b + oHp);
    double* part_g = (double*)(b + oPg);
    long long* part_i = (long long*)(b + oPi);
    double* part_tr = (double*)(b + oTr);
    IndPick* pick = (IndPick*)(b + oPk);
    Hyper* h = (Hyper*)(b + oH);
    const T* Xa = X;
    if (G > 0) {
      HIPCHK(hipMemcpyAsync(b + oX, X, (size_t)n * row, hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemcpyAsync(b + oX + (size_t)n * row, given, (size_t)G * row, hipMemcpyDeviceToDevice, s));
      Xa = (const T*)(b + oX);
    }
    if (c->per) {
      const CoordTab tb = coord_tab(c);
      const int64_t nx = nt * tb.nsrc;
      hipLaunchKernelGGL(prep_hyper_per_kernel<T>, dim3(1), dim3(64), 0, s, params, tb, (HyperPer*)h);
      hipLaunchKernelGGL((embed_per_kernel<T, T>), dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, s, nt, tb, Xa, params, (T*)(b + oXe), (T*)nullptr);
      Xa = (const T*)(b + oXe);
    } else if (c->ard) {
      hipLaunchKernelGGL(prep_hyper_ard_kernel<T>, dim3(1), dim3(64), 0, s, params, params + param_lay(c).ard, c->D, h);
    } else {
      hipLaunchKernelGGL(prep_hyper_kernel<T>, dim3(1), dim3(64), 0, s, params, h);
    }
    hipLaunchKernelGGL(inducing_init_kernel<TS>, dim3((unsigned)nparts), dim3(256), 0, s, n, nt, c->kind, (const Hyper*)h, d, taken, part_g, part_i, part_tr);
    IndPrep<TS> pr{0, G, Tm, nparts, n, nt, ntiles, floor, part_g, part_i, part_tr, (const TS*)cbuf, (const TS*)d, hp, pick, taken,
                   (long long*)idx_out, pivots_out, trace_out, rank_out};
    IndPass<TS, T> ps{0, c->D, c->kind, n, nt, (const Hyper*)h, Xa, (const TS*)hp, (const IndPick*)pick, cbuf, d, taken, part_g, part_i, part_tr};
    for (int t = 0; t <= Tm; ++t) {           // t = Tm: the trace of the last pass
      pr.t = ps.t = t;
      hipLaunchKernelGGL(inducing_prep_kernel<TS>, dim3(1), dim3(256), 0, s, pr);
      if (t == Tm) break;
      const size_t lds = (size_t)t * sizeof(TS);
      if (ard_fwd(c)) hipLaunchKernelGGL((inducing_pass_kernel<TS, T, true>), dim3((unsigned)nparts), dim3(256), lds, s, ps);
      else hipLaunchKernelGGL((inducing_pass_kernel<TS, T, false>), dim3((unsigned)nparts), dim3(256), lds, s, ps);
    }
    if (resid_out) hipLaunchKernelGGL(inducing_resid_out_kernel<TS>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const TS*)d, n, resid_out);
    LAUNCHCHK("select_inducing");
    HIPCHK(hipStreamSynchronize(s));
    return 0;
  }
};


int gdrf_knm(gdrf_ctx* c, const void* X, int64_t n, const void* Z, const void* params, void* out, int64_t ldo, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  hipStream_t s = (hipStream_t)stream;
  if (c->dtype == GDRF_F64) return Impl<double, double>::knm(c, (const double*)X, n, (const double*)Z, (const double*)params, (double*)out, ldo, s);
  return Impl<float, float>::knm(c, (const float*)X, n, (const float*)Z, (const float*)params, (float*)out, ldo, s);
}

int gdrf_fill_eps(gdrf_ctx* c, uint64_t seed, uint32_t step, int64_t n_offset, int64_t n, void* eps, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)((n + 255) / 256), c->K);
  if (c->esz == 4) hipLaunchKernelGGL(fill_eps_kernel<float>, grid, dim3(256), 0, s, seed, step, n_offset, n, c->K, (float*)eps, n);
  else hipLaunchKernelGGL(fill_eps_kernel<double>, grid, dim3(256), 0, s, seed, step, n_offset, n, c->K, (double*)eps, n);
  LAUNCHCHK("fill_eps");
  return 0;
}

// red_d (red_nd(c) doubles) -> tail of red_T, and back after the all-reduce
int gdrf_payload_pack(gdrf_ctx* c, void* redT, const double* redd, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  const int nd = (int)red_nd(c);
  if (c->esz == 8) hipLaunchKernelGGL(payload_pack_kernel<double>, dim3((nd + 255) / 256), dim3(256), 0, (hipStream_t)stream, redd, nd, (double*)redT + red_lay(c).tail);
  else hipLaunchKernelGGL(payload_pack_kernel<float>, dim3((nd + 255) / 256), dim3(256), 0, (hipStream_t)stream, redd, nd, (float*)redT + red_lay(c).tail);
  LAUNCHCHK("payload_pack");
  return 0;
}
int gdrf_payload_unpack(gdrf_ctx* c, const void* redT, double* redd, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  const int nd = (int)red_nd(c);
  if (c->esz == 8) hipLaunchKernelGGL(payload_unpack_kernel<double>, dim3((nd + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const double*)redT + red_lay(c).tail, nd, redd);
  else hipLaunchKernelGGL(payload_unpack_kernel<float>, dim3((nd + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)redT + red_lay(c).tail, nd, redd);
  LAUNCHCHK("payload_unpack");
  return 0;
}

int gdrf_set_allreduce(gdrf_ctx* c, gdrf_allreduce_fn fn, void* user) {
  c->allreduce = fn; c->allreduce_user = user;
  return 0;
}
// the step's single collective: pack red_d into the tail of red_T, the caller's sum over the ranks on the whole flat buffer, unpack
int gdrf_payload_allreduce(gdrf_ctx* c, void* redT, double* redd, void* stream) {
  if (!c->allreduce) return 0;
  if (int rc = gdrf_payload_pack(c, redT, redd, stream)) return rc;
  const int rc = c->allreduce(redT, red_lay(c).total, c->esz == 8 ? 1 : 0, stream, c->allreduce_user);
  if (rc) return fail(-2, "gdrf_payload_allreduce", "the registered all-reduce function reported an error");
  return gdrf_payload_unpack(c, redT, redd, stream);
}

int gdrf_ll_const_dev(gdrf_ctx* c, const int32_t* ws, int64_t n, double* out_dev, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  hipStream_t s = (hipStream_t)stream;
  if (int rc = counts_check(c, ws, n, "gdrf_ll_const")) return rc;
  int64_t blocks = (n + 255) / 256; if (blocks > 2048) blocks = 2048; if (blocks < 1) blocks = 1;
  if (c->csr_crow) {
    blocks = std::max<int64_t>(1, std::min<int64_t>((n + 15) / 16, 2048));
    hipLaunchKernelGGL(ll_const_csr_kernel, dim3((unsigned)blocks), dim3(256), 0, s, c->csr_crow, c->csr_val, n, c->csr_nnz, c->llpart);
  } else {
    hipLaunchKernelGGL(ll_const_kernel, dim3((unsigned)blocks), dim3(256), 0, s, ws, n, c->V, c->llpart);
  }
  hipLaunchKernelGGL(reduce_dparts_kernel, dim3(1), dim3(1024), 0, s, c->llpart, blocks, 1, out_dev);
  LAUNCHCHK("ll_const");
  return 0;
}

int gdrf_ll_const(gdrf_ctx* c, const int32_t* ws, int64_t n, double* out_host, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (int rc = gdrf_ll_const_dev(c, ws, n, c->dsmall + 8, stream)) return rc;
  HIPCHK(hipMemcpyAsync(out_host, c->dsmall + 8, sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

#define TYPED3(c, fn, ...)                                                                                         \
  do {                                                                                                             \
    if ((c)->dtype == GDRF_F32) { using T = float; using I = Impl<float, double>; return I::fn(__VA_ARGS__); }     \
    if ((c)->dtype == GDRF_F64) { using T = double; using I = Impl<double, double>; return I::fn(__VA_ARGS__); }   \
    { using T = float; using I = Impl<float, float>; return I::fn(__VA_ARGS__); }                                  \
  } while (0)

static int probe_dispatch(gdrf_ctx* c, const void* Z, const void* params, const double* jitters, int nlev, hipStream_t s) {
  TYPED3(c, probe, c, (const T*)Z, (const T*)params, jitters, nlev, s);
}

int gdrf_probe(gdrf_ctx* c, const void* Z, const void* params, const double* jitters, int nlev, int* failed_host, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  if (nlev < 1 || nlev > 8) return fail(-1, "gdrf_probe", "nlev must be in [1, 8]");
  hipStream_t s = (hipStream_t)stream;
  int rc = probe_dispatch(c, Z, params, jitters, nlev, s);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(failed_host, c->flag + 8, sizeof(int) * nlev, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

// the two halves of gdrf_probe: the launch alone (asynchronous), and the read of its flags (waits for the stream)
int gdrf_probe_launch(gdrf_ctx* c, const void* Z, const void* params, const double* jitters, int nlev, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  if (nlev < 1 || nlev > 8) return fail(-1, "gdrf_probe_launch", "nlev must be in [1, 8]");
  return probe_dispatch(c, Z, params, jitters, nlev, (hipStream_t)stream);
}
int gdrf_probe_read(gdrf_ctx* c, int nlev, int* failed_host, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  if (nlev < 1 || nlev > 8) return fail(-1, "gdrf_probe_read", "nlev must be in [1, 8]");
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(failed_host, c->flag + 8, sizeof(int) * nlev, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

int gdrf_factorize(gdrf_ctx* c, const void* Z, const void* params, double jitter, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  hipStream_t s = (hipStream_t)stream;
  TYPED3(c, factorize, c, (const T*)Z, (const T*)params, jitter, s);
}

int gdrf_factorize_mode(gdrf_ctx* c, const void* Z, const void* params, double jitter, void* stream, int mode) {
  HIPCHK(hipSetDevice(c->dev));
  if (mode < 0 || mode > 2) return fail(-1, "gdrf_factorize_mode", "mode must be 0, 1 or 2");
  hipStream_t s = (hipStream_t)stream;
  TYPED3(c, factorize, c, (const T*)Z, (const T*)params, jitter, s, mode);
}

int gdrf_step_local(gdrf_ctx* c, const void* X, const int32_t* ws, const void* eps, int64_t n, const void* Z, const void* params,
                    void* redT, double* redd, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  if (n < 1 || n > c->ncap) return fail(-1, "gdrf_step_local", "n_local outside [1, n_cap]");
  if (int rc = counts_check(c, ws, n, "gdrf_step_local")) return rc;
  hipStream_t s = (hipStream_t)stream;
  TYPED3(c, step_local, c, (const T*)X, ws, (const T*)eps, n, (const T*)Z, (const T*)params, (T*)redT, redd, s);
}

int gdrf_step_local_link(gdrf_ctx* c, const void* X, const int32_t* ws, const void* eps, int64_t n, const void* Z, const void* params,
                         void* redT, double* redd, void* stream, int phase, const void* ext, int64_t ext_ld) {
  HIPCHK(hipSetDevice(c->dev));
  if (n < 1 || n > c->ncap) return fail(-1, "gdrf_step_local_link", "n_local outside [1, n_cap]");
  if (phase < 0 || phase > 2) return fail(-1, "gdrf_step_local_link", "phase must be 0, 1 or 2");
  if (int rc = counts_check(c, ws, n, "gdrf_step_local_link")) return rc;
  if (phase > 0 && (!ext || ext_ld < n)) return fail(-1, "gdrf_step_local_link", "phases 1 and 2 take a (K, ext_ld >= n) array");
  hipStream_t s = (hipStream_t)stream;
  TYPED3(c, step_local_link, c, (const T*)X, ws, (const T*)eps, n, (const T*)Z, (const T*)params, (T*)redT, redd, s, phase, (const T*)ext, ext_ld);
}

int gdrf_step_local2(gdrf_ctx* c, const void* X_model, const void* X_guide, const int32_t* ws, const void* eps, int64_t n, const void* Z,
                     const void* params, void* redT, double* redd, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  if (n < 1 || n > c->ncap) return fail(-1, "gdrf_step_local2", "n_local outside [1, n_cap]");
  if (c->Tst) return fail(-1, "gdrf_step_local2", "needs the dense Wbar form (GDRF_STORE_T_OFF)");
  if (int rc = counts_check(c, ws, n, "gdrf_step_local2")) return rc;
  hipStream_t s = (hipStream_t)stream;
  TYPED3(c, step_local2, c, (const T*)X_model, (const T*)X_guide, ws, (const T*)eps, n, (const T*)Z, (const T*)params, (T*)redT, redd, s);
}

int gdrf_step_finish(gdrf_ctx* c, const void* Z, const void* params, const void* redT, const double* redd, double n_global,
                     double ll_const, void* grads, double* out_d, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  hipStream_t s = (hipStream_t)stream;
  TYPED3(c, step_finish, c, (const T*)Z, (const T*)params, (const T*)redT, redd, n_global, ll_const, (T*)grads, out_d, s);
}

int gdrf_adam(gdrf_ctx* c, int mode, void* params, const void* grads, void* m, void* v, int64_t t, double lr, double b1, double b2,
              double eps, double wd, double clip, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = param_lay(c).total;
  const double bc1 = 1.0 - std::pow(b1, (double)t), bc2 = 1.0 - std::pow(b2, (double)t);
  dim3 grid((unsigned)((n + 255) / 256));
  ScopedTimer tm(c, 14, s);
  if (c->esz == 4)
    hipLaunchKernelGGL(adam_kernel<float>, grid, dim3(256), 0, s, n, (float*)params, (const float*)grads, (float*)m, (float*)v, mode, lr,
                       b1, b2, eps, wd, clip, bc1, bc2, (const int*)c->flag);
  else
    hipLaunchKernelGGL(adam_kernel<double>, grid, dim3(256), 0, s, n, (double*)params, (const double*)grads, (double*)m, (double*)v, mode,
                       lr, b1, b2, eps, wd, clip, bc1, bc2, (const int*)c->flag);
  LAUNCHCHK("adam");
  return 0;
}

int gdrf_optim_step(gdrf_ctx* c, int rule, const gdrf_opt_seg* segs, int nseg, void* params, const void* grads, void* s1, void* s2, void* s3,
                    void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  if (rule < GDRF_ADAM || rule > GDRF_ADAGRAD_RMSPROP) return fail(-1, "gdrf_optim_step", "unknown rule");
  if (nseg < 0 || (nseg > 0 && !segs)) return fail(-1, "gdrf_optim_step", "segment table");
  if (!params || !grads || !s1 || !s2) return fail(-1, "gdrf_optim_step", "params, grads, s1 and s2 are required");
  const int64_t total = param_lay(c).total;
  // every segment inside the vector, no two overlapping (an element is updated at most once)
  std::vector<std::pair<int64_t, int64_t>> iv;
  int64_t npart = 0;
  for (int k = 0; k < nseg; ++k) {
    const gdrf_opt_seg& g = segs[k];
    if (g.offset < 0 || g.length < 0 || g.offset > total - g.length) return fail(-1, "gdrf_optim_step", "segment outside the parameter vector");
    if ((g.flags & GDRF_OPT_CLIP_NORM) && !(g.clip_norm >= 0)) return fail(-1, "gdrf_optim_step", "clip_norm must be >= 0");
    if ((g.flags & GDRF_OPT_CLIP_VALUE) && !(g.clip_value >= 0)) return fail(-1, "gdrf_optim_step", "clip_value must be >= 0");
    if (rule == GDRF_RMSPROP && (g.flags & GDRF_OPT_MOMENTUM) && (g.flags & GDRF_OPT_CENTERED) && !s3)
      return fail(-1, "gdrf_optim_step", "RMSprop with momentum and centered needs s3");
    if (g.length) iv.push_back({g.offset, g.length});
    if (g.flags & GDRF_OPT_CLIP_NORM) npart += (g.length + OPT_NRM - 1) / OPT_NRM;
  }
  std::sort(iv.begin(), iv.end());
  for (size_t k = 1; k < iv.size(); ++k)
    if (iv[k - 1].first + iv[k - 1].second > iv[k].first) return fail(-1, "gdrf_optim_step", "segments overlap");
  if (npart > c->opt_part_cap) {                 // first use (the partials of all segments of a call fit; chunks reuse the buffer)
    const int64_t cap = total / OPT_NRM + nseg + 1;
    if (int rc = ctx_alloc(c, &c->opt_part, (size_t)cap * sizeof(double), "hipMalloc(opt_part)")) return rc;
    c->opt_part_cap = cap;
  }
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer tm(c, 14, s);
  for (int k0 = 0; k0 < nseg; k0 += OPT_MAX_SEGS) {
    OptTable tab;
    std::memset(&tab, 0, sizeof(tab));
    tab.nseg = std::min(OPT_MAX_SEGS, nseg - k0);
    int64_t ub = 0, nb = 0;
    for (int k = 0; k < tab.nseg; ++k) {
      tab.seg[k] = segs[k0 + k];
      tab.ub[k] = (int)ub; tab.nb[k] = (int)nb;
      ub += (tab.seg[k].length + OPT_UPD - 1) / OPT_UPD;
      if (tab.seg[k].flags & GDRF_OPT_CLIP_NORM) nb += (tab.seg[k].length + OPT_NRM - 1) / OPT_NRM;
    }
    tab.ub[tab.nseg] = (int)ub; tab.nb[tab.nseg] = (int)nb;
    if (ub == 0) continue;
    if (ub > INT32_MAX / 2) return fail(-1, "gdrf_optim_step", "segments too long");
    if (c->esz == 4) {
      if (nb) hipLaunchKernelGGL(opt_sumsq_kernel<float>, dim3((unsigned)nb), dim3(OPT_THREADS), 0, s, tab, (const float*)grads, c->opt_part,
                                 (const int*)c->flag);
      hipLaunchKernelGGL(opt_update_kernel<float>, dim3((unsigned)ub), dim3(OPT_THREADS), 0, s, tab, rule, (float*)params, (const float*)grads,
                         (float*)s1, (float*)s2, (float*)s3, (const double*)c->opt_part, (const int*)c->flag);
    } else {
      if (nb) hipLaunchKernelGGL(opt_sumsq_kernel<double>, dim3((unsigned)nb), dim3(OPT_THREADS), 0, s, tab, (const double*)grads, c->opt_part,
                                 (const int*)c->flag);
      hipLaunchKernelGGL(opt_update_kernel<double>, dim3((unsigned)ub), dim3(OPT_THREADS), 0, s, tab, rule, (double*)params,
                         (const double*)grads, (double*)s1, (double*)s2, (double*)s3, (const double*)c->opt_part, (const int*)c->flag);
    }
    LAUNCHCHK("optim_step");
  }
  return 0;
}

int gdrf_predict(gdrf_ctx* c, const void* X, int64_t n, const void* Z, const void* params, const int32_t* ws, int mode,
                 void* out, double* out_d, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  if (mode < 0 || mode > 4) return fail(-1, "gdrf_predict", "mode");
  if (n < 1) return fail(-1, "gdrf_predict", "n must be >= 1");
  if (mode == 3 && !ws && !c->csr_crow) return fail(-1, "gdrf_predict", "perplexity needs ws");
  if (mode == 3)
    if (int rc = counts_check(c, ws, n, "gdrf_predict")) return rc;
  hipStream_t s = (hipStream_t)stream;
  TYPED3(c, predict, c, (const T*)X, n, (const T*)Z, (const T*)params, ws, mode, (T*)out, out_d, s);
}

int gdrf_predict_mc(gdrf_ctx* c, const void* X, int64_t n, const void* Z, const void* params, const int32_t* ws, int mode, int num_samples,
                    uint64_t seed, int64_t row_offset, const void* eps, void* out, double* out_d, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  if (mode < 0 || mode > 3) return fail(-1, "gdrf_predict_mc", "mode");
  if (n < 1) return fail(-1, "gdrf_predict_mc", "n must be >= 1");
  if (n > c->ncap) return fail(-1, "gdrf_predict_mc", "needs n <= n_cap");
  if (num_samples < 1) return fail(-1, "gdrf_predict_mc", "num_samples must be >= 1");
  if (row_offset < 0) return fail(-1, "gdrf_predict_mc", "row_offset must be >= 0");
  if (mode == MC_SCORE && c->csr_crow) return fail(-1, "gdrf_predict_mc", "the predictive score reads dense counts: clear the CSR binding");
  if (mode == MC_SCORE && (!ws || !out_d)) return fail(-1, "gdrf_predict_mc", "the predictive score needs ws and out_d");
  if (mode != MC_SCORE && !out) return fail(-1, "gdrf_predict_mc", "out is required");
  hipStream_t s = (hipStream_t)stream;
  TYPED3(c, predict_mc, c, (const T*)X, n, (const T*)Z, (const T*)params, ws, mode, num_samples, seed, row_offset, (const T*)eps, (T*)out, out_d, s);
}

int gdrf_predict_info(gdrf_ctx* c, const void* X, int64_t n, const void* Z, const void* params, int num_samples, uint64_t seed,
                      int64_t row_offset, const void* eps, double* out, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  if (n < 1) return fail(-1, "gdrf_predict_info", "n must be >= 1");
  if (n > c->ncap) return fail(-1, "gdrf_predict_info", "needs n <= n_cap");
  if (num_samples < 1) return fail(-1, "gdrf_predict_info", "num_samples must be >= 1");
  if (row_offset < 0) return fail(-1, "gdrf_predict_info", "row_offset must be >= 0");
  if (!out) return fail(-1, "gdrf_predict_info", "out is required");
  hipStream_t s = (hipStream_t)stream;
  TYPED3(c, predict_info, c, (const T*)X, n, (const T*)Z, (const T*)params, num_samples, seed, row_offset, (const T*)eps, out, s);
}

int gdrf_predict_score(gdrf_ctx* c, const void* X, int64_t n, const void* Z, const void* params, const int32_t* ws, const int64_t* crow,
                       const int32_t* col, const int32_t* val, int num_samples, uint64_t seed, int64_t row_offset, const void* eps, double* out,
                       void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  if (n < 1) return fail(-1, "gdrf_predict_score", "n must be >= 1");
  if (n > c->ncap) return fail(-1, "gdrf_predict_score", "needs n <= n_cap");
  if (num_samples < 1) return fail(-1, "gdrf_predict_score", "num_samples must be >= 1");
  if (num_samples > 65535) return fail(-1, "gdrf_predict_score", "a call takes at most 65535 samples");
  if (row_offset < 0) return fail(-1, "gdrf_predict_score", "row_offset must be >= 0");
  if ((ws != nullptr) == (crow != nullptr)) return fail(-1, "gdrf_predict_score", "needs the counts either dense (ws_dev) or CSR (crow_dev)");
  if (crow && (!col || !val)) return fail(-1, "gdrf_predict_score", "CSR counts need col_dev and val_dev");
  if (!out) return fail(-1, "gdrf_predict_score", "out is required");
  hipStream_t s = (hipStream_t)stream;
  TYPED3(c, predict_score, c, (const T*)X, n, (const T*)Z, (const T*)params, ws, crow, col, val, num_samples, seed, row_offset, (const T*)eps, out, s);
}

// the argument errors gdrf_predict_loo and gdrf_psis_rows share
static int loo_args(const char* fn, int64_t n, int num_samples, int tail_len, const double* out) {
  if (n < 1) return fail(-1, fn, "n must be >= 1");
  if (num_samples < GDRF_LOO_MIN_SAMPLES || num_samples > GDRF_LOO_MAX_SAMPLES)
    return fail(-1, fn, "num_samples must be in GDRF_LOO_MIN_SAMPLES .. GDRF_LOO_MAX_SAMPLES (25 .. 1024)");
  if (tail_len != forms::loo_tail_len(num_samples)) return fail(-1, fn, "tail_len must be ceil(min(num_samples / 5, 3 sqrt(num_samples)))");
  if (!out) return fail(-1, fn, "out is required");
  return 0;
}

int gdrf_predict_loo(gdrf_ctx* c, const void* X, int64_t n, const void* Z, const void* params, const int32_t* ws, const int64_t* crow,
                     const int32_t* col, const int32_t* val, int num_samples, int tail_len, uint64_t seed, int64_t row_offset, const void* eps,
                     double* out, double* a_out, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  if (int rc = loo_args("gdrf_predict_loo", n, num_samples, tail_len, out)) return rc;
  if (n > c->ncap) return fail(-1, "gdrf_predict_loo", "needs n <= n_cap");
  if (row_offset < 0) return fail(-1, "gdrf_predict_loo", "row_offset must be >= 0");
  if ((ws != nullptr) == (crow != nullptr)) return fail(-1, "gdrf_predict_loo", "needs the counts either dense (ws_dev) or CSR (crow_dev)");
  if (crow && (!col || !val)) return fail(-1, "gdrf_predict_loo", "CSR counts need col_dev and val_dev");
  hipStream_t s = (hipStream_t)stream;
  TYPED3(c, predict_loo, c, (const T*)X, n, (const T*)Z, (const T*)params, ws, crow, col, val, num_samples, seed, row_offset, (const T*)eps, out, a_out, s);
}

int gdrf_psis_rows(gdrf_ctx* c, const double* log_lik, int num_samples, int tail_len, int64_t n, double* out, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  if (int rc = loo_args("gdrf_psis_rows", n, num_samples, tail_len, out)) return rc;
  if (!log_lik) return fail(-1, "gdrf_psis_rows", "log_lik is required");
  const forms::LooPlan pl = forms::loo_plan(0, 0, num_samples, 0, PSIS_LG, true);
  c->loo_plan[0] = pl.RP; c->loo_plan[1] = (int)pl.lds;
  const int64_t nblk = (n + pl.RP - 1) / pl.RP;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(nblk, 1024));
  if (int rc = launch_lds(psis_rows_kernel<PSIS_LG>, dim3(grid), dim3(256), pl.lds, (hipStream_t)stream, n, num_samples, pl.RP, pl.P, pl.M, pl.stride,
                          log_lik, out)) return rc;
  LAUNCHCHK("psis_rows");
  return 0;
}

int gdrf_predict_quant(gdrf_ctx* c, const void* X, int64_t n, const void* Z, const void* params, int mode, int num_samples, uint64_t seed,
                       int64_t row_offset, const void* eps, const double* levels, int nlevels, const int32_t* words, int nwords, double* out,
                       void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  const char* fn = "gdrf_predict_quant";
  if (mode < QUANT_Q || mode > QUANT_DOMINANT) return fail(-1, fn, "mode");
  if (n < 1) return fail(-1, fn, "n must be >= 1");
  if (n > c->ncap) return fail(-1, fn, "needs n <= n_cap");
  if (num_samples < 1) return fail(-1, fn, "num_samples must be >= 1");
  if (mode == QUANT_Q && num_samples > GDRF_QUANT_MAX_SAMPLES) return fail(-1, fn, "the quantile mode takes at most GDRF_QUANT_MAX_SAMPLES samples");
  if (mode != QUANT_Q && num_samples > 65535) return fail(-1, fn, "a call takes at most 65535 samples");
  if (row_offset < 0) return fail(-1, fn, "row_offset must be >= 0");
  if (nwords < 0 || (nwords > 0) != (words != nullptr)) return fail(-1, fn, "words_dev and nwords go together");
  if (mode == QUANT_DOMINANT && nwords) return fail(-1, fn, "the dominant-topic mode is over topics: no words");
  if (mode == QUANT_DOMINANT ? nlevels != 0 : (nlevels < 1 || nlevels > GDRF_QUANT_MAX_LEVELS || !levels))
    return fail(-1, fn, "needs 1 .. GDRF_QUANT_MAX_LEVELS levels (none for the dominant-topic mode)");
  if (!out) return fail(-1, fn, "out is required");
  QuantLevels lev{};
  for (int t = 0; t < nlevels; ++t) {
    if (mode == QUANT_Q) {
      if (!(levels[t] >= 0.0 && levels[t] <= 1.0)) return fail(-1, fn, "a quantile level must be in [0, 1]");
      const double hh = levels[t] * (double)(num_samples - 1), lo = std::floor(hh);
      lev.lo[t] = (int)lo; lev.v[t] = hh - lo;
    } else {
      if (!std::isfinite(levels[t])) return fail(-1, fn, "a threshold must be finite");
      lev.v[t] = levels[t];
    }
  }
  hipStream_t s = (hipStream_t)stream;
  TYPED3(c, predict_quant, c, (const T*)X, n, (const T*)Z, (const T*)params, mode, num_samples, seed, row_offset, (const T*)eps, lev, nlevels, words,
         nwords, out, s);
}

int gdrf_fold_in(gdrf_ctx* c, const void* X, int64_t n, const void* Z, const void* params, const int32_t* ws, const int64_t* crow, const int32_t* col,
                 const int32_t* val, const int32_t* ws2, const int64_t* crow2, const int32_t* col2, const int32_t* val2, int mode, int num_iters,
                 double tol, void* out, double* diag, double* out_d, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  if (mode < 0 || mode > 3) return fail(-1, "gdrf_fold_in", "mode");
  if (n < 1) return fail(-1, "gdrf_fold_in", "n must be >= 1");
  if (n > c->ncap) return fail(-1, "gdrf_fold_in", "needs n <= n_cap");
  if (num_iters < 0) return fail(-1, "gdrf_fold_in", "num_iters must be >= 0");
  if (!(tol >= 0) || !std::isfinite(tol)) return fail(-1, "gdrf_fold_in", "tol must be finite and >= 0");
  if ((ws != nullptr) == (crow != nullptr)) return fail(-1, "gdrf_fold_in", "needs the counts either dense (ws_dev) or CSR (crow_dev)");
  if (crow && (!col || !val)) return fail(-1, "gdrf_fold_in", "CSR counts need col_dev and val_dev");
  if (mode == FI_SCORE) {
    if (!out_d) return fail(-1, "gdrf_fold_in", "the score needs out_d");
    if (!ws2 && !crow2) { ws2 = ws; crow2 = crow; col2 = col; val2 = val; }
    if ((ws2 != nullptr) != (ws != nullptr) || (crow2 != nullptr) != (crow != nullptr) || (crow2 && (!col2 || !val2)))
      return fail(-1, "gdrf_fold_in", "the scored counts must have the layout of the fitted ones");
  } else if (!out) return fail(-1, "gdrf_fold_in", "out is required");
  if (!diag) return fail(-1, "gdrf_fold_in", "diag is required");
  hipStream_t s = (hipStream_t)stream;
  TYPED3(c, fold_in, c, (const T*)X, n, (const T*)Z, (const T*)params, ws, crow, col, val, ws2, crow2, col2, val2, mode, num_iters, tol, (T*)out, diag,
         out_d, s);
}

int gdrf_sample_counts(gdrf_ctx* c, const void* theta, int64_t n, const void* params, const int32_t* totals, int tmax, const int32_t* ws, int mode,
                       int num_samples, uint64_t seed, int64_t row_offset, double* u, int32_t* out, double* dev, int64_t* zeros, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  if (mode < 0 || mode > 2) return fail(-1, "gdrf_sample_counts", "mode");
  if (n < 1) return fail(-1, "gdrf_sample_counts", "n must be >= 1");
  if (num_samples < 1) return fail(-1, "gdrf_sample_counts", "num_samples must be >= 1");
  if (num_samples > 65535) return fail(-1, "gdrf_sample_counts", "a call takes at most 65535 samples");
  if (row_offset < 0) return fail(-1, "gdrf_sample_counts", "row_offset must be >= 0");
  if (tmax < 0) return fail(-1, "gdrf_sample_counts", "totals must be non-negative (tmax < 0)");
  hipStream_t s = (hipStream_t)stream;
  if (mode == SC_UNIFORMS) {
    if (!u) return fail(-1, "gdrf_sample_counts", "the uniforms need u_dev to be written to");
    const int64_t nthr = n * ((tmax + 3) / 4);
    if (nthr > (int64_t)256 * 0x7fffffff) return fail(-1, "gdrf_sample_counts", "n x tmax too large for one call");
    if (nthr > 0)
      hipLaunchKernelGGL(sc_fill_uniforms_kernel, dim3((unsigned)((nthr + 255) / 256), (unsigned)num_samples), dim3(256), 0, s, seed, row_offset, n, tmax, u);
    LAUNCHCHK("sample_counts");
    return 0;
  }
  if (c->V > GDRF_SC_MAX_V)
    return fail(-1, "gdrf_sample_counts", "num_observation_categories exceeds the limit of 4096 words (one wave's CDF, counts and p live in LDS)");
  if (c->K > GDRF_SC_KP) return fail(-1, "gdrf_sample_counts", "num_topic_categories exceeds the 128 topics a wave holds in LDS");
  if (!theta || !params || !totals) return fail(-1, "gdrf_sample_counts", "theta, params and totals are required");
  if (mode == SC_STATS && (!ws || !dev || !zeros)) return fail(-1, "gdrf_sample_counts", "the check statistics need ws, dev and zeros");
  if (mode == SC_COUNTS && !out) return fail(-1, "gdrf_sample_counts", "out is required");
  TYPED3(c, sample_counts, c, (const T*)theta, n, (const T*)params, totals, tmax, ws, mode, num_samples, seed, row_offset, (const double*)u, out, dev,
         zeros, s);
}

// the shape limits of the joint calls: the launches index rows and sample-topic pairs with a 16-bit grid dimension
static int joint_check(const gdrf_ctx* c, const char* fn, int64_t n, int64_t nsk) {
  if (n < 1) return fail(-1, fn, "n must be >= 1");
  if (n > c->ncap) return fail(-1, fn, "needs n <= n_cap");
  if (n > 65535 - 32 || nsk > 65535) return fail(-1, fn, "a joint call takes at most 65503 rows and 65535 (sample, topic) pairs");
  return 0;
}

int gdrf_predict_cov(gdrf_ctx* c, const void* X, int64_t n, const void* Z, const void* params, int which, void* out, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  if (which != COV_FULL && which != COV_RESID) return fail(-1, "gdrf_predict_cov", "which");
  if (int rc = joint_check(c, "gdrf_predict_cov", n, 1)) return rc;
  if (!out) return fail(-1, "gdrf_predict_cov", "out is required");
  hipStream_t s = (hipStream_t)stream;
  TYPED3(c, predict_cov, c, (const T*)X, n, (const T*)Z, (const T*)params, which, (T*)out, s);
}

int gdrf_sample_joint(gdrf_ctx* c, const void* X, int64_t n, const void* Z, const void* params, int num_samples, uint64_t seed, const void* xi,
                      const void* zeta, double jitter_total, void* out, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  if (num_samples < 1) return fail(-1, "gdrf_sample_joint", "num_samples must be >= 1");
  if (int rc = joint_check(c, "gdrf_sample_joint", n, (int64_t)num_samples * c->K)) return rc;
  if (!out) return fail(-1, "gdrf_sample_joint", "out is required");
  hipStream_t s = (hipStream_t)stream;
  TYPED3(c, sample_joint, c, (const T*)X, n, (const T*)Z, (const T*)params, num_samples, seed, (const T*)xi, (const T*)zeta, jitter_total, (T*)out, s);
}

int gdrf_sample_joint_retry(gdrf_ctx* c, int64_t n, int num_samples, double jitter_total, void* out, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  if (n < 1 || num_samples < 1 || n != c->jlast_n || (int64_t)num_samples * c->K != c->jlast_sk)
    return fail(-1, "gdrf_sample_joint_retry", "needs the gdrf_sample_joint call with this n and num_samples directly in front of it");
  if (!out) return fail(-1, "gdrf_sample_joint_retry", "out is required");
  hipStream_t s = (hipStream_t)stream;
  TYPED3(c, joint_draw, c, n, num_samples, jitter_total, (T*)out, s);
}

int gdrf_select_batch(gdrf_ctx* c, const void* X, int64_t n, const void* Z, const void* params, const void* given, int G, int count, double noise,
                      int64_t* idx_out, double* gains_out, double* var_out, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  if (n < 1) return fail(-1, "gdrf_select_batch", "n must be >= 1");
  if (G < 0) return fail(-1, "gdrf_select_batch", "G must be >= 0");
  if (n + G > c->ncap) return fail(-1, "gdrf_select_batch", "needs n + G <= n_cap");
  if (count < 1 || count > n) return fail(-1, "gdrf_select_batch", "count must be in [1, n]");
  if (G + count > GDRF_SELECT_MAX_PICKS) return fail(-1, "gdrf_select_batch", "G + count exceeds GDRF_SELECT_MAX_PICKS (256)");
  if (!(noise > 0) || !std::isfinite(noise)) return fail(-1, "gdrf_select_batch", "noise must be positive and finite");
  if (G > 0 && !given) return fail(-1, "gdrf_select_batch", "G > 0 needs given_dev");
  if (!idx_out || !gains_out) return fail(-1, "gdrf_select_batch", "idx_out and gains_out are required");
  hipStream_t s = (hipStream_t)stream;
  TYPED3(c, select_batch, c, (const T*)X, n, (const T*)Z, (const T*)params, (const T*)given, G, count, noise, idx_out, gains_out, var_out, s);
}

int gdrf_select_inducing(gdrf_ctx* c, const void* X, int64_t n, const void* params, const void* given, int G, int count, double floor, int64_t* idx_out,
                         double* pivots_out, double* trace_out, double* resid_out, int* rank_out, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  if (n < 1) return fail(-1, "gdrf_select_inducing", "n must be >= 1");
  if (G < 0) return fail(-1, "gdrf_select_inducing", "G must be >= 0");
  if (n + G > c->ncap) return fail(-1, "gdrf_select_inducing", "needs n + G <= n_cap");
  if (count < 0 || count > n) return fail(-1, "gdrf_select_inducing", "count must be in [0, n]");
  if (G + count < 1) return fail(-1, "gdrf_select_inducing", "needs G + count >= 1");
  if (G + count > GDRF_INDUCING_MAX_PICKS) return fail(-1, "gdrf_select_inducing", "G + count exceeds GDRF_INDUCING_MAX_PICKS (1024)");
  if (!(floor >= 0) || !std::isfinite(floor)) return fail(-1, "gdrf_select_inducing", "floor must be finite and >= 0");
  if (!X || !params) return fail(-1, "gdrf_select_inducing", "X_dev and params_dev are required");
  if (G > 0 && !given) return fail(-1, "gdrf_select_inducing", "G > 0 needs given_dev");
  if (!pivots_out || !trace_out || !rank_out || (count > 0 && !idx_out))
    return fail(-1, "gdrf_select_inducing", "idx_out (count > 0), pivots_out, trace_out and rank_out are required");
  hipStream_t s = (hipStream_t)stream;
  TYPED3(c, select_inducing, c, (const T*)X, n, (const T*)params, (const T*)given, G, count, floor, idx_out, pivots_out, trace_out, resid_out, rank_out, s);
}

int gdrf_joint_failed(gdrf_ctx* c, int* failed, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  hipStream_t s = (hipStream_t)stream;
  *failed = 0;
  if (!c->jflag) return 0;
  HIPCHK(hipMemcpyAsync(failed, c->jflag, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

int gdrf_chol_failed(gdrf_ctx* c, int* failed, void* stream) {
  HIPCHK(hipSetDevice(c->dev));
  hipStream_t s = (hipStream_t)stream;
  if (int rc = join_fact(c, s)) return rc;
  int f17[17];                               // [0] the factorisation failed, [16] a reused factorisation's inputs had changed
  HIPCHK(hipMemcpyAsync(f17, c->flag, sizeof(f17), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *failed = f17[0] | f17[16];
  return 0;
}
