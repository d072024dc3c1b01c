/* libgdrf_hip: C ABI of the MI355X-native GDRF SVI ELBO hot path.
 *
 * The reference (san-soucie/gdrf v0.1.3) is pure Python and has no FFI; the seam this library
 * sits behind is the duck-typed Python surface of SURVEY.md 8(b).  Each entry point below names
 * the reference code (paths under /root/reference) whose work it replaces; the Python mirror in
 * gdrf_amd/ binds them with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions: every function returns 0 on success, < 0 on a HIP/argument error (message from
 * gdrf_last_error()); pointers named *_dev are borrowed device pointers that the caller keeps
 * alive until the stream has been synchronised; `stream` is a hipStream_t passed as void*;
 * no exceptions cross the ABI; one host thread per context.  kernel_id: 0 RBF, 1 Matern52, 2 Matern32, 3 Exponential,
 * 4 RationalQuadratic, 5 Periodic (D <= 2, gdrf_set_period_count), 6 a product of RBF and Periodic factors (gdrf_set_product).
 * dtype fixes the element type of every "void*" real array below:
 *   GDRF_F32 (0)      float arrays.  The K-fold contractions are f32 GEMMs evaluated on the matrix cores in the arithmetic
 *                     gdrf_set_mfma_mode() selects (native f32 MFMA, or split operands on the 16-bit matrix path with f32
 *                     accumulation and f32-level error); the ill-conditioned pieces (K_uu, its Cholesky factor and inverse,
 *                     the solve W = K_nm L^-T, its backward and the M x M epilogue) run in f64, because the fp32 solve
 *                     cancels terms |L^-1||k| >> |w| (DESIGN.md "precision").
 *   GDRF_F64 (1)      double arrays, everything f64.
 *   GDRF_F32_PURE (2) float arrays, everything f32 (the reference's literal .float() arithmetic; for A/B runs).
 */
#ifndef GDRF_HIP_H
#define GDRF_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct gdrf_ctx gdrf_ctx;

enum { GDRF_F32 = 0, GDRF_F64 = 1, GDRF_F32_PURE = 2 };
enum { GDRF_RBF = 0, GDRF_MATERN52 = 1, GDRF_MATERN32 = 2, GDRF_EXPONENTIAL = 3, GDRF_RATIONALQUADRATIC = 4, GDRF_PERIODIC = 5,
       GDRF_PRODUCT = 6 };
enum { GDRF_ADAM = 0, GDRF_ADAMW = 1, GDRF_CLIPPED_ADAM = 2 };
enum { GDRF_PRED_LOC = 0, GDRF_PRED_TOPIC_PROBS = 1, GDRF_PRED_WORD_PROBS = 2, GDRF_PRED_PERPLEXITY = 3, GDRF_PRED_LOC_VAR = 4 };

const char* gdrf_last_error(void);
int gdrf_version(void);

/* Workspaces for at most n_cap local observations.  Replaces the tensors pyro/autograd allocate
 * per step inside SVI.step (gdrf/train_script.py:365-371,467). */
int gdrf_ctx_create(gdrf_ctx** out, int device, int64_t n_cap, int M, int K, int V, int D, int dtype, int kernel_id);
/* As above with an explicit choice for the backward of the variance term: GDRF_STORE_T_ON keeps T_k = W S_k
 * (K*n_cap*M elements) from the forward so that Wbar is the triangular product sum_k diag(2 vbar_k) T_k S_k^T;
 * GDRF_STORE_T_OFF (what gdrf_ctx_create uses) takes the dense form sum_k diag(2 vbar_k) W (S_k S_k^T): twice the
 * MFMA flops, no extra memory, but its A operand is reused across the K topics from LDS -- measured faster on MI355X
 * (43 vs 47 ms at the headline size).  GDRF_STORE_T_AUTO currently resolves to OFF. */
enum { GDRF_STORE_T_OFF = 0, GDRF_STORE_T_ON = 1, GDRF_STORE_T_AUTO = 2 };
int gdrf_ctx_create_ex(gdrf_ctx** out, int device, int64_t n_cap, int M, int K, int V, int D, int dtype, int kernel_id, int store_t);
int gdrf_stores_t(const gdrf_ctx* ctx);
/* Arithmetic of the four f32 GEMM-shaped contractions of the step (tt = |S_k^T w|^2, Wbar, A_k = W^T diag(vbar_k) W,
 * G^T = W^T Wbar) in float contexts (csrc/gemm_split.h):
 *   0  v_mfma_f32_16x16x4_f32 (native f32 MFMA);
 *   1  "bf16x6": each f32 operand as 3 bf16 pieces, the 6 cross products of weight >= 2^-16 on v_mfma_f32_16x16x32_bf16,
 *      f32 accumulation: 16/6 of the f32 MFMA rate;
 *   2  "f16x3": each f32 operand, times one power-of-two block scale that puts its largest magnitude below 2^15, as 2 fp16
 *      pieces (22-23 significand bits), the 3 cross products hh + hl + lh on v_mfma_f32_16x16x32_f16, f32 accumulation, the
 *      scales undone in the epilogues: 16/3 of the f32 MFMA rate.
 * Modes 1 and 2 are held to the error of mode 0 against fp64 products of the same inputs (tests/test_gpu_parity.py).  They
 * need float arrays and the dense Wbar form (GDRF_STORE_T_OFF); a fresh context is in mode 0, gdrf_amd.Engine selects 2 for
 * float32 with the f64 solve by default. */
int gdrf_set_mfma_mode(gdrf_ctx* ctx, int mode);
int gdrf_get_mfma_mode(const gdrf_ctx* ctx);
/* How the K_nm parts of the kernel hyper-parameter gradients (sum Kbar_nm o K_nm, sum Kbar_nm o dK_nm/dlog ls) are formed:
 *   0  (default) Kbar_nm = Wbar L^-1 tile by tile in the solve precision (gemm_nt<BwdKnmProb>, f64 matrix pipe), never stored;
 *   1  no backward solve: sum Kbar o K = sum Wbar o W, and sum Kbar o dK = sum_{i>=j} Linv[i][j] Hd[j][i] with Hd = dK^T Wbar, an M x M
 *      contraction over the rows on the split-fp16 TN kernel (csrc/hyper_tn.h), its contraction with L^-1 in double.  Applies to float arrays
 *      in mode f16x3 with fixed inducing inputs and a kernel other than RationalQuadratic; every other configuration runs form 0.  Faster
 *      (no f64 GEMM), but Hd carries float32-level rounding INTO the cancelling contraction with L^-1: d loss / d log lengthscale is then
 *      accurate to ~4e-4 instead of ~1e-7 at the headline conditioning (tests/test_gpu_round3.py), hence opt-in.
 * gdrf_get_hyper_backward reports the form the next step will actually use. */
int gdrf_set_hyper_backward(gdrf_ctx* ctx, int mode);
int gdrf_get_hyper_backward(const gdrf_ctx* ctx);
/* How the per-row terms that touch the vocabulary (p = theta Phi, the Multinomial log-likelihood, thetabar = Phi pbar, Phi-bar) are formed
 * by gdrf_step_local and gdrf_predict modes 0-3:
 *   0  (default) the LDS forms: the matrix-core row kernel for K <= 32, V <= 64, else one thread per row; each keeps the whole (K, V) Phi
 *      (and most its gradient and a (V + 1) row per thread) in LDS, so K x V is bounded by the LDS budget and larger shapes fail with
 *      "too large".  Their Phi-bar partials take [1024][K][V] elements, allocated on the first call that needs them.
 *   1  vocabulary-streamed (csrc/rows_vstream.h), any V >= 1 and K <= 128: a workgroup keeps only the theta of its 64 rows (K x 64) in
 *      LDS and streams Phi through LDS in tiles of 64 words (float) or 32 (double), each count read once; the V-free terms run in kernels
 *      without any K x V array (csrc/rows_lds.h).  Workspace: a (K, n_cap) array, Phi-bar slots [G][K][V] and [G][K] with
 *      G = min(1024, max(16, 256 MiB / (K V element size)), ceil(n_cap / 64)), all allocated on the first form-1 call.  gdrf_predict
 *      modes 0-1 read no Phi; modes 2-3 stream it over n_cap rows at a time.  Same element type and precision as form 0; sums are
 *      formed in another order, so results agree with form 0 to rounding, and are bit-identical from run to run.
 * gdrf_step_local2 and all three phases of gdrf_step_local_link have the one route of form 1 and take it whatever the form is set to
 * (same kernels, grid and workspace, so the same bits in either form); they have no K x V bound beyond K <= 128.
 * Any other value is an error. */
int gdrf_set_rows_form(gdrf_ctx* ctx, int form);
int gdrf_get_rows_form(const gdrf_ctx* ctx);
/* Sparse counts (csrc/rows_csr.h).  Binds a CSR count matrix of n rows and the context's V columns: crow_dev (n + 1) row pointers with
 * crow[0] = 0 and crow[n] = nnz, col_dev (nnz) column indices in [0, V), val_dev (nnz) counts; all BORROWED device arrays that must stay
 * valid and unchanged while bound.  Column indices need not be sorted inside a row; a stored 0 behaves as an absent entry; duplicate
 * (row, column) entries are not supported.  The column grouping is the caller's to supply: cperm_dev (nnz) lists the CSR positions
 * 0 .. nnz - 1 sorted by (column, row) - a stable sort of col_dev by value - and ccol_dev (V + 1) are the column pointers into it
 * (ccol[v] = the number of entries with a column < v).  The steps need it; gdrf_predict mode 3 and the data constant do not (NULL, NULL).
 * While a matrix is bound, gdrf_step_local, gdrf_step_local2, gdrf_step_local_link, gdrf_predict mode 3, gdrf_ll_const and
 * gdrf_ll_const_dev must be given ws_dev = NULL and n = the bound row count (anything else is an error) and read the bound matrix; the
 * per-row stage then runs the decomposition of row form 1 with its one vocabulary kernel replaced by a row pass over the stored entries
 * and a column pass for Phi-bar, whatever the row form is set to: nnz x K work instead of n x V x K, no dense (n, V) array anywhere.
 * gdrf_predict streams the bound rows n_cap at a time, so there n may exceed n_cap.  Scratch: Phi^T, an (n_cap, K) array, one (K, V) slot,
 * allocated on the first such call; and 8 bytes + an element per stored entry plus K elements per column segment (256 entries), grown with
 * nnz.  Same element type and arithmetic per stored entry as form 1, sums in another order; bit-identical from run to run.
 * crow_dev = NULL clears the binding: every call then does what it does without one. */
int gdrf_bind_counts_csr(gdrf_ctx* ctx, const int64_t* crow_dev, const int32_t* col_dev, const int32_t* val_dev, int64_t n, int64_t nnz,
                         const int64_t* ccol_dev, const int64_t* cperm_dev);
/* whiten = 0: the unwhitened branch of pyro's gp.util.conditional (gdrf/models/sparse_gdrf.py:30,175-185: the
 * constructor's `whiten` argument): u_loc and u_scale_tril parameterise q(f(Z)) itself, the predictive uses
 * L^-1 u_loc and L^-1 u_scale_tril.  Default 1 (whitened), which is what the reference's train() always runs. */
int gdrf_set_whiten(gdrf_ctx* ctx, int whiten);
/* mean_function (gdrf/models/abstract_gdrf.py:17-18,33-48; applied as `f_loc + self._mean_function(xs)` in model and guide,
 * gdrf/models/sparse_gdrf.py:346,395): `mean` is a BORROWED device array of the context's element type holding the values
 * the callable returned for the rows of the next gdrf_step_local call(s), addressed as mean[k*stride_k + n*stride_n]
 * (a stride of 0 broadcasts: the reference's (N,) return value is stride_k = 0, stride_n = 1).  NULL = zero_mean (default).
 * The mean shifts the sampled mu that enters the link; the Normal site terms depend on mu - f_loc only, and - as in the
 * reference - log_topic_probs / the predictive path do not add it (sparse_gdrf.py:161-186). */
int gdrf_set_mean(gdrf_ctx* ctx, const void* mean, int64_t stride_k, int64_t stride_n);
/* Learnable inducing inputs (gdrf/models/sparse_gdrf.py:79-88, fixed_inducing_points=False: a PyroParam under
 * stack([interval(0, 1)] * D), i.e. Z = sigmoid(unconstrained)).  The flat parameter vector always carries an (M, D)
 * block for the unconstrained values, gdrf_inducing_layout -> {offset, M*D}; the caller evaluates Z = sigmoid(block) and
 * passes it as Z_dev as before.  With on = 1, gdrf_step_local additionally accumulates
 * G[j][d] = sum_n Kbar_nm[n][j] dk/dr2 (z_jd - x_nd) into red_d[8 + j*D + d] (all-reduced with the rest) and
 * gdrf_step_finish writes d loss / d unconstrained into the block of grads (K_nm and K_uu paths, sigmoid Jacobian);
 * with on = 0 (default) that block of grads stays zero. */
int gdrf_set_learn_inducing(gdrf_ctx* ctx, int on);
int gdrf_inducing_layout(const gdrf_ctx* ctx, int64_t out[2]);
/* ARD kernels (one lengthscale per input dimension): pyro.contrib.gp.kernels.Isotropy with a lengthscale of shape (input_dim,), whose
 * _scale(X) = X / lengthscale divides every input axis by its own lengthscale before the squared distance
 * r2 = sum_d ((x_d - z_d) / ls_d)^2 (pyro 1.8.0 kernels/isotropic.py; the reference passes a list through
 * wandb.config.kernel_lengthscale, gdrf/train_script.py:290-296).  With on = 1 the flat parameter vector grows by a segment of D
 * log-lengthscales (gdrf_ard_layout -> {offset, D}; {offset of the would-be segment, 0} when off), slot 0 is then unused (its gradient
 * is 0), red_d grows by D doubles at 8 + M*D (the per-axis K_nm sums, all-reduced with the rest), and every covariance evaluation uses the
 * per-axis scales.  Call it before reading gdrf_param_layout / gdrf_red_layout.  The opt-in hyper-gradient form
 * (gdrf_set_hyper_backward(1)) falls back to the default f64 form.  Default 0: the layouts are those of a context that
 * never called it. */
int gdrf_set_ard(gdrf_ctx* ctx, int on);
int gdrf_ard_layout(const gdrf_ctx* ctx, int64_t out[2]);
/* Periodic kernel (kernel_id GDRF_PERIODIC, D <= 2): pyro.contrib.gp.kernels.Periodic,
 * k(x, z) = variance * exp(-2 sum_d sin^2(pi (x_d - z_d) / period_d) / lengthscale_d^2).  It is evaluated as the RBF kernel at lengthscale 1 on
 * the embedded coordinates (cos(t_d x_d), sin(t_d x_d)) / lengthscale_d, t_d = 2 pi / period_d.  The flat parameter vector grows by a segment
 * of log-periods (gdrf_periodic_layout -> {offset, count}; {offset of the would-be segment, 0} in other contexts), right behind the ARD
 * segment when there is one.  Slot 0 holds the log-lengthscale unless gdrf_set_ard(1) gives one per axis.  gdrf_set_period_count sets
 * count = 1 (one shared period, the default) or D; call it before reading gdrf_param_layout.  red_d then carries, at 8 + M*2D, 2D
 * embedded-coordinate sums and D sums of d / d log period_d (all-reduced with the rest), and the learnable-inducing-input sums at 8 are
 * (M, 2D) in the embedded coordinates.  The opt-in gdrf_set_hyper_backward(1) falls back to the f64 form. */
int gdrf_set_period_count(gdrf_ctx* ctx, int count);
int gdrf_periodic_layout(const gdrf_ctx* ctx, int64_t out[2]);
/* Product kernel (kernel_id GDRF_PRODUCT; D = the raw input axes): pyro.contrib.gp.kernels.Product of RBF and Periodic factors, each over
 * its own active axes, k = prod_f variance_f * k_f(x[axes_f], z[axes_f]).  It is evaluated as the RBF kernel at lengthscale 1 on the
 * concatenated embedded coordinates: (cos(t x_a), sin(t x_a)) / lengthscale for an axis a of a Periodic factor, x_a / lengthscale for one
 * of an RBF factor; at most 4 of them.  gdrf_set_product sets the table before the first step: nfactors (1-4) rows of 8 ints
 * {kind (GDRF_RBF or GDRF_PERIODIC), axis count, lengthscale count (1 or the axis count), period count (0 for RBF; 1 or the axis count),
 * axes[4] (each < D, the unused ones 0)}; a table with an axis >= D or more than 4 coordinates returns -1 (gdrf_last_error).  Until it is
 * called the table is one RBF factor over every axis.  The parameter vector then holds three segments (gdrf_product_layout -> {offset,
 * count} of the nfactors log-variances, of the log-lengthscales and of the log-periods, each in factor order; counts 0 in other contexts);
 * slots 0 and 1 are not read and receive a zero gradient, and every factor log-variance receives the gradient of the total log-variance.
 * red_d carries, at 8 + M*D', D' embedded-coordinate sums and one sum per Periodic axis, D' = the table's coordinate count; the
 * learnable-inducing-input sums at 8 are (M, D') in the embedded coordinates.  gdrf_set_hyper_backward(1) falls back to the f64 form. */
int gdrf_set_product(gdrf_ctx* ctx, int nfactors, const int* table);
int gdrf_product_layout(const gdrf_ctx* ctx, int64_t out[6]);
/* Trainable mean_function parameters (gdrf/models/abstract_gdrf.py:33-48: the mean_function is an attribute of a gp.Parameterized, so the
 * parameters of a torch.nn.Module mean - registered by pyro.module - or a PyroModule mean's own PyroParams land in the param store and
 * SVI.step trains them with the optimizer of every other parameter, gdrf/train_script.py:365-371,467).  The library never evaluates the
 * mean_function: the caller does, and chains the row adjoints through it.  With count > 0 the flat parameter vector (and grads, and the
 * two moment vectors of gdrf_adam) grows by a segment of `count` elements (gdrf_mean_param_layout -> {offset, count}; {offset of the
 * would-be segment, 0} when count = 0), and red_d by `count` doubles at total_d - count (total_d of gdrf_red_layout).  Per step the caller
 *   - after each gdrf_step_local / gdrf_step_local2 / phase 2 of gdrf_step_local_link reads the row adjoints of the mean values it passed:
 *     locbar (gdrf_ws_ptr 6) = d elbo / d (model-side mean), and in gdrf_step_local2 also gdrf_ws_ptr 18 = d elbo / d (guide-side mean),
 *     (K, n) arrays with leading dimension round_up(n_cap, 4), elbo = the unscaled sum of the per-row ELBO terms (the loss is
 *     -elbo / n_global).  Through a mean that enters both sides at the same inputs, locbar alone is the whole adjoint;
 *   - writes the vector-Jacobian product sum_kn adjoint[k][n] d mean[k][n] / d theta into that red_d segment (the step calls do not touch
 *     it), where it takes part in the particle combination and the collective like every other sum;
 *   - gdrf_step_finish then writes -segment / n_global into the segment of grads, and gdrf_adam updates it with the rest.
 * Call it before reading gdrf_param_layout / gdrf_red_layout and before the first gdrf_step_local2.  Default 0: the layouts are those of a
 * context that never called it. */
int gdrf_set_mean_params(gdrf_ctx* ctx, int64_t count);
int gdrf_mean_param_layout(const gdrf_ctx* ctx, int64_t out[2]);
void gdrf_ctx_destroy(gdrf_ctx* ctx);

/* Flat unconstrained-parameter vector (the PyroParam storage of gdrf/models/sparse_gdrf.py:96-122
 * and the pyro kernel's lengthscale/variance): out = {off_log_lengthscale, off_log_variance,
 * off_log_noise, off_u_loc (K*M), off_phi_unc (K*V), off_u_scale_tril_unc (K*M*M), total}.  Element 3 of the vector
 * (between log_noise and u_loc) is log(scale_mixture) of the RationalQuadratic kernel (pyro 1.8.0
 * kernels.isotropic.RationalQuadratic: variance * (1 + r2 / (2 scale_mixture))^(-scale_mixture)); the other kernels
 * ignore it and its gradient is 0. */
int gdrf_param_layout(const gdrf_ctx* ctx, int64_t out[7]);
/* Per-step all-reduce payload: out = {off_ubar, off_phibar, off_A, off_GT, total_T, total_d}; total_d = 8 + M*D (+ D in ARD contexts; 8 + M*2D + 3D in periodic ones; see gdrf_set_product for product ones)
 * (+ the count of gdrf_set_mean_params, the last doubles). */
int gdrf_red_layout(const gdrf_ctx* ctx, int64_t out[6]);
/* The step's ONE collective ("one ncclAllReduce(sum) per step over a flat buffer"): gdrf_payload_pack copies the
 * 8 + M*D doubles of red_d into the tail of red_T (total_T of gdrf_red_layout includes it) in red_T's element type - as they
 * are for double contexts, as four float pieces each (12 + 12 + 12 + 24 mantissa bits: sums over <= 8 ranks are exact while the
 * ranks' values of an entry lie within 2^9 of each other, as the loss sums do, and accurate to 2^-24 of the largest summand otherwise)
 * for float ones -; the caller all-reduces red_T alone and gdrf_payload_unpack restores red_d from the reduced tail. */
int gdrf_payload_pack(gdrf_ctx* ctx, void* red_T_dev, const double* red_d_dev, void* stream);
int gdrf_payload_unpack(gdrf_ctx* ctx, const void* red_T_dev, double* red_d_dev, void* stream);
/* The collective behind the C ABI, for hosts that do not go through torch.distributed: the caller registers ONE function that sums
 * `count` elements of `buf` (device memory; float when is_double = 0, double otherwise) in place over its ranks on `stream` - e.g. a
 * wrapper of ncclAllReduce(buf, buf, count, ncclFloat / ncclDouble, ncclSum, comm, stream) on the RCCL communicator it owns (`user`) - and
 * returns 0 on success.  gdrf_payload_allreduce then is the step's single collective: pack, that function on the whole flat payload
 * (total_T elements of gdrf_red_layout), unpack.  With no function registered it is a no-op (one rank).  gdrf_amd.Engine uses it when it is
 * constructed with allreduce_fn=...; its default remains torch.distributed.all_reduce between gdrf_payload_pack and gdrf_payload_unpack. */
typedef int (*gdrf_allreduce_fn)(void* buf_dev, int64_t count, int is_double, void* stream, void* user);
int gdrf_set_allreduce(gdrf_ctx* ctx, gdrf_allreduce_fn fn, void* user);
int gdrf_payload_allreduce(gdrf_ctx* ctx, void* red_T_dev, double* red_d_dev, void* stream);
/* Dirichlet concentration (K*V doubles, host): validate_dirichlet_param, gdrf/models/utils.py:6-24. */
int gdrf_set_dirichlet(gdrf_ctx* ctx, const double* alpha_host);

/* K_nm = k(X, Z), row-major (n, ldo): pyro RBF/Matern52.forward(X, Z) as used inside
 * gp.util.conditional (gdrf/models/sparse_gdrf.py:334-344).  The HBM-roofline kernel. */
int gdrf_knm(gdrf_ctx* ctx, const void* X_dev, int64_t n, const void* Z_dev, const void* params_dev,
             void* out_dev, int64_t ldo, void* stream);

/* eps[k][n] ~ N(0,1), Philox keyed by (seed; global row n_offset+n, k, step): the rsample of the
 * guide's mu site (gdrf/models/sparse_gdrf.py:403-405). */
int gdrf_fill_eps(gdrf_ctx* ctx, uint64_t seed, uint32_t step, int64_t n_offset, int64_t n, void* eps_dev, void* stream);

/* sum_n [lgamma(sum_v w+1) - sum_v lgamma(w+1)]: the data-only part of Multinomial.log_prob
 * (gdrf/models/sparse_gdrf.py:363-372).  Synchronises the stream. */
int gdrf_ll_const(gdrf_ctx* ctx, const int32_t* ws_dev, int64_t n, double* out_host, void* stream);
/* The same constant written to a device double (e.g. red_d + 7, where gdrf_step_finish reads it when its ll_const argument
 * is NaN), without synchronising: a mini-batch step (gdrf/train_script.py:461-465) then needs no host round trip for it. */
int gdrf_ll_const_dev(gdrf_ctx* ctx, const int32_t* ws_dev, int64_t n, double* out_dev, void* stream);

/* jittercholesky's retry loop (gdrf/models/utils.py:27-40) on kernel(inducing_points)
 * (gdrf/models/sparse_gdrf.py:327-328,382-383): nlev (<= 8) attempts with the cumulative jitters
 * jitters_host[0..nlev) factorised concurrently in ONE launch, in the array precision -- the precision in
 * which the reference's torch.linalg.cholesky decides whether more jitter is needed.  failed_host[l] != 0 when
 * attempt l hit a non-positive pivot; the caller takes the first success (same outcome as trying them in order).
 * Synchronises the stream.  Uses its own workspace and flag slots: it may run on a second stream beside
 * gdrf_factorize()/gdrf_step_local() of the same parameters (gdrf_amd.Engine overlaps it that way). */
int gdrf_probe(gdrf_ctx* ctx, const void* Z_dev, const void* params_dev, const double* jitters_host, int nlev,
               int* failed_host, void* stream);
/* The same in two calls: the launch alone (asynchronous, so that the caller can enqueue the step it speculates on beside it) and
 * the read of the flags of the last launch (waits for `stream`). */
int gdrf_probe_launch(gdrf_ctx* ctx, const void* Z_dev, const void* params_dev, const double* jitters_host, int nlev, void* stream);
int gdrf_probe_read(gdrf_ctx* ctx, int nlev, int* failed_host, void* stream);

/* K_uu + jitter_total*I, its Cholesky factor L and L^{-1} in the solve precision, kept in the context for
 * the calls below. */
int gdrf_factorize(gdrf_ctx* ctx, const void* Z_dev, const void* params_dev, double jitter_total, void* stream);
/* The same with a mode: 0 = gdrf_factorize.  1 = factorise AHEAD of the step that will use the result (call it right behind the optimizer
 * update: the chain then runs while the host reads the loss and enqueues the next step) and keep a copy of its inputs (the kernel
 * hyper-parameters and Z).  2 = the step's own call: if a mode-1 factorisation with this jitter is waiting, its inputs are only compared
 * with the current ones on the device - gdrf_chol_failed then reports a mismatch like a failure, and the caller redoes the step with
 * mode 0; otherwise as mode 0. */
int gdrf_factorize_mode(gdrf_ctx* ctx, const void* Z_dev, const void* params_dev, double jitter_total, void* stream, int mode);

/* Forward + backward over this rank's n_local observations: everything of one
 * SVI.step(xs, ws) (gdrf/train_script.py:467 -> sparse_gdrf.py:323-409) that is a sum over
 * observations.  X (n,D), ws (n,V) int32, eps (K,n).  Writes the partial sums to red_T
 * (dtype elements) and red_d (doubles); the caller all-reduces both over ranks.  Needs gdrf_factorize() on the same params. */
int gdrf_step_local(gdrf_ctx* ctx, const void* X_dev, const int32_t* ws_dev, const void* eps_dev, int64_t n_local,
                    const void* Z_dev, const void* params_dev, void* red_T_dev, double* red_d_dev, void* stream);

/* One step around a caller-supplied link function (the reference's `link_function` constructor argument, gdrf/models/abstract_gdrf.py:34-50,
 * used as `self._link_function(mu).transpose(-2, -1)` in gdrf/models/sparse_gdrf.py:361), which the caller evaluates itself between three calls:
 *   phase 0: everything of gdrf_step_local up to mu = f_loc + f_var eps (+ mean) -> workspace 14 (K, ldk);
 *   phase 1: ext = theta = link(mu), (K, ext_ld) -> d loglik / d theta in workspace 6, the word-topic gradient and the log-likelihood sum;
 *   phase 2: ext = mubar = J_link^T thetabar, (K, ext_ld) -> the Normal sites, the row-local backward and the rest of gdrf_step_local.
 * theta need not sum to one over the topics (Multinomial normalises p = theta^T Phi, as torch does).  Not a fused path. */
int gdrf_step_local_link(gdrf_ctx* ctx, const void* xs_dev, const int32_t* ws_dev, const void* eps_dev, int64_t n_local, const void* Z_dev,
                         const void* params_dev, void* red_T_dev, double* red_d_dev, void* stream, int phase, const void* ext_dev, int64_t ext_ld);

/* The same with the guide and the model evaluated at DIFFERENT inputs: the reference's guide scales its inputs twice
 * (gdrf/models/sparse_gdrf.py:376 @scale_decorator and :380 `xs = self.scale(xs)`), its model once (:324), so for a world other
 * than the unit cube the guide's gp.util.conditional sees X_guide = scale(scale(xs)) and the model's X_model = scale(xs).
 * mu is drawn from the guide-side predictive, log q uses it, log p(mu) the model-side one; both are differentiated.  About 2.5 x
 * the work of gdrf_step_local (two forwards and backwards, the guide's forward twice); the mean_function values of the guide side
 * come from gdrf_set_mean_guide, the model side's from gdrf_set_mean. */
int gdrf_step_local2(gdrf_ctx* ctx, const void* X_model_dev, const void* X_guide_dev, const int32_t* ws_dev, const void* eps_dev,
                     int64_t n_local, const void* Z_dev, const void* params_dev, void* red_T_dev, double* red_d_dev, void* stream);
int gdrf_set_mean_guide(gdrf_ctx* ctx, const void* mean, int64_t stride_k, int64_t stride_n);

/* Replicated epilogue: Cholesky / kernel hyper-parameter backward, constraint Jacobians, Dirichlet
 * term, loss.  grads (same layout as params) = d loss / d unconstrained.  out_d (8 doubles) =
 * {loss, cholesky_failed, site_sum, loglik_sum, log_prior_phi, ...}.  ll_const = the data-only constant of the
 * Multinomial log-likelihood (gdrf_ll_const, summed over ranks); pass NaN to take it from red_d[7] on the device. */
int gdrf_step_finish(gdrf_ctx* ctx, const void* Z_dev, const void* params_dev, const void* red_T_dev,
                     const double* red_d_dev, double n_global, double ll_const, void* grads_dev, double* out_d_dev,
                     void* stream);

/* pyro.optim.{Adam,AdamW,ClippedAdam} on every unconstrained tensor at once (train_script.py:73-87);
 * skipped on the device when the step's Cholesky failed. t = 1-based step count. */
int gdrf_adam(gdrf_ctx* ctx, int mode, void* params_dev, const void* grads_dev, void* m_dev, void* v_dev, int64_t t,
              double lr, double beta1, double beta2, double eps, double weight_decay, double clip, void* stream);

/* The pyro.optim rules of train_script.py:73-87 per named parameter tensor, with pyro's clip_args and per-parameter optim_args
 * (PyroOptim keeps one torch optimizer per tensor).  A segment is one parameter tensor: elements [offset, offset + length) of the flat
 * vector; elements outside every segment are not touched.  The caller computes each segment's scalars a[] in double for every step:
 *   GDRF_ADAM, GDRF_ADAMW, GDRF_CLIPPED_ADAM  {lr, beta1, beta2, eps, weight_decay, clip, 1 - beta1^t, 1 - beta2^t}  (gdrf_adam's arithmetic)
 *   GDRF_ADAMAX            {lr / (1 - beta1^t), beta1, beta2, eps, weight_decay}           s1 exp_avg, s2 exp_inf
 *   GDRF_RMSPROP           {lr, alpha, eps, weight_decay, momentum}                        s2 square_avg, s1 momentum_buffer (flag MOMENTUM),
 *                          grad_avg (flag CENTERED) in s3 when both flags are set, else in s1
 *   GDRF_ADAGRAD           {lr / (1 + (t - 1) lr_decay), eps, weight_decay}                s2 sum
 *   GDRF_ADADELTA          {lr, rho, eps, weight_decay}                                    s2 square_avg, s1 acc_delta
 *   GDRF_ASGD              {eta, mu, lambd, weight_decay} (eta, mu: the values stored before this step)   s1 ax
 *   GDRF_RPROP             {eta_minus, eta_plus, step_size_min, step_size_max}             s1 prev, s2 step_size
 *   GDRF_ADAGRAD_RMSPROP   {eta t^(-1/2 + delta), t (the mixing rate), 1 at the first step else 0}   s2 sum
 * Flag CLIP_NORM scales the segment's gradient by clip_norm / (|g|_2 + 1e-6) when that is below 1 (torch clip_grad_norm_), then
 * CLIP_VALUE clamps it to +-clip_value (clip_grad_value_); the gradient buffer itself is not written.  Up to 24 segments take one launch
 * (two with CLIP_NORM: a sum of squares per 8192 elements, summed in a fixed order - bitwise reproducible); more take one such pair per 24.
 * s3 may be NULL unless an RMSprop segment sets both MOMENTUM and CENTERED.  Skipped on the device when the step's Cholesky failed. */
enum { GDRF_ADAMAX = 3, GDRF_RMSPROP = 4, GDRF_ADAGRAD = 5, GDRF_ADADELTA = 6, GDRF_ASGD = 7, GDRF_RPROP = 8, GDRF_ADAGRAD_RMSPROP = 9 };
enum { GDRF_OPT_CLIP_NORM = 1, GDRF_OPT_CLIP_VALUE = 2, GDRF_OPT_MOMENTUM = 4, GDRF_OPT_CENTERED = 8 };
typedef struct gdrf_opt_seg {
  int64_t offset, length;
  double clip_norm, clip_value;
  int32_t flags, reserved;
  double a[8];
} gdrf_opt_seg;
int gdrf_optim_step(gdrf_ctx* ctx, int rule, const gdrf_opt_seg* segs_host, int nseg, void* params_dev, const void* grads_dev,
                    void* s1_dev, void* s2_dev, void* s3_dev, void* stream);

/* Predictive mean path: log_topic_probs / topic_probs / word_probs / perplexity
 * (gdrf/models/sparse_gdrf.py:161-186, abstract_gdrf.py:113-139).  mode 0: out (K,n) ;
 * 1: out (n,K) ; 2: out (n,V) ; 3: out_d_dev[0..1] = {sum w log p, sum w}.  Modes 0-3 never form the variance (the reference
 * computes and discards it, quirk Q4): K_nm is generated tile by tile as the A operand of the solve-precision matrix instruction and
 * multiplied with L^-T u (csrc/predict.h); any n.
 * mode 4: out (2,K,n) = {f_loc, f_var} of gp.util.conditional(full_cov=False) as SparseGDRF.forward(Xnew) returns them
 * (gdrf/models/sparse_gdrf.py:277-319; the mean_function is added by the caller): the step's forward (K_nm, W = K_nm L^-T,
 * loc = W U^T, tt = |S_k^T w|^2) plus one pass for var = clamp(variance - |w|^2, 0) + tt; n <= n_cap.  Needs gdrf_factorize(). */
int gdrf_predict(gdrf_ctx* ctx, const void* X_dev, int64_t n, const void* Z_dev, const void* params_dev,
                 const int32_t* ws_dev, int mode, void* out_dev, double* out_d_dev, void* stream);

/* Monte-Carlo integration over the guide's posterior q(mu) at new inputs (csrc/predict_mc.h): the quantities of gdrf_predict are plug-ins
 * softmax(f_loc); these integrate over mu ~ Normal(f_loc, f_var) as the guide writes it (f_var as the SCALE, gdrf/models/sparse_gdrf.py:403-405):
 *   mu[s][k][n] = f_loc[k][n] + mean[k][n] + f_var[k][n] eps[s][k][n],  theta[s][n][:] = softmax_k(mu[s][:][n]),  p[s][n][:] = theta[s][n][:] Phi,
 * (f_loc, f_var) as mode 4 of gdrf_predict gives them (X: the inputs scaled ONCE), mean = the values set with gdrf_set_mean (NULL: zero).
 * eps_dev: an (S, K, n) array of the context's element type, or NULL for Philox4x32-10 draws keyed by `seed` with counter (row_offset + n, k, s):
 * sample s of row n is the number gdrf_fill_eps(seed, step = s, n_offset = row_offset) writes, so cutting the rows into several calls, each
 * with its row_offset, changes no draw.  S = num_samples >= 1.
 *   GDRF_MC_THETA    out (S, n, K): the theta samples
 *   GDRF_MC_MOMENTS  out (2, n, K): mean and variance (divisor S) of theta over the samples; no sample is stored
 *   GDRF_MC_SCORE    out_d_dev[0..1] = {sum_n l_n, sum w}, l_n = logsumexp_s(sum_v w[n][v] log p[s][n][v]) - log S (the Multinomial
 *                    coefficient left out, as gdrf_predict mode 3 leaves it out); ws_dev (n, V) dense int32 counts (not with a bound CSR
 *                    matrix); Phi, the counts and theta of a workgroup's rows live in LDS, so K x V is bounded as for the LDS row forms
 *                    ("too large" otherwise); p is never stored; deterministic sums (per-workgroup partials, no atomics)
 *   GDRF_MC_MU       out (S, K, n): the mu samples, for a link function the caller evaluates
 * n <= n_cap.  Runs the step's forward (as mode 4), so it overwrites the same workspaces; every step recomputes them.  Everything but the
 * two sums of GDRF_MC_SCORE is bit-identical however the rows are batched.  Needs gdrf_factorize(). */
enum { GDRF_MC_THETA = 0, GDRF_MC_MOMENTS = 1, GDRF_MC_SCORE = 2, GDRF_MC_MU = 3 };
int gdrf_predict_mc(gdrf_ctx* ctx, const void* X_dev, int64_t n, const void* Z_dev, const void* params_dev, const int32_t* ws_dev, int mode,
                    int num_samples, uint64_t seed, int64_t row_offset, const void* eps_dev, void* out_dev, double* out_d_dev, void* stream);

/* Per-location entropy and information-gain maps (csrc/predict_info.h): how uncertain the field is at the n new inputs and how much of
 * that comes from the latent field not being known there - the part that shrinks when the location is sampled.  Over the S = num_samples
 * draws gdrf_predict_mc makes (the same mu, theta_s, p_s = theta_s Phi, the same eps_dev / seed / row_offset, bit for bit), with
 * h(q) = -sum_i q_i log q_i (0 log 0 = 0) and theta_bar = (1/S) sum_s theta_s, out_dev (6, n) doubles holds the rows
 *   0  topic_entropy           h(theta_bar)                     3  word_entropy           h(theta_bar Phi)
 *   1  topic_expected_entropy  (1/S) sum_s h(theta_s)           4  word_expected_entropy  (1/S) sum_s h(p_s)
 *   2  topic_information       row 0 - row 1                    5  word_information       row 3 - row 4
 * Rows 2 and 5 are the Monte-Carlo estimates of the mutual information between the topic (the word) of one token observed at x and the
 * latent field there (BALD): Jensen-Shannon divergences of the sampled distributions, 0 <= row 5 <= row 2 <= log min(K, S) up to
 * rounding, returned as computed (not clamped).  theta_bar is bit for bit the mean GDRF_MC_MOMENTS returns.  p and p log p are formed in
 * the array precision, every sum over topics, words and samples in double.  No sample is stored; Phi passes through LDS in chunks of
 * GDRF_INFO_V_CHUNK words, so any V is served, and every K the context supports; 1 <= num_samples <= 65535.
 * n <= n_cap.  Runs the step's forward (as mode 4 of gdrf_predict), so it overwrites the same workspaces; every step recomputes them.
 * Every output is bit-identical however the rows are batched (no atomics, no sum over rows).  Needs gdrf_factorize(). */
#define GDRF_INFO_V_CHUNK 128
int gdrf_predict_info(gdrf_ctx* ctx, const void* X_dev, int64_t n, const void* Z_dev, const void* params_dev, int num_samples, uint64_t seed,
                      int64_t row_offset, const void* eps_dev, double* out_dev, void* stream);

/* Per-row Monte-Carlo log predictive densities (csrc/predict_score.h): how well the fitted field explains each of n observed rows, under
 * its own posterior.  Over the S = num_samples draws gdrf_predict_mc makes (the same mu, theta_s, p_s = theta_s Phi, the same eps_dev /
 * seed / row_offset, bit for bit) and with the row's counts w, a_s = sum_{v: w_v != 0} w_v log p_s[v], out_dev (5, n) doubles holds the rows
 *   0  lpd           logsumexp_s(a_s) - log S                      3  total     sum_v w_v
 *   1  mean_log_lik  (1/S) sum_s a_s                               4  log_coef  lgamma(total + 1) - sum_v lgamma(w_v + 1)
 *   2  var_log_lik   sum_s (a_s - row 1)^2 / (S - 1), 0 for S = 1
 * Row 0 is the l_n whose sum over the rows GDRF_MC_SCORE returns; rows 0 and 1 leave the Multinomial coefficient out, as it does, and
 * row 4 is that coefficient's log.  sum_n (row 0 - row 2) is the WAIC estimate of the expected log pointwise predictive density.
 * The counts are either dense - ws_dev (n, V) int32, crow_dev NULL - or CSR - ws_dev NULL, crow_dev (n + 1) int64 row pointers from 0,
 * col_dev / val_dev int32; only the stored entries are visited, a stored zero is an absent entry, a row without entries gives five
 * zeros.  A CSR matrix bound with gdrf_bind_counts_csr plays no part.  p and its log are formed in the array precision with k ascending,
 * every sum over words and samples in double (rows 1 and 2 from the sums of a_s - a_0 and of its square: equal draws give a variance of
 * exactly 0).  No sample is stored.  Dense: Phi passes through LDS in chunks of GDRF_SCORE_V_CHUNK words and the samples are taken in
 * tiles of GDRF_SCORE_S_TILE, so any V is served; CSR: Phi is read from global memory.  Every K the context supports;
 * 1 <= num_samples <= 65535.  n <= n_cap.  Runs the step's forward (as mode 4 of gdrf_predict), so it overwrites the same workspaces;
 * every step recomputes them.  Every output is bit-identical however the rows are batched (no atomics, no sum over rows).  Needs
 * gdrf_factorize(). */
#define GDRF_SCORE_V_CHUNK 128
#define GDRF_SCORE_S_TILE 64
int gdrf_predict_score(gdrf_ctx* ctx, const void* X_dev, int64_t n, const void* Z_dev, const void* params_dev, const int32_t* ws_dev,
                       const int64_t* crow_dev, const int32_t* col_dev, const int32_t* val_dev, int num_samples, uint64_t seed,
                       int64_t row_offset, const void* eps_dev, double* out_dev, void* stream);

/* Credible-interval, exceedance and dominant-topic maps (csrc/predict_quant.h): uncertainty of the field at the n new inputs in a form
 * that can be shown.  Over the S = num_samples draws gdrf_predict_mc makes (the same mu[s][k] = f_loc[k][n] + mean[k][n] +
 * f_var[k][n] eps[s][k][n] with f_var as the scale, theta_s = softmax(mu_s), the same eps_dev / seed / row_offset, bit for bit) a
 * component c of a row is a topic, x_s = theta_s[c] (words_dev NULL, nwords 0: C = K), or a chosen word v = words_dev[c],
 * x_s = sum_k theta_s[k] Phi[k][v] formed in the array precision with k ascending (C = nwords; the list is int32 on the device, may
 * repeat and be in any order).  By mode:
 *   GDRF_QUANT_QUANTILE  out_dev (nlevels, n, C): the type-7 ("linear") sample quantile of x_0 .. x_{S-1} at the levels q =
 *                        levels_host[i] in [0, 1]: with h = q (S - 1), lo = floor(h), hi = min(lo + 1, S - 1), frac = h - lo (formed here,
 *                        on the host, in double) and x_(r) the r-th order statistic, (double)x_(lo) + frac ((double)x_(hi) - (double)x_(lo)).
 *                        1 <= num_samples <= GDRF_QUANT_MAX_SAMPLES.
 *   GDRF_QUANT_EXCEED    out_dev (nlevels, n, C): #{s : x_s > tau} / S for the finite thresholds tau = levels_host[i], strict, the integer
 *                        count divided once in double.  1 <= num_samples <= 65535.
 *   GDRF_QUANT_DOMINANT  out_dev (n, K): #{s : argmax_k theta_s = k} / S, equal values to the lower topic; topics only (nwords 0) and
 *                        nlevels 0.  1 <= num_samples <= 65535.
 * 1 <= nlevels <= GDRF_QUANT_MAX_LEVELS for the first two modes.  No V and no K the context supports is refused.  The entries of
 * words_dev must lie in [0, V): the library does not read the list on the host, the Python layer (engine.check_quant_args) validates it
 * before the call.  n <= n_cap.  Runs the step's forward (as mode 4 of gdrf_predict), so it overwrites the same workspaces; every step
 * recomputes them.  Every output is bit-identical however the rows are batched (no atomics, nothing shared between rows).  Needs
 * gdrf_factorize().  gdrf_quant_last_plan: (rows per workgroup pass RP, components per pass CP, dynamic LDS bytes) of the last call's
 * launch - the quantile mode's plan is csrc/forms.h::quant_plan. */
#define GDRF_QUANT_MAX_SAMPLES 1024
#define GDRF_QUANT_MAX_LEVELS 16
enum { GDRF_QUANT_QUANTILE = 0, GDRF_QUANT_EXCEED = 1, GDRF_QUANT_DOMINANT = 2 };
int gdrf_predict_quant(gdrf_ctx* ctx, const void* X_dev, int64_t n, const void* Z_dev, const void* params_dev, int mode, int num_samples,
                       uint64_t seed, int64_t row_offset, const void* eps_dev, const double* levels_host, int nlevels,
                       const int32_t* words_dev, int nwords, double* out_dev, void* stream);
int gdrf_quant_last_plan(const gdrf_ctx* ctx, int out[3]);

/* Pareto-smoothed importance-sampling leave-one-out (csrc/predict_loo.h has the definition, step by step): for each of n observed rows, from
 * the S = num_samples log likelihoods a_s that gdrf_predict_score forms (the same draws, eps_dev / seed / row_offset, the same counts in
 * either layout, bit for bit) out_dev (6, n) doubles holds the rows
 *   0  elpd_loo  the row's held-out log predictive density, logsumexp_s(a_s + lw_s) with the smoothed, truncated, normalised log
 *                weights lw of the importance ratios 1 / p(w_n | theta_s)
 *   1  pareto_k  the shape of the generalised Pareto distribution fitted to the M = tail_len largest ratios (Zhang & Stephens 2009 with
 *                the weakly informative prior of Vehtari et al.); NaN where nothing is fitted: the tail's lower quartile is not above
 *                the cutoff (constant a_s - an empty row, K = 1, V = 1, eps = 0 - or an underflowing tail)
 *   2  ess       1 / sum_s exp(2 lw_s), the effective sample size of the weights
 *   3  lpd  4  total  5  log_coef    rows 0, 3 and 4 of gdrf_predict_score, bit for bit
 * Rows 0 and 3 leave the Multinomial coefficient out.  Everything from the a_s on is in double.  tail_len must be
 * ceil(min(S / 5, 3 sqrt(S))) formed in double (the Python layer's engine.loo_tail_len); GDRF_LOO_MIN_SAMPLES <= num_samples <=
 * GDRF_LOO_MAX_SAMPLES: all S values of a row are kept in LDS and ordered there.  a_out_dev, optional, (S, n) doubles, receives the a_s.
 * Any V, dense or CSR, every K the context supports; n <= n_cap.  Runs the step's forward (as mode 4 of gdrf_predict), so it overwrites
 * the same workspaces; every step recomputes them.  Every output is bit-identical however the rows are batched (no atomics, nothing
 * shared between rows).  Needs gdrf_factorize().
 * gdrf_psis_rows: the same from a caller's own log_lik_dev (S, n) doubles - out_dev (3, n): elpd_loo, pareto_k, ess - for models whose
 * a_s the library cannot form; no model quantity is read, no factorisation needed, any n >= 1.
 * gdrf_loo_last_plan: (rows per workgroup pass RP, dynamic LDS bytes) of the last launch of either - csrc/forms.h::loo_plan. */
#define GDRF_LOO_MAX_SAMPLES 1024
#define GDRF_LOO_MIN_SAMPLES 25
int gdrf_predict_loo(gdrf_ctx* ctx, const void* X_dev, int64_t n, const void* Z_dev, const void* params_dev, const int32_t* ws_dev,
                     const int64_t* crow_dev, const int32_t* col_dev, const int32_t* val_dev, int num_samples, int tail_len, uint64_t seed,
                     int64_t row_offset, const void* eps_dev, double* out_dev, double* a_out_dev, void* stream);
int gdrf_psis_rows(gdrf_ctx* ctx, const double* log_lik_dev, int num_samples, int tail_len, int64_t n, double* out_dev, void* stream);
int gdrf_loo_last_plan(const gdrf_ctx* ctx, int out[2]);

/* Fold-in (csrc/foldin.h): the topic proportions of OBSERVED rows from their own counts, with the GP as the prior.  For row n, with
 *   m_k = f_loc[k][n] + mean[k][n],  s_k = f_var[k][n] + noise   ((f_loc, f_var) as mode 4 of gdrf_predict gives them; s_k is the scale of the
 *   model's mu site, Normal(f_loc, f_var + noise), gdrf/models/sparse_gdrf.py:354-357),  R = sum_v w_v,  theta = softmax(mu),  p = theta Phi:
 *   J(mu) = sum_{v: w_v > 0} w_v log p_v - 1/2 sum_k ((mu_k - m_k) / s_k)^2
 * the result mu_hat is a local maximiser of J reached from mu = m by at most num_iters monotone EM / Newton iterations (J never decreases;
 * csrc/foldin.h has the iteration); a row stops early once |g|_inf / max(1, R) <= tol, g the gradient of J.  theta_hat = softmax(mu_hat).
 * The counts are either dense - ws_dev (n, V) int32, crow_dev NULL; Phi, the counts and theta of a workgroup's rows live in LDS, so K x V is
 * bounded as for the LDS row forms ("too large" otherwise) - or CSR - ws_dev NULL, crow_dev (n + 1) int64 row pointers from 0, col_dev /
 * val_dev int32; only the stored entries are visited, a stored zero is an absent entry, no limit on V.  A CSR matrix bound with
 * gdrf_bind_counts_csr plays no part.
 *   GDRF_FI_THETA   out (n, K): theta_hat
 *   GDRF_FI_MU      out (K, n): mu_hat
 *   GDRF_FI_COUNTS  out (n, K): the expected topic counts r_k = theta_k sum_v w_v Phi_kv / p_v at theta_hat (a row sums to R)
 *   GDRF_FI_SCORE   out_d_dev[0..1] = {sum_n sum_v w2 log p_hat, sum w2} for a second count matrix (ws2_dev or crow2_dev / col2_dev /
 *                   val2_dev) in the layout of the first; all four NULL: the fitted counts themselves.  Deterministic sums, no atomics.
 * Every mode also writes diag_dev (3, n) doubles: J at the result, |g|_inf / max(1, R) there, the iterations used.
 * n <= n_cap, num_iters >= 0, tol finite and >= 0.  Runs the step's forward (as mode 4 of gdrf_predict), so it overwrites the same
 * workspaces; every step recomputes them.  Everything but the two sums of GDRF_FI_SCORE is bit-identical however the rows are batched.
 * Needs gdrf_factorize(). */
enum { GDRF_FI_THETA = 0, GDRF_FI_MU = 1, GDRF_FI_COUNTS = 2, GDRF_FI_SCORE = 3 };
int gdrf_fold_in(gdrf_ctx* ctx, const void* X_dev, int64_t n, const void* Z_dev, const void* params_dev, const int32_t* ws_dev,
                 const int64_t* crow_dev, const int32_t* col_dev, const int32_t* val_dev, const int32_t* ws2_dev, const int64_t* crow2_dev,
                 const int32_t* col2_dev, const int32_t* val2_dev, int mode, int num_iters, double tol, void* out_dev, double* diag_dev,
                 double* out_d_dev, void* stream);

/* Posterior-predictive count samples (csrc/sample_counts.h): replicated counts w_rep drawn from Multinomial(T_n, theta_s Phi), what
 * pyro.infer.Predictive(model, guide=guide, num_samples=S) samples at the model's `w` site.  theta_dev: (S, n, K) samples of the topic
 * proportions in the context's element type (as GDRF_MC_THETA returns them); Phi = softmax of the phi block of params_dev, as the
 * predictive calls form it; totals_dev: (n) int32 row totals T_n, tmax their maximum (a row's total is read as min(max(T_n, 0), tmax)).
 *   p[s][n][v] = sum_k theta[s][n][k] Phi[k][v]                        (array precision)
 *   c[s][n][v] = p[s][n][0] + ... + p[s][n][v]                         (inclusive prefix sum, in double)
 *   word(s,n,t) = the smallest v with u[s][n][t] c[s][n][V-1] < c[s][n][v]  (in double),  t = 0 .. T_n - 1
 *   w_rep[s][n][v] = #{ t : word(s,n,t) = v }
 * u_dev: injected uniforms (S, n, tmax) double in [0, 1), or NULL for Philox4x32-10 draws keyed by `seed` with counter
 * (row_offset + n, 2^31 | t / 4, s): word t % 4 of the block gives u = (word + 0.5) / 2^32.  The 2^31 keeps the token draws of a seed apart
 * from the normals gdrf_fill_eps / gdrf_predict_mc draw under it (their third counter word is a topic index), and cutting the rows into
 * several calls, each with its row_offset, changes no draw.
 *   GDRF_SC_COUNTS    out_dev (S, n, V) int32: w_rep
 *   GDRF_SC_STATS     the statistics of a posterior predictive check against the observed dense counts ws_dev (n, V) int32, from the draws
 *                     GDRF_SC_COUNTS makes (bit for bit) without storing them: with q = p / c[V-1], dev_dev (2, S) doubles =
 *                     {dev_rep[s] = 2 sum_n sum_{v: w_rep > 0} w_rep log(w_rep / (T_n q_v)); dev_obs[s] = the same for ws[n] with its own row
 *                     sum as T_n}, and zeros_dev (S, V) int64 = #{ n : w_rep[s][n][v] = 0 }.  The sums: per-workgroup partials added in a
 *                     fixed order, no float atomics; the integers are exact however the rows are batched.
 *   GDRF_SC_UNIFORMS  u_dev (S, n, tmax) is WRITTEN: the uniforms the other modes draw from `seed` and `row_offset`; nothing else is read
 * 1 <= num_samples <= 65535; any n >= 1 (no workspace is per row); V <= GDRF_SC_MAX_V (error otherwise); every K the context supports.
 * Overwrites the context's Phi workspace and partial-sum scratch, as every predictive call does.  Needs no factorisation. */
enum { GDRF_SC_COUNTS = 0, GDRF_SC_STATS = 1, GDRF_SC_UNIFORMS = 2 };
#define GDRF_SC_MAX_V 4096
int gdrf_sample_counts(gdrf_ctx* ctx, const void* theta_dev, int64_t n, const void* params_dev, const int32_t* totals_dev, int tmax,
                       const int32_t* ws_dev, int mode, int num_samples, uint64_t seed, int64_t row_offset, double* u_dev, int32_t* out_dev,
                       double* dev_dev, int64_t* zeros_dev, void* stream);

/* The joint posterior q(f_k(X*)) = N(loc_k, C_k) at n new inputs (csrc/predict_cov.h; gp.util.conditional(..., full_cov=True) as
 * SparseGDRF.forward(Xnew, full_cov=True) calls it, gdrf/models/sparse_gdrf.py:277-319).  With W = K_*m L^-T (n x M, the step's forward):
 *   R   = K_** - W W^T                       (n x n, the same for every topic; nothing added to its diagonal, no clamp)
 *   C_k = R + (W S_k)(W S_k)^T               (whiten = 0: S_k, u_k stand for L^-1 S_k, L^-1 u_k, as in mode 4 of gdrf_predict)
 * K_** is the context's kernel between the rows (Periodic and Product contexts: on the embedded coordinates).  Apart from mode 4's
 * clamp(variance - |w|^2, 0), the diagonal of C_k is mode 4's f_var; loc_k is mode 4's f_loc (this call does not return it).
 *   GDRF_COV_FULL   out (K, n, n)
 *   GDRF_COV_RESID  out (n, n) = R
 * in the context's element type, equal to their transposes to the bit (the tiles on and below the diagonal are computed and mirrored).
 * Everything n x n is formed in the solve precision (W is recomputed in it from the step's solve-precision K_nm and L^-1: K_** - W W^T
 * cancels almost completely near the inducing points) on the solve-precision matrix instruction, and rounded on output.  X: the inputs
 * scaled ONCE; n <= n_cap; needs gdrf_factorize().  Runs the step's forward (as mode 4), so it overwrites the same workspaces, which every
 * step recomputes; its own buffers (n x M, n x n and, for GDRF_COV_FULL, K x n x M solve-precision elements) are allocated on first use
 * and grow with n.  No atomics: bit-identical from call to call. */
enum { GDRF_COV_FULL = 0, GDRF_COV_RESID = 1 };
int gdrf_predict_cov(gdrf_ctx* ctx, const void* X_dev, int64_t n, const void* Z_dev, const void* params_dev, int which, void* out_dev, void* stream);
/* Joint (spatially coherent) samples of the latent field at n new inputs, in the pathwise form, which needs one n x n factorisation
 * instead of K:
 *   f[s][k][:] = W (u_k + S_k xi[s][k][:]) + G zeta[s][k][:] + mean[k][:],    G G^T = R + jitter_total I,
 * out (S, K, n), S = num_samples; xi (S, K, M) and zeta (S, K, n) standard normal; mean = the values set with gdrf_set_mean (NULL: zero).
 * The covariance of f[.][k][:] is C_k + jitter_total I (gdrf_predict_cov).  R + jitter_total I is factorised in the solve precision by the
 * one-workgroup Cholesky of the jitter probe, on a buffer of this call's own; a non-positive pivot sets a flag (and is replaced by 1, so
 * the output stays finite but is not a sample): read it with gdrf_joint_failed and call again with the next cumulative jitter of the
 * schedule, as for gdrf_factorize / gdrf_chol_failed.
 * xi_dev, zeta_dev: arrays of the context's element type, or NULL for Philox4x32-10 draws keyed by `seed`, rounded to the element type,
 * with the counter words (index, topic, sample) of gdrf_fill_eps on two streams of their own:
 *   xi[s][k][m]   = the number gdrf_fill_eps(seed, step = s, n_offset = 2^61) writes at [k][m],
 *   zeta[s][k][i] = the number gdrf_fill_eps(seed, step = s, n_offset = 2^62) writes at [k][i],  i = the row's position within THIS call.
 * No xi draw is a zeta draw, and neither is a draw of gdrf_predict_mc or of a training step's eps for rows below 2^61.  A joint draw
 * cannot be cut into row pieces: there is no row_offset, and n <= n_cap (at most 65503 rows and 65535 (sample, topic) pairs).
 * Needs gdrf_factorize(); workspaces as for gdrf_predict_cov.  No atomics: bit-identical from call to call. */
int gdrf_sample_joint(gdrf_ctx* ctx, const void* X_dev, int64_t n, const void* Z_dev, const void* params_dev, int num_samples, uint64_t seed,
                      const void* xi_dev, const void* zeta_dev, double jitter_total, void* out_dev, void* stream);
/* The same samples on another jitter: only R + jitter_total I, its factorisation and the two sample products are redone, from the W, R,
 * u_k + S_k xi and zeta that the gdrf_sample_joint call directly in front of it left in the context (same n and num_samples, same stream;
 * the same mean still set).  Anything else is an error: gdrf_predict_cov or another gdrf_sample_joint in between rewrites those buffers.
 * The output is bit for bit what gdrf_sample_joint with this jitter_total would have written. */
int gdrf_sample_joint_retry(gdrf_ctx* ctx, int64_t n, int num_samples, double jitter_total, void* out_dev, void* stream);
/* Did the factorisation of the last gdrf_sample_joint() / gdrf_sample_joint_retry() hit a non-positive pivot?  Synchronises the stream. */
int gdrf_joint_failed(gdrf_ctx* ctx, int* failed_host, void* stream);

/* The greedy choice of a non-redundant batch of `count` of the n rows X (csrc/select_batch.h).  With C_k the joint posterior covariances of
 * gdrf_predict_cov and s2 = noise > 0 an observation-noise variance, the information in noisy observations f_k(x_a) + N(0, s2) at the rows A is
 *   I(A) = 1/2 sum_k log det(I + C_k[A, A] / s2)
 * (monotone and submodular).  `count` times the row not picked yet with the largest gain g_j = 1/2 sum_k log1p(max(d_k[j], 0) / s2) is
 * picked, ties to the lower index; d_k[j] is the variance of f_k(x_j) given noisy observations at every pick so far, and starts as mode 4's
 * f_var (its clamp included) widened to the solve precision.  Pick t at row p updates, per topic,
 *   c_k,t[j] = (C_k[j][p] - sum_{s<t} c_k,s[j] c_k,s[p]) / sqrt(d_k[p] + s2),    d_k[j] -= c_k,t[j]^2
 * so sum_t gain_t = I(picked).  s2 > 0 keeps every pivot positive: there is no failure flag and no jitter.  Link, Phi and mean do not enter.
 *   given_dev  G rows (scaled once, as X), or NULL with G = 0: places already sampled.  They are forced pivots, in their order, ahead of the
 *              free picks; they are no candidates and their gains are not returned
 *   idx_out    count int64 row indices in the order picked;  gains_out  count doubles, the gain of each pick when it was made
 *   var_out    NULL, or (K, n) doubles: d after the last pick
 * No n x n matrix is formed: one covariance column per pick comes from the solve-precision W of gdrf_predict_cov.  n >= 1, G >= 0,
 * n + G <= n_cap, 1 <= count <= n, G + count <= GDRF_SELECT_MAX_PICKS, noise positive and finite; 16 M solve-precision elements must fit
 * the pass's LDS (M <= 1120 with the f64 solve).  Needs gdrf_factorize().  Runs the step's forward (as mode 4) over the n + G rows, so it
 * overwrites the same workspaces; its own buffers ((n + G) M, K (G + count) (n + G) and K (n + G) solve-precision elements) are allocated on
 * first use and grow with the call.  Nothing is read back between the picks.  No atomics: bit-identical from call to call. */
#define GDRF_SELECT_MAX_PICKS 256
int gdrf_select_batch(gdrf_ctx* ctx, const void* X_dev, int64_t n, const void* Z_dev, const void* params_dev, const void* given_dev, int G, int count,
                      double noise, int64_t* idx_out_dev, double* gains_out_dev, double* var_out_dev, void* stream);

/* The greedy conditional-variance choice of `count` inducing points among the n rows X (csrc/select_inducing.h): the pivoted partial Cholesky
 * of the PRIOR kernel matrix K_nn (Burt, Rasmussen, van der Wilk 2020, Alg. 1), gdrf_select_batch's rule without a posterior.  With k the
 * context's kernel at the hyper-parameters in params_dev (every kind, ARD, Periodic and Product), all in the solve precision:
 *   d[j] = k(x_j, x_j);   pick t:  p = the t-th given row (t < G), else the candidate not picked yet with the largest d[j], ties to the lower
 *   index;  piv_t = d[p];  if piv_t > floor:  c_t[j] = (k(x_j, x_p) - sum_{s<t} c_s[j] c_s[p]) / sqrt(piv_t),  d[j] -= c_t[j]^2;  else c_t = 0
 *   (a degenerate pick: nothing left to explain, or a duplicate among the given rows);  trace_t = sum_{j<n} d[j] = tr(K_nn - Q_nn) so far.
 *   given_dev   G rows (scaled once, as X), or NULL with G = 0: forced pivots, in their order, ahead of the free picks; they are no candidates
 *   floor       pivots at or below it are degenerate; the rounding of the history sum, (G + count) eps k(x, x), is the level to pass
 *   idx_out     count int64 row indices in the order picked (may be NULL when count = 0)
 *   pivots_out, trace_out   G + count doubles each, the given rows included: d[p] when pick t was made, the residual trace after it
 *   resid_out   NULL, or (n) doubles: d after the last pick, diag(K_nn - Q_nn)
 *   rank_out    one int: the picks with piv_t > floor
 * n >= 1, G >= 0, n + G <= n_cap, 0 <= count <= n, G + count >= 1, G + count <= GDRF_INDUCING_MAX_PICKS, floor finite and >= 0.  count = 0
 * with G > 0 scores an existing set of points.  Needs no factorisation; neither Z nor the variational parameters enter, and no workspace of the
 * context is written.  Its buffers, (G + count + 1) (n + G) solve-precision elements, are allocated by the call and released before it
 * returns, so it synchronises the stream.  Two launches per pick, nothing read back between the picks.  No atomics: bit-identical from call
 * to call. */
#define GDRF_INDUCING_MAX_PICKS 1024
int gdrf_select_inducing(gdrf_ctx* ctx, const void* X_dev, int64_t n, const void* params_dev, const void* given_dev, int G, int count, double floor,
                         int64_t* idx_out_dev, double* pivots_out_dev, double* trace_out_dev, double* resid_out_dev, int* rank_out_dev, void* stream);

/* Did the last gdrf_factorize() hit a non-positive pivot?  Synchronises the stream. */
int gdrf_chol_failed(gdrf_ctx* ctx, int* failed_host, void* stream);

/* Borrowed pointers into the workspace (for parity tests): which = 0 W, 1 Wbar, 2 q, 3 loc, 4 tt,
 * 5 vbar, 6 locbar, 7 asum, 8 Kuu, 9 L, 10 Linv, 11 S, 12 B, 13 phi, 14 mu, 15 LinvT, 16 ST, 17 the step's K_nm, 18 the guide-side
 * locbar of gdrf_step_local2 (d elbo / d guide-side loc and mean; 0 elements before its first call). */
int gdrf_ws_ptr(gdrf_ctx* ctx, int which, void** ptr, int64_t* nelem);
/* Element size (4 or 8 bytes) of that buffer: Kuu, L, Linv, LinvT and the step's K_nm live in the solve precision. */
int gdrf_ws_elem_size(gdrf_ctx* ctx, int which);
/* Device-to-device copy of the first nelem elements of that buffer into dst_dev. */
int gdrf_ws_copy(gdrf_ctx* ctx, int which, void* dst_dev, int64_t nelem, void* stream);

/* Per-kernel timing with HIP events recorded on the launch stream (off by default).  Slots:
 * 0 probe, 1 k_nm, 2 transforms+B_k, 3 fwd_w, 4 loc (W U^T), 5 fwd_t, 6 elbo_rows, 7 bwd_wbar,
 * 8 bwd_knm, 9 tn_sym (A_k), 10 tn_gt, 11 slab reductions, 12 ubar, 13 step_finish, 14 adam / gdrf_optim_step, 15 factorize.
 * gdrf_get_timing synchronises on the recorded events and returns accumulated ms and counts. */
int gdrf_set_timing(gdrf_ctx* ctx, int enable);
int gdrf_get_timing(gdrf_ctx* ctx, double* ms_out, int64_t* count_out, int nslots);

/* The kernel form each stage that the host picks from K, Mp or n launched in the most recent call that ran it (host bookkeeping,
 * no synchronisation; 0 = not run yet in this context).  out[i] = slot i for i < n (slots past GDRF_NFORMS read 0):
 *   GDRF_FORM_WBAR         Wbar: 1 gemm_nt (dense B_k), 2 gemm_nt on the stored T_k, 3 bwd_wbar_split<SP,1>, 4 bwd_wbar_split<SP,2>,
 *                          5 bwd_wbar_split_cc, 6 bwd_wbar_f16_k64, 7 bwd_wbar_f16_w1 (one wave per SIMD, B_k from L2 to registers)
 *   GDRF_FORM_WBAR_NSLICE  reduction slices of the k64 form (> 1: partial sums in slabs, then wbar_slab_sum); 1 for the others
 *   GDRF_FORM_AK           A_k: 1 gemm_tn, 2 gemm_tn_split, 3 tn_topics_f16 (two waves per SIMD), 4 tn_topics_w2 (one wave per SIMD)
 *   GDRF_FORM_AK_KGROUPS   10-topic groups of forms 3 and 4 (0 for the others)
 *   GDRF_FORM_FWD_T        tt: 1 gemm_nt, 2 fwd_t_split_q4, 3 fwd_t_split_cc, 4 fwd_t_f16_w1 (one wave per SIMD, two topics per wave,
 *                          S_k^T from L2 to registers)
 *   GDRF_FORM_FWD_T_KG     topics per L2 group of forms 2, 3 and 4 (0 for gemm_nt)
 *   GDRF_FORM_LOC          loc = W U^T: 1 loc_rows, 2 gemm_nt, 3 gemm_nt with two column tiles (f64, K > 64)
 *   GDRF_FORM_UBAR_Q4      topic quads per pass of ubar_part
 *   GDRF_FORM_ROWS         row terms: 1 elbo_rows_mfma, 2 elbo_rows (one thread per row), 3 vocabulary-streamed
 *   GDRF_FORM_ROWS_KT, _VT 16-topic and 16-word tiles of elbo_rows_mfma (0 for the others)
 *   GDRF_FORM_GT           G^T = W^T Wbar: 1 gemm_tn, 2 gemm_tn_split
 *   GDRF_FORM_HYPER        K_nm parts of the hyper-parameter gradients: 1 the backward GEMM (form 0 of gdrf_set_hyper_backward), 2 Hd (form 1)
 *   GDRF_FORM_PREDICT      gdrf_predict modes 0-3: 1 predict_mfma, 2 predict_rows with the coefficients in LDS, 3 predict_rows reading them
 *                          from memory, 4 predict_rows_bigk (K > 32), 5 the streamed route (row form 1, or mode 3 on a bound CSR matrix);
 *                          mode 4 runs the step's forward and leaves both slots as they are
 *   GDRF_FORM_PREDICT_NB   16-topic column blocks of predict_mfma (0 for the others)
 *   GDRF_FORM_MM_CHAIN     the single M x M products of step_finish's Cholesky backward (solve precision): 1 one launch of the NT core,
 *                          2 the reduction split over 8 slices into the context's slab buffer and summed in a fixed order
 *   GDRF_FORM_MM_SBAR      Sbar_k = 2 A_k S_k of step_finish (array precision), the same codes: always 1 for K >= 2, and always 1 in the
 *                          whitened form, where it runs on the side stream beside the chain and must not share the chain's slab buffer */
enum { GDRF_FORM_WBAR = 0, GDRF_FORM_WBAR_NSLICE, GDRF_FORM_AK, GDRF_FORM_AK_KGROUPS, GDRF_FORM_FWD_T, GDRF_FORM_FWD_T_KG, GDRF_FORM_LOC,
       GDRF_FORM_UBAR_Q4, GDRF_FORM_ROWS, GDRF_FORM_ROWS_KT, GDRF_FORM_ROWS_VT, GDRF_FORM_GT, GDRF_FORM_HYPER, GDRF_FORM_PREDICT,
       GDRF_FORM_PREDICT_NB, GDRF_FORM_MM_CHAIN, GDRF_FORM_MM_SBAR, GDRF_NFORMS };
int gdrf_last_forms(const gdrf_ctx* ctx, int* out, int n);

#ifdef __cplusplus
}
#endif
#endif
