/* gpfit_mi355x.h -- C ABI of the MI355X-native GP fit path (libgpfit_mi355x.so).
 *
 * Drop-in boundary for the hot path of Spatial_GP_repo/utils.py (the reference has no
 * FFI layer of its own; the Python module gaussian_processes_amd/utils.py binds these
 * entry points with ctypes and keeps the reference's function signatures).
 *
 * Conventions
 *   - every matrix/vector pointer is a DEVICE pointer to contiguous row-major fp64 unless
 *     the parameter is documented as host; the caller owns every buffer; the library
 *     owns only the workspace inside a gpfit_ctx;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls enqueue
 *     work and return unless documented as synchronising;
 *   - return value: 0 ok; > 0 LAPACK-style info (1-based index of the first
 *     non-positive pivot); < 0 argument / runtime error (-2 = hyperparameter outside
 *     its limits, -3 = bad argument, -100 = HIP runtime error), message from
 *     gpfit_last_error();
 *   - hyperparameter vectors are double[6] in the reference's dict order
 *     sigma_0, eps_0x, eps_0y, -2log2beta, -log2rho2, Amp  (utils.py:824).
 */
#ifndef GPFIT_MI355X_H
#define GPFIT_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPFIT_VERSION 100

int gpfit_version(void);
const char* gpfit_last_error(void);

/* Raw fp64 MFMA GEMM:  C[M,N] = alpha * op(A)[M,K] * op(B)[K,N] + beta * C.
 * Replaces the torch `@` / torch.matmul call sites of the path (utils.py:978-982,
 * 1012-1017, 2047-2062, 1318-1333).  a_kmajor: 0 = A stored [M][K], 1 = A stored [K][M];
 * b_kmajor: 1 = B stored [K][N], 0 = B stored [N][K].  out_lower: compute only the 128-tiles
 * on/below the diagonal; a_tri/b_tri: 0 dense, 1 op() lower-, 2 op() upper-triangular.
 * K % 16 == 0; M, N, lda, ldb even.  Runs on the caller's current device.  Large launches (>= 384
 * output tiles of 128 x 128, K >= 1024) may use the stream-K schedule; its partial-tile workspace is
 * kept per (device, stream) for this context-free entry point, so calls on different streams are
 * independent (the context-based entry points own their workspaces). */
int gpfit_dgemm(void* stream, int a_kmajor, int b_kmajor, int M, int N, int K, double alpha,
                const double* A, int64_t lda, const double* B, int64_t ldb, double beta, double* C,
                int64_t ldc, int out_lower, int a_tri, int b_tri);
/* Same with the tuning knobs exposed: walk (bit 0: tile grid backwards, bit 1: column-major -- also
 * for the lower triangle of an out_lower launch --, bit 2: every tile walks k downwards, bit 3: XCD-aware
 * macro-tile schedule for launches of >= 1536 tiles, bit 4: one workgroup per CU)
 * and tile (0 = automatic, or 128 / 64 / 32).  Where only the tail of a launch takes the stream-K schedule,
 * head and tail follow the same walk, so every combination of the bits covers the output exactly once. */
int gpfit_dgemm_ex(void* stream, int a_kmajor, int b_kmajor, int M, int N, int K, double alpha,
                   const double* A, int64_t lda, const double* B, int64_t ldb, double beta, double* C,
                   int64_t ldc, int out_lower, int a_tri, int b_tri, int walk, int tile);

/* ---- workspace context -------------------------------------------------------------
 * One context per (device, maximum problem size); owns ~13 N^2 + O(N d) doubles of HBM
 * workspace, one auxiliary HIP stream and two events.  A context is NOT re-entrant: calls
 * on the same context must be serialised by the caller (one context per host thread; the Python
 * module keeps one per (device, thread)).  Every context entry point selects the context's device
 * for the duration of the call and restores the caller's current device on return; while an
 * asynchronous evaluation is pending (gpfit_fit_eval bit 2) every other entry point on that
 * context returns -3 until gpfit_fit_eval_finish has collected it.
 * n_max: stimuli; d_max: masked pixels; d_full_max: pixels of the full image. */
typedef struct gpfit_ctx gpfit_ctx;
int gpfit_ctx_create(int device, int64_t n_max, int64_t d_max, int64_t d_full_max, gpfit_ctx** out);
void gpfit_ctx_destroy(gpfit_ctx* ctx);

/* Hyperparameter box check of localker (utils.py:865-867) / closure_hyperparams
 * (utils.py:2020-2028).  0 inside, -2 outside (message names the offender).  Host only. */
int gpfit_check_limits(const double* theta, const double* lower, const double* upper);

/* Pixel mask of localker (utils.py:880-883) for an n_rows x n_cols grid: mask_host[p] = 1
 * where alpha_p >= 0.001; *d_out = number of kept pixels.  Host only (n_rows*n_cols exps). */
int gpfit_localker_mask(const double* theta, int n_rows, int n_cols, uint8_t* mask_host, int64_t* d_out);

/* localker (utils.py:861-914): spatial metric C[d][d] over the kept pixels of an n_rows x
 * n_cols grid and, when dC is non-NULL, its five derivatives as dC[5][d][d] in the order
 * Amp, -2log2beta, -log2rho2, eps_0x, eps_0y (the key order of the reference's dC dict,
 * utils.py:910).  mask_host/d come from gpfit_localker_mask.  Synchronises `stream`. */
int gpfit_localker(gpfit_ctx* ctx, void* stream, const double* theta, int n_rows, int n_cols,
                   const uint8_t* mask_host, int64_t d, double* C, double* dC);

/* acosker, diag=False (utils.py:968-1025): K[n1][n2] from already-masked x1[n1][d],
 * x2[n2][d] and the metric C[d][d]; symmetrised when n1 == n2 (utils.py:1024).  When dK is
 * non-NULL it receives six [n1][n2] matrices in theta dict order (sigma_0, eps_0x, eps_0y,
 * -2log2beta, -log2rho2, Amp); dC (layout as gpfit_localker) may be NULL, in which case only
 * the sigma_0 derivative is written.  Pass x2 == x1 for the square self-kernel (lower-tile
 * fast path).  Enqueues on `stream`, does not synchronise. */
int gpfit_acosker(gpfit_ctx* ctx, void* stream, double sigma0, const double* x1, int64_t ld1, int64_t n1,
                  const double* x2, int64_t ld2, int64_t n2, int64_t d, const double* C, int64_t ldC,
                  const double* dC, double* K, int64_t ldk, double* dK);

/* Rectangular pull-back for acosker(x1, x2), x1 != x2 (the K[n_t][n_tilde] of the sparse regime):
 * for an adjoint W[n1][n2] of K, the contraction sum_ij W_ij dK_p,ij with the reference's analytic
 * derivatives (utils.py:996-1021) reduces to <dC_p, sym(M)> for the five metric parameters and to
 * sigma_0 (2 out[0] + out[1] + out[2]) for sigma_0, with
 *   A_w = W o (pi - delta)/pi,  B_m = W o sqrt(1 - c^2)/pi,  u1 = B_m q2,  u2 = B_m^T q1,
 *   M = x1^T A_w x2 + x1^T diag(u1/(2 q1) + t1_extra) x1 + x2^T diag(u2/(2 q2)) x2      (d x d),
 *   out_host[3] = { sum A_w, sum u1/q1, sum u2/q2 }.
 * x1[n1][ld1], x2[n2][ld2] already masked, C[d][ldC]; t1_extra[n1] may be NULL (it carries the
 * dKvec adjoint of the closure); M_out[d][ldm] device.  Nothing n1 x n2 x 6 is materialised.
 * Synchronises. */
int gpfit_acosker_pullback(gpfit_ctx* ctx, void* stream, double sigma0, const double* x1, int64_t ld1,
                           int64_t n1, const double* x2, int64_t ld2, int64_t n2, int64_t d, const double* C,
                           int64_t ldC, const double* W, int64_t ldw, const double* t1_extra, double* M_out,
                           int64_t ldm, double* out_host);

/* acosker, diag=True (utils.py:1027-1044): Kvec[n1] = x_i C x_i + sigma_0^2 and optionally
 * dKvec[6][n1] (theta dict order). */
int gpfit_acosker_diag(gpfit_ctx* ctx, void* stream, double sigma0, const double* x1, int64_t ld1,
                       int64_t n1, int64_t d, const double* C, int64_t ldC, const double* dC, double* Kvec,
                       double* dKvec);

/* The fused unit of work: ONE evaluation of the M-step closure (utils.py:2017-2112) in the
 * full-rank regime (n_tilde == n_t, all eigenvalues kept), original basis:
 *   localker -> acosker (K~, Kvec) -> Cholesky(K~), Cholesky(V) -> lambda moments, f,
 *   log-likelihood, KL -> the six analytic gradients.
 * X[N][ldx] is the UN-masked stimulus matrix (device), r, m [N], V[N][ldv] symmetric (device).
 * out_host[16] (HOST): 0 loss = -(loglik - KL), 1 loglik, 2 KL, 3..8 d loss/d theta (dict order),
 *   9 log|K~|, 10 log|V|, 11 tr(K~^-1 V), 12 m^T K~^-1 m, 13 masked pixel count,
 *   14 info(K~), 15 info(V).  (In the library: enum OutSlot of csrc/context.h -- OUT_LOSS, OUT_LOGLIK, OUT_KL,
 *   OUT_GRAD, OUT_LOGDET_K, OUT_LOGDET_V, OUT_TRACE, OUT_MKM, OUT_D, OUT_INFO_K, OUT_INFO_V.)
 * want_grad: bit 0 = compute the gradients; bit 1 = V is unchanged since the previous call on
 * this context (constant during an M-step): reuse its Cholesky factor and log-det; bit 2 =
 * asynchronous: only enqueue on `stream` and return (out_host is not written); the caller collects
 * the result with gpfit_fit_eval_finish.  Independent units (other cells, other theta points) can
 * then be kept in flight on several contexts / streams, so that one unit's latency-bound
 * factorisation overlaps another's GEMMs (multi.py); bit 3 = mixed precision (fp64 entry point only):
 * kernel build, both Cholesky factorisations, both log-determinants, the likelihood and m^T K~^-1 m in fp64, the
 * N^3-heavy products (T, Q, W and the pull-back) in fp32 on single-precision copies of the factors -- T's norm
 * included, so the trace term tr(K~^-1 V) of the loss is fp32-derived (measured effect on the loss: 2e-9 relative
 * over the 512-point lattice at N = 8192, asserted <= 1e-7 in tests/test_gpu_fp32.py) -- the hyperparameter-grid configuration (BASELINE configs[4]) at the north star's 1e-5
 * bar on the log marginal likelihood, which the all-fp32 instance misses on some grid points.
 * lam_m/lam_var/f (device, [N]) may be NULL.  Synchronises `stream` before returning unless bit 2.
 * Returns 0; -2 when theta is outside [lower, upper] (out_host[0] = +inf and gradients
 * +inf, exactly what the reference closure hands to L-BFGS); > 0 LAPACK info. */
int gpfit_fit_eval(gpfit_ctx* ctx, void* stream, const double* theta, const double* lower,
                   const double* upper, int n_rows, int n_cols, const double* X, int64_t ldx, int64_t N,
                   const double* r, const double* m, const double* V, int64_t ldv, double logA,
                   double lambda0, int want_grad, double* out_host, double* lam_m, double* lam_var,
                   double* f);

/* Collect the evaluation enqueued on `ctx` by gpfit_fit_eval / gpfit_fit_eval_f32 with bit 2 of
 * want_grad: waits for its stream, writes out_host[16] and returns what the synchronous call
 * would have returned (0 or the LAPACK info).  -3 if nothing is pending.  A unit enqueued by
 * gpfit_fit_eval_batch waits for its GROUP's completion event instead of the stream, so a later group (on other
 * contexts) may already be running on the same stream while this one is collected. */
int gpfit_fit_eval_finish(gpfit_ctx* ctx, double* out_host);

/* n_units (1 .. 16) independent units of work of the same N in one call -- the cells / hyperparameter-grid
 * points of BASELINE configs[3], [4] (no dependency between units), unit u on its own context
 * ctxs[u] with theta[6 u ..], X[u], r[u], m[u], V[u] (device pointers; X may be the same matrix for every
 * unit), logA[u], lambda0[u].  Replaces n_units calls of the closure utils.py:2017-2112.  Everything runs on
 * `stream`: the 2 n_units Cholesky recursions in lock step (their latency-bound leaves and small products are
 * shared launches), the products behind them as pointer-batched launches wherever one unit's product cannot
 * fill the chip.  Each unit's results are bit-identical to gpfit_fit_eval on its own.  want_grad: bits 0, 1, 3
 * as gpfit_fit_eval; the call is always asynchronous: rc_out[u] = 0 -> collect unit u with
 * gpfit_fit_eval_finish(ctxs[u], ...); -2 -> theta outside the limits, out_host[16 u ..] already holds the
 * infinite loss / gradients and nothing is pending.  A group's per-unit housekeeping is two launches (pixel
 * lists / info words / padded means at the start; the 64 result scalars and info words of every unit written
 * straight into its pinned host buffers at the end, followed by the completion event gpfit_fit_eval_finish waits
 * for).  Returns 0 or < 0 (bad argument / capacity / HIP error). */
int gpfit_fit_eval_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* theta,
                         const double* lower, const double* upper, int n_rows, int n_cols,
                         const double* const* X, int64_t ldx, int64_t N, const double* const* r,
                         const double* const* m, const double* const* V, int64_t ldv, const double* logA,
                         const double* lambda0, int want_grad, double* out_host, int* rc_out);
/* The same for the fp32 instance of the library (gpfit_fit_eval_f32). */
int gpfit_fit_eval_batch_f32(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* theta,
                             const double* lower, const double* upper, int n_rows, int n_cols,
                             const float* const* X, int64_t ldx, int64_t N, const float* const* r,
                             const float* const* m, const float* const* V, int64_t ldv, const double* logA,
                             const double* lambda0, int want_grad, double* out_host, int* rc_out);

/* Gradient pull-back for an externally supplied adjoint: out_host[6] (theta dict order) =
 *   sum_ij W_ij dK~_p,ij + sum_i gvec_i dKvec_p,i
 * with the reference's analytic derivatives dK~_p (acosker, utils.py:996-1021) and dKvec_p
 * (utils.py:1036-1044) at theta, without materialising any dK (the contraction is pulled back to
 * the d x d metric, as in gpfit_fit_eval).  X[N][ldx] un-masked stimuli, W[N][ldw] symmetric
 * (lower triangle read), gvec[N], all device.  Serves the truncated-rank (B-projected) closure
 * of utils.py:2047-2099, whose n x n adjoints lift to W = (B G_Kb~ + G_Kb) B^T.  Synchronises. */
int gpfit_grad_pullback(gpfit_ctx* ctx, void* stream, const double* theta, int n_rows, int n_cols,
                        const double* X, int64_t ldx, int64_t N, const double* W, int64_t ldw,
                        const double* gvec, double* out_host);

/* Truncated-rank M-step closure, fused: the reference's B-projected closure (utils.py:2030-2099) in the
 * regime its default EIGVAL_TOL produces at realistic sizes -- inducing set = training set, n_kept < N
 * eigen-directions kept.  X[N][ldx] un-masked stimuli, r[N], B[N][ldb] the kept eigenvectors (orthonormal
 * columns, utils.py:1685), m_b[n_kept], V_b[n_kept][ldvb], all device.  One call does the kernel build,
 * the projections K_b = K~ B and K~_b = sym(B^T K_b), the Cholesky factorisations of K~_b and V_b, the
 * moments / likelihood / KL of utils.py:1090-1326 with a = B (:2068), the adjoints of the loss with
 * respect to K_b, K~_b and Kvec (da_p of :1114 included), their lift to the N x N adjoint
 * W = (B G_K~b + G_Kb) B^T and its contraction with the analytic dK~_p / dKvec_p by the pull-back to
 * the metric -- no dK, no N x N x 6 tensor, nothing computed by the host framework.
 * out_host[16] as gpfit_fit_eval (9 log|K~_b|, 10 log|V_b|, 11 tr(K~_b^-1 V_b), 12 m_b^T K~_b^-1 m_b,
 * 14 / 15 LAPACK info of the two factorisations).  Returns 0; -2 outside the hyperparameter box
 * (infinite loss and gradients); > 0 when a factorisation meets a non-positive pivot (the caller then
 * takes the reference's eigen-fallback of log_det, utils.py:1279-1304).  Synchronises. */
int gpfit_fit_eval_projected(gpfit_ctx* ctx, void* stream, const double* theta, const double* lower,
                             const double* upper, int n_rows, int n_cols, const double* X, int64_t ldx, int64_t N,
                             const double* r, const double* B, int64_t ldb, int64_t n_kept, const double* m_b,
                             const double* V_b, int64_t ldvb, double logA, double lambda0, double* out_host);

/* gpfit_fit_eval_projected for 1 .. GPFIT_FIT_EVAL_PROJECTED_MAX_UNITS independent units -- cells recorded on the same
 * stimuli, restarts of one cell -- as ONE call: unit u runs on its own context ctxs[u] (pairwise distinct, one device, one
 * capacity) with its own theta[6u ..], lower[6u ..], upper[6u ..] (both NULL: no limits), X[u] (may be the same matrix for
 * every unit), r[u], B[u], ldb[u], n_kept[u], m_b[u], V_b[u], ldvb[u], logA[u], lambda0[u]; n_rows, n_cols, ldx and N are
 * shared.  Everything is enqueued on `stream`, one synchronisation at the end.  The kernel builds and the pull-backs run
 * unit by unit (the masked pixel count differs from unit to unit); between them the 2 n_units factorisations run as one
 * lock-step recursion, every product goes out for the list of units and every small kernel is one launch for the group,
 * so that stretch costs the launches of one unit.  (Two chains per unit in a pointer batch of 32: hence 16 units.)
 * All units of a call must have the same round_up(n_kept[u], 128) (n_kept[u] itself may differ): the recursion's split
 * depends on the padded size.  All contexts of a call must have been created for the same number of stimuli
 * (round_up(n_max, 128)): the k slabs of the projections and the route of the lift W depend on a context's capacity, and
 * a unit takes in a group exactly what it takes alone on its context.  Otherwise -3 -- the caller groups its units by
 * padded size and capacity.
 * out_host[16 n_units]: the 16 slots of gpfit_fit_eval_projected, unit by unit, each with the bits of that call on the
 * unit alone (on the same context) whatever else is in the group.  rc_out[n_units]: what the single call would have
 * returned for the unit -- 0; -2 theta outside the unit's limits (its slots hold the infinite loss and gradients, nothing
 * was enqueued for it); > 0 the LAPACK info of a failed pivot, which changes nothing in the other units.
 * Returns 0, or < 0 for a bad argument, insufficient capacity or a HIP error: for the first two nothing has been
 * enqueued and neither out_host nor rc_out has been written.  gpfit_fit_eval_projected itself is this call with one
 * unit. */
#define GPFIT_FIT_EVAL_PROJECTED_MAX_UNITS 16
int gpfit_fit_eval_projected_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* theta,
                                   const double* lower, const double* upper, int n_rows, int n_cols,
                                   const double* const* X, int64_t ldx, int64_t N, const double* const* r,
                                   const double* const* B, const int64_t* ldb, const int64_t* n_kept,
                                   const double* const* m_b, const double* const* V_b, const int64_t* ldvb,
                                   const double* logA, const double* lambda0, double* out_host, int* rc_out);

/* Sparse M-step closure, fused: n_tilde < n_t inducing stimuli (the regime of the lab's own fits,
 * one_cell_fit.ipynb:89: n_t ~ 3160, n_tilde up to 2100): K[n_t][n_tilde] = acosker(x, xtilde) differs from
 * K~ = acosker(xtilde, xtilde), a = K_b K~_b^-1 (utils.py:1693, 2068) and da_p is non-zero (:1114).
 * X[N][ldx] training stimuli, Xtilde[Ntilde][ldxt] inducing stimuli (both un-masked), B[Ntilde][ldb] the
 * kept eigenvectors of K~, m_b[n_kept], V_b[n_kept][ldvb].  As gpfit_fit_eval_projected, with two
 * adjoints pulled back to the metric: B G_K~b B^T against dK~_p on the inducing stimuli and G_Kb B^T
 * against dK_p on (x, xtilde), the dKvec term riding on the latter.  Same out_host and return
 * conventions.  Synchronises. */
int gpfit_fit_eval_sparse(gpfit_ctx* ctx, void* stream, const double* theta, const double* lower, const double* upper,
                          int n_rows, int n_cols, const double* X, int64_t ldx, int64_t N, const double* Xtilde,
                          int64_t ldxt, int64_t Ntilde, const double* r, const double* B, int64_t ldb, int64_t n_kept,
                          const double* m_b, const double* V_b, int64_t ldvb, double logA, double lambda0,
                          double* out_host);

/* gpfit_fit_eval_sparse (the reference's M-step closure, utils.py:2030-2099) for 1 .. GPFIT_FIT_EVAL_SPARSE_MAX_UNITS
 * independent units -- cells recorded on the same stimuli, restarts of one cell -- as ONE call: unit u runs on its own
 * context ctxs[u] (pairwise distinct, one device) with its own theta[6u ..], lower[6u ..], upper[6u ..] (both NULL: no
 * limits), X[u], Xtilde[u] (may be the same matrix for every unit), r[u], B[u], ldb[u], n_kept[u], m_b[u], V_b[u],
 * ldvb[u], logA[u], lambda0[u]; n_rows, n_cols, ldx, N, ldxt, Ntilde are shared.  Everything is enqueued on `stream`,
 * one synchronisation at the end.  The kernel builds and the two pull-backs run unit by unit (the masked pixel count
 * differs from unit to unit); between them the 2 n_units factorisations run as one lock-step recursion, every product
 * goes out for the list of units and every small kernel is one launch for the group, so that stretch costs the launches
 * of one unit.  (Two chains per unit in a pointer batch of 32: hence 16 units.)
 * All units of a call must have the same round_up(n_kept[u], 128) (n_kept[u] itself may differ): the recursion's split
 * depends on the padded size; otherwise -3 -- the caller groups its units by padded size.
 * out_host[16 n_units]: the 16 slots of gpfit_fit_eval_sparse, unit by unit, each with the bits of that call on the unit
 * alone whatever else is in the group.  rc_out[n_units]: what the single call would have returned for the unit -- 0; -2
 * theta outside the unit's limits (its slots hold the infinite loss and gradients, nothing was enqueued for it); > 0 the
 * LAPACK info of a failed pivot, which changes nothing in the other units.
 * Returns 0, or < 0 for a bad argument, insufficient capacity or a HIP error: for the first two nothing has been
 * enqueued and neither out_host nor rc_out has been written.  gpfit_fit_eval_sparse itself is this call with one unit. */
#define GPFIT_FIT_EVAL_SPARSE_MAX_UNITS 16
int gpfit_fit_eval_sparse_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* theta,
                                const double* lower, const double* upper, int n_rows, int n_cols,
                                const double* const* X, int64_t ldx, int64_t N, const double* const* Xtilde,
                                int64_t ldxt, int64_t Ntilde, const double* const* r, const double* const* B,
                                const int64_t* ldb, const int64_t* n_kept, const double* const* m_b,
                                const double* const* V_b, const int64_t* ldvb, const double* logA,
                                const double* lambda0, double* out_host, int* rc_out);

/* Cholesky factorisation A = L L^T of a symmetric positive definite n x n matrix (lower
 * triangle read) by the recursive MFMA algorithm; replaces torch.linalg.cholesky in log_det
 * (utils.py:1275) and, through L^-1, the LU torch.linalg.solve(., I) of the closure
 * (utils.py:2067).  L / Linv (device, may be NULL) receive the factor and its inverse with the
 * strict upper part zeroed; *logdet_host = 2 sum log L_ii (utils.py:1278).  Synchronises.
 * Returns 0, or the LAPACK info (1-based index of the first non-positive pivot). */
int gpfit_potrf(gpfit_ctx* ctx, void* stream, const double* A, int64_t lda, int64_t n, double* L, int64_t ldl,
                double* Linv, int64_t ldi, double* logdet_host, int* info_host);

/* Rank-1 append to a Cholesky factorisation: given L and L^-1 of the n x n matrix K (device, row-major,
 * leading dimensions > n so that row and column n exist) and kcol[0..n] = the new last column of
 * K' = [K k; k^T kappa] (device), writes row n of both factors in place,
 *   L'[n][:] = (l^T, lambda),  L'^-1[n][:] = (-(L^-T l)^T / lambda, 1 / lambda),  l = L^-1 k,
 *   lambda = sqrt(kappa - l.l),
 * zeroes column n above the diagonal and adds 2 log(lambda) to *logdet_inout_host.  O(n^2) instead of
 * the O(n^3) refactorisation: the closed loop of one_cell_active_training.ipynb appends one stimulus
 * per iteration and updates its kernel matrices 'by their latest column' (:1889-1891).  Synchronises.
 * Returns 0, or n + 1 (LAPACK info) when the Schur complement kappa - l.l is not positive. */
int gpfit_potrf_append(gpfit_ctx* ctx, void* stream, double* L, int64_t ldl, double* Linv, int64_t ldi, int64_t n,
                       const double* kcol, double* logdet_inout_host, int* info_host);

/* Block append: k rows at once (1 <= k <= 128).  L and L^-1 of the n x n matrix K sit in the leading blocks of
 * (n + k)-sized arrays (device, row-major, ldl, ldi >= n + k) as for the rank-1 call; Kcols[n + k][ldk >= k] holds the
 * new last k columns of K' = [K K12; K12^T K22] (device, row-major; of its bottom k x k block only the lower
 * triangle is read, and of L^-1 only its lower triangle).  Writes rows n .. n + k - 1 of both factors in place,
 *   Y = L^-1 K12,  L21 = Y^T,  L22 = chol(K22 - Y^T Y),  [L'^-1]22 = L22^-1,  [L'^-1]21 = -L22^-1 Y^T L^-1,
 * zeroes columns n .. n + k - 1 of the rows above and the strict upper triangles of the new diagonal blocks, and
 * adds 2 sum log diag L22 to *logdet_inout_host.  O(n^2 k) in two passes over L^-1, a fixed number of launches
 * whatever n and k, no floating-point atomics (the same inputs give the same bits), one synchronisation.
 * Returns 0, or the LAPACK info n + j + 1 (1-based, in K') of the first non-positive pivot: rows n .. are then
 * meaningless, the leading n x n blocks and the log-det are untouched.  -3: a null pointer, n < 1, k outside
 * 1 .. 128, ldl or ldi < n + k, ldk < k, n + k above the context capacity, a pending asynchronous evaluation
 * (the argument checks come before the context or the device is touched). */
int gpfit_potrf_append_block(gpfit_ctx* ctx, void* stream, double* L, int64_t ldl, double* Linv, int64_t ldi, int64_t n,
                             int64_t k, const double* Kcols, int64_t ldk, double* logdet_inout_host, int* info_host);

/* E-step Newton update of q(lambda~) = N(m, V) (Estep, alpha = 1 branch, utils.py:1420-1439) in
 * the original basis (a = I): with s = A sqrt(f), M = I + S K~ S = L_M L_M^T, T = L_M^-1 S K~:
 *   V_new = K~ - T^T T,  m_new = V_new (A^2 f o m + A (r - f)).
 * K~[N][ldk] symmetric (full), r, m, f [N] -> m_new [N], V_new[N][ldv] (full, symmetric).
 * Synchronises; returns LAPACK info if M is not positive definite. */
int gpfit_estep(gpfit_ctx* ctx, void* stream, const double* K, int64_t ldk, int64_t N, const double* r,
                const double* m, const double* f, double logA, double* m_new, double* V_new, int64_t ldv);

/* The same Newton update in the basis in force when K~ is truncated or the inducing set is a subset (the else branch of
 * varGP's E-step, utils.py:1880 -> Estep :1420-1439 with a = K K~^-1 in the B basis): with L = chol(K~_b) and
 * aL = a L supplied by the caller (both fixed between two kernel rebuilds, i.e. over the nEstep updates of an EM
 * iteration), s = A sqrt(f), Y = diag(s) aL:
 *   W = I + Y^T Y = I + L^T G L = L_W L_W^T        (G = A^2 a^T diag(f) a, :1422)
 *   V_new = P P^T, P = L L_W^-T                     (= solve(I + K~ G, K~), :1430)
 *   m_new = L W^-1 aL^T u,  u = A^2 f o (a m) + A (r - f)   (= V_new (G m + g), :1431)
 * a[N][lda], aL[N][ldal] (N x nb), L[nb][ldl] lower, r, f [N], m [nb] -> m_new [nb], V_new[nb][ldv] (full, symmetric).
 * Optionally (all three pointers or none) the moments of lambda behind the update, which varGP evaluates next
 * (lambda_moments, utils.py:1090, 1101): with kv0 = Kvec - rowsum(K o a) [N] (fixed between kernel rebuilds) and
 * Z = aL L_W^-T,  lam_m = a m_new = Z (L_W^-1 aL^T u),  lam_var = kv0 + diag(a V_new a^T) = kv0 + row norms^2 of Z.
 * One call, one synchronisation; returns LAPACK info if W is not positive definite. */
int gpfit_estep_projected(gpfit_ctx* ctx, void* stream, const double* a, int64_t lda, const double* aL, int64_t ldal,
                          const double* L, int64_t ldl, int64_t N, int64_t nb, const double* r, const double* m,
                          const double* f, double logA, double* m_new, double* V_new, int64_t ldv, const double* kv0,
                          double* lam_m_out, double* lam_var_out);

/* The damped Newton update of the same basis (Estep with a step size alpha != 1, utils.py:1432-1436), in a form that
 * keeps V positive definite by construction.  The reference's
 *   V_new = V solve((1 - a) K~ + a V + a K~ G V, K~)      is      V_new^-1 = (1 - a) V^-1 + a (K~^-1 + G),
 * a convex combination of positive definite precisions for 0 < a <= 1.  With K~ = L L^T, Y = diag(A sqrt f) aL:
 *   W1  = I + Y^T Y = L_W1 L_W1^T                    (the matrix gpfit_estep_projected factors)
 *   P   = L^-1 V L^-T = L_P L_P^T                    (positive definite iff V is; factored beside W1 in lock step)
 *   W_a = (1 - a) L_P^-T L_P^-1 + a W1 = L_Wa L_Wa^T
 *   V_new = (L L_Wa^-T)(L L_Wa^-T)^T
 *   m_new = (1 - a) m + a L W1^-1 aL^T u              (u as in gpfit_estep_projected; equal to :1436, because
 *                                                     m - (I + K~ G)^-1 (m - K~ g) = (I + K~ G)^-1 K~ (G m + g))
 * Cholesky factorisations only: V_new is exactly symmetric and positive definite.  alpha = 1 gives the update of
 * gpfit_estep_projected (W_a = W1 then; V is still factored and must be positive definite).
 * Arguments as gpfit_estep_projected, without the moments, plus Linv[nb][ldli] = L^-1 and V[nb][ldv_in] = the current
 * V (symmetric); of both only the lower triangle is read.  V_new may be V itself (V is read before V_new is written).
 * Runs on the caller's stream, allocates nothing, synchronises once.
 * Returns 0, or a positive LAPACK info when a factorisation fails; *info_v_host (may be NULL) tells which one:
 *   *info_v_host != 0 (= the return value): V is not positive definite;
 *   *info_v_host == 0: I + L^T G L (or, behind it, W_a) is not positive definite -- NaN or negative rates.
 * gpfit_last_error() names the matrix as well.  The outputs are meaningless after a failure.
 * -3 (before the context or any operand is read): a null pointer, N or nb <= 0, a leading dimension < nb, alpha not
 * finite or outside (0, 1]; then: a problem above the context capacity, a pending asynchronous evaluation.
 * *info_v_host is written only when the call ran. */
int gpfit_estep_projected_damped(gpfit_ctx* ctx, void* stream, const double* a, int64_t lda, const double* aL,
                                 int64_t ldal, const double* L, int64_t ldl, const double* Linv, int64_t ldli,
                                 const double* V, int64_t ldv_in, int64_t N, int64_t nb, const double* r, const double* m,
                                 const double* f, double logA, double alpha, double* m_new, double* V_new, int64_t ldv,
                                 int* info_v_host);

/* One pass over the training points for the firing-rate parameters (mean_f_given_lambda_moments
 * utils.py:1126-1141, lambda0_given_logA :1215-1229, compute_loglikelihood with
 * compute_grad_for_f_params :1243-1255).  out_host[7]: lambda0 used (closed form if requested,
 * else lambda0_in), loglik, d loglik / d logA, sum f, sum r, r.lam_m, closed-form lambda0.
 * f_out (device [N]) may be NULL. */
int gpfit_fparam_eval(gpfit_ctx* ctx, void* stream, const double* lam_m, const double* lam_var,
                      const double* r, int64_t N, double logA, int closed_form_lambda0, double lambda0_in,
                      double* f_out, double* out_host);

/* The whole rate-parameter optimiser of an E-step (varGP utils.py:1892-1934: lambda0_given_logA, then
 * LBFGS([logA], lr, max_iter, tolerance_grad, tolerance_change, history_size, line_search_fn='strong_wolfe')
 * .step(closure_f_params), then lambda0_and_rate) as one launch of one workgroup and one synchronisation.  The
 * optimiser is a port of torch 2.10's LBFGS.step for one scalar (max_eval = max_iter*5/4); the closure's k-th call
 * evaluates the pass of gpfit_fparam_eval at (logA_k, lambda0_{k-1}) and then sets lambda0_k to the closed form at
 * logA_k, lambda0_0 being the closed form at logA0.  lambda0_mode = 1: every call uses lambda0_fixed instead
 * (f_params carrying loglambda0: exp(loglambda0)).  A non-finite sum f stops the optimiser.
 * out_host[9]: final logA, closed-form lambda0 there (NaN after a failure), first loss, last loss (at the final
 * logA), closure calls, iterations, status (0, or the 1-based number of the call whose sum f was not finite),
 * logA and lambda0 that call left behind (0 when status is 0).  f_out (device [N], may be NULL): the rate at the
 * final (logA, lambda0), written when status is 0.  history_size up to 2040. */
int gpfit_fparam_lbfgs(gpfit_ctx* ctx, void* stream, const double* lam_m, const double* lam_var,
                       const double* r, int64_t N, double logA0, int lambda0_mode, double lambda0_fixed,
                       int max_iter, int history_size, double lr, double tol_grad, double tol_change,
                       double* f_out, double* out_host);
/* The same optimiser and closure on host arrays (lam_m, lam_var, r, f_out), sums in index order: the CPU
 * instance that checks the port against torch.optim.LBFGS without a GPU.  Same arguments and results. */
int gpfit_fparam_lbfgs_host(const double* lam_m, const double* lam_var, const double* r, int64_t N,
                            double logA0, int lambda0_mode, double lambda0_fixed, int max_iter,
                            int history_size, double lr, double tol_grad, double tol_change, double* f_out,
                            double* out_host);

/* The E-steps between two kernel rebuilds as ONE call (varGP utils.py:1864-1934 in the truncated and sparse regimes):
 * n_steps x (gpfit_estep_projected with its moments, then gpfit_fparam_lbfgs started at the logA in force), everything
 * enqueued on `stream`, one synchronisation at the end.  logA, lambda0 and the rate stay on the device between steps.
 * Fixed: a, aL, L, r, kv0 as in gpfit_estep_projected (kv0 is required here).  State, device, in/out: m [nb], f [N]
 * (updated in place: each step's first kernel consumes both before anything of that step writes them).  Outputs, device:
 * V[nb][ldv], lam_m [N], lam_var [N] of the last step that ran.  By value: logA0, lambda0_mode / lambda0_fixed and the
 * optimiser's max_iter, history_size, lr, tol_grad, tol_change as in gpfit_fparam_lbfgs;
 * 1 <= n_steps <= GPFIT_ESTEP_CHAIN_MAX_STEPS.
 * rec_host[n_steps][12], one record per step: [0..8] out_host of gpfit_fparam_lbfgs, [9] LAPACK info of W = I + L^T G L,
 * [10] 1 when the step ran and its results were committed, 0 when it was skipped or its factorisation failed,
 * [11] the A = exp(logA) its Newton update used (exp of the device; gpfit_estep_projected takes the host's).  At equal
 * A a step gives the bits of the two calls it stands for.
 * With lambda0_mode = 1 a step is still exactly those two calls: the rate it leaves in f, which the next step's update
 * reads, is the one gpfit_fparam_lbfgs writes, at the closed-form lambda0 of the final logA and not at lambda0_fixed.
 * varGP with f_params carrying loglambda0 evaluates the rate at the fixed lambda0 before every update
 * (utils.py:1877 -> :1136): such a caller keeps its host loop.
 * A step whose W is not positive definite (info != 0) commits nothing; a step whose optimiser fails (status != 0) has
 * committed m, V and the moments, and leaves f, logA and lambda0 alone.  After either, no later step changes m, V, f,
 * lam_m, lam_var, logA or lambda0, and its record is all zero.
 * There is one implementation for this call and gpfit_estep_chain_batch: the single call is the group of one.
 * Returns 0 when the chain ran, whatever the records say; < 0 on bad arguments or insufficient capacity. */
#define GPFIT_ESTEP_CHAIN_MAX_STEPS 1024
int gpfit_estep_chain(gpfit_ctx* ctx, void* stream, const double* a, int64_t lda, const double* aL, int64_t ldal,
                      const double* L, int64_t ldl, int64_t N, int64_t nb, const double* r, const double* kv0,
                      double* m, double* f, double* V, int64_t ldv, double* lam_m, double* lam_var, double logA0,
                      int lambda0_mode, double lambda0_fixed, int n_steps, int max_iter, int history_size, double lr,
                      double tol_grad, double tol_change, double* rec_host);

/* The same chain in the full-rank regime (inducing set = training set, every eigenvalue kept, identity basis: varGP
 * utils.py:1864-1934 with a = B = I): n_steps x (the update of gpfit_estep in the original basis, the moments
 * lam_m = m_new, lam_var = kv0 + diag(V_new), then gpfit_fparam_lbfgs started at the logA in force), everything enqueued
 * on `stream`, one synchronisation at the end.  logA, lambda0 and the rate stay on the device between steps.
 * Fixed: K[N][ldk] symmetric (full) as in gpfit_estep, r [N], kv0 [N] = Kvec - diag(K~) (the caller's).  State, device,
 * in/out: m [N], f [N] (updated in place: each step's first kernel consumes both before anything of that step writes
 * them).  Outputs, device: V[N][ldv] (full, symmetric), lam_m [N], lam_var [N] of the last step that committed.  By
 * value: logA0, lambda0_mode / lambda0_fixed and the optimiser's settings as in gpfit_fparam_lbfgs;
 * 1 <= n_steps <= GPFIT_ESTEP_CHAIN_MAX_STEPS.
 * rec_host[n_steps][12]: the records of gpfit_estep_chain, slot for slot; [9] is the LAPACK info of M = I + S K S,
 * [11] the A = exp(logA) the device used (gpfit_estep takes the host's).  At equal A a step gives the bits of the calls
 * it stands for: gpfit_estep, (Kvec - diag K~) + diag V, gpfit_fparam_lbfgs.
 * lambda0_mode = 1 means what it means in gpfit_estep_chain, with the same caveat: a caller whose f_params carry
 * loglambda0 keeps its host loop.
 * A step whose M is not positive definite (info != 0) commits nothing; a step whose optimiser fails (status != 0) has
 * committed m, V and the moments, and leaves f, logA and lambda0 alone.  After either, no later step changes m, V, f,
 * lam_m, lam_var, logA or lambda0, and its record is all zero.
 * There is one implementation for this call and gpfit_estep_chain_full_batch: the single call is the group of one.
 * Returns 0 when the chain ran, whatever the records say; -3, with nothing enqueued, on a bad argument, n_steps outside
 * its range or round_up(N, 128) above the context's capacity. */
int gpfit_estep_chain_full(gpfit_ctx* ctx, void* stream, const double* K, int64_t ldk, int64_t N, const double* r,
                           const double* kv0, double* m, double* f, double* V, int64_t ldv, double* lam_m,
                           double* lam_var, double logA0, int lambda0_mode, double lambda0_fixed, int n_steps,
                           int max_iter, int history_size, double lr, double tol_grad, double tol_change,
                           double* rec_host);

/* gpfit_estep_chain for 1 .. GPFIT_ESTEP_CHAIN_MAX_UNITS independent units (cells, restarts of one cell) as ONE call:
 * unit u runs on its own context ctxs[u] (pairwise distinct, one device) with its own a[u], aL[u], L[u], r[u], kv0[u],
 * m[u], f[u], V[u], lam_m[u], lam_var[u], leading dimensions lda[u], ldal[u], ldl[u], ldv[u], size nb[u] and start
 * logA0[u] / lambda0_fixed[u] (read when lambda0_mode is 1); N, n_steps, lambda0_mode and the optimiser's settings are
 * shared.  Everything is enqueued on `stream`, one synchronisation at the end.  The factorisations of the units run in
 * lock step and every small kernel of a step is one launch for the group, so a step costs the launches of one unit.
 * All units of a call must have the same round_up(nb[u], 128) (nb[u] itself may differ): the recursion's split depends
 * on the padded size; otherwise -3 -- the caller groups its units by padded size.
 * rec_host[n_units][n_steps][12]: the records of gpfit_estep_chain, unit by unit.  Every output and record of unit u has
 * the bits it has when that unit is called alone (gpfit_estep_chain is this call with one unit); a unit that stops (W not positive definite, optimiser
 * failure) stops alone, exactly as there, and changes nothing in the others.
 * Returns 0 when the chains ran, whatever the records say; < 0 on bad arguments (nothing is enqueued then). */
#define GPFIT_ESTEP_CHAIN_MAX_UNITS 16
int gpfit_estep_chain_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* const* a,
                            const int64_t* lda, const double* const* aL, const int64_t* ldal, const double* const* L,
                            const int64_t* ldl, int64_t N, const int64_t* nb, const double* const* r,
                            const double* const* kv0, double* const* m, double* const* f, double* const* V,
                            const int64_t* ldv, double* const* lam_m, double* const* lam_var, const double* logA0,
                            int lambda0_mode, const double* lambda0_fixed, int n_steps, int max_iter, int history_size,
                            double lr, double tol_grad, double tol_change, double* rec_host);

/* The damped E-steps between two kernel rebuilds as ONE call (varGP with fit_parameters['estep_alpha'] != 1), for one
 * unit and for 1 .. GPFIT_ESTEP_CHAIN_MAX_UNITS units in lock step: n_steps x (the update of
 * gpfit_estep_projected_damped, the moments of lambda at the committed (m, V), then gpfit_fparam_lbfgs started at the
 * logA in force), everything enqueued on `stream`, one synchronisation at the end.
 * Operands per unit: those of gpfit_estep_chain (gpfit_estep_chain_batch) plus Linv[nb][ldli] = L^-1 (its lower triangle
 * is read).  alpha in (0, 1] is shared by the call (the blend of W_a rides on a product's scalars).  V[nb][ldv] is
 * in/out here: step 0 reads the caller's V (symmetric; its lower triangle is read), step k what step k - 1 committed.
 * A = exp(logA) of a step is formed on the device, as in the other chains.  All units of a call share N,
 * round_up(nb, 128), n_steps, alpha, lambda0_mode and the optimiser's settings.
 * A step: W1 = I + Y^T Y and P = L^-1 V L^-T are factored in one lock-step recursion (two chains per unit);
 * m_new = (1 - alpha) m + alpha L W1^-1 aL^T u; W_a = (1 - alpha) P^-1 + alpha W1 and its factorisation;
 * V_new = (L L_Wa^-T)(L L_Wa^-T)^T.  Behind the commit: lam_var = kv0 + rowsum((aL L_Wa^-T)^2), lam_m = a m_new.
 * V not positive definite (P's factorisation fails while W1's does not) is answered on the device, as varGP's host loop
 * answers it: that one update is the full Newton step -- the mean is not blended, W_a is W1 -- and the step commits the
 * full step's m and V.  Nothing of the failed factorisation reaches them, and nothing in the other units of a group
 * depends on it.
 * rec_host[n_units][n_steps][12]: the records of gpfit_estep_chain, slot for slot, except that [10] reads 2 for a step
 * committed as the full step because V was not positive definite (1: committed as the damped step; 0: skipped, or its
 * factorisation failed).  [9] is the LAPACK info of W1, or of W_a when W1's was 0.  A step with [9] != 0 commits
 * nothing and stops its unit exactly as in gpfit_estep_chain; so does a failing optimiser, behind the commit of m, V
 * and the moments.  Every output and record of a unit has the same bits alone and in any group; at equal A a step's
 * (m, V) have the bits of gpfit_estep_projected_damped, its slots 0-8 and rate those of gpfit_fparam_lbfgs on its moments.
 * No work matrix is added to the context; a cached factor of V in it is invalidated.
 * Returns 0 when the chains ran, whatever the records say; -3, with nothing enqueued and nothing written, for every
 * refusal of gpfit_estep_chain / _batch, a null Linv, ldli < nb, alpha not finite or outside (0, 1], or units of
 * different round_up(nb, 128). */
int gpfit_estep_chain_damped(gpfit_ctx* ctx, void* stream, const double* a, int64_t lda, const double* aL, int64_t ldal,
                             const double* L, int64_t ldl, const double* Linv, int64_t ldli, int64_t N, int64_t nb,
                             const double* r, const double* kv0, double* m, double* f, double* V, int64_t ldv,
                             double* lam_m, double* lam_var, double logA0, double alpha, int lambda0_mode,
                             double lambda0_fixed, int n_steps, int max_iter, int history_size, double lr,
                             double tol_grad, double tol_change, double* rec_host);
int gpfit_estep_chain_damped_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* const* a,
                                   const int64_t* lda, const double* const* aL, const int64_t* ldal,
                                   const double* const* L, const int64_t* ldl, const double* const* Linv,
                                   const int64_t* ldli, int64_t N, const int64_t* nb, const double* const* r,
                                   const double* const* kv0, double* const* m, double* const* f, double* const* V,
                                   const int64_t* ldv, double* const* lam_m, double* const* lam_var,
                                   const double* logA0, double alpha, int lambda0_mode, const double* lambda0_fixed,
                                   int n_steps, int max_iter, int history_size, double lr, double tol_grad,
                                   double tol_change, double* rec_host);

/* gpfit_estep_chain_full for 1 .. GPFIT_ESTEP_CHAIN_FULL_MAX_UNITS independent units (cells, restarts of one cell) as ONE
 * call: unit u runs on its own context ctxs[u] (pairwise distinct, one device) with its own K[u], r[u], kv0[u], m[u],
 * f[u], V[u], lam_m[u], lam_var[u], leading dimensions ldk[u], ldv[u] and start logA0[u] / lambda0_fixed[u] (read when
 * lambda0_mode is 1); N, n_steps, lambda0_mode and the optimiser's settings are shared.  Everything is enqueued on
 * `stream`, one synchronisation at the end.  The factorisations of the units run in lock step, every product of a step
 * is one call on the list of units and every small kernel one launch for the group, so a step costs the launches of one
 * unit.
 * rec_host[n_units][n_steps][12]: the records of gpfit_estep_chain_full, unit by unit.  Every output and record of unit
 * u has the bits it has when that unit is called alone (gpfit_estep_chain_full is this call with one unit); a unit that
 * stops (M not positive definite, optimiser failure) stops alone, exactly as there, and changes nothing in the others.
 * Returns 0 when the chains ran, whatever the records say; -3, with nothing enqueued and nothing written, for n_units or
 * n_steps outside their ranges, a null pointer, ldk[u] < N or ldv[u] < N, contexts on different devices, the same
 * context twice, a context with a pending asynchronous evaluation, or round_up(N, 128) above a context's capacity. */
#define GPFIT_ESTEP_CHAIN_FULL_MAX_UNITS 16
int gpfit_estep_chain_full_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* const* K,
                                 const int64_t* ldk, int64_t N, const double* const* r, const double* const* kv0,
                                 double* const* m, double* const* f, double* const* V, const int64_t* ldv,
                                 double* const* lam_m, double* const* lam_var, const double* logA0, int lambda0_mode,
                                 const double* lambda0_fixed, int n_steps, int max_iter, int history_size, double lr,
                                 double tol_grad, double tol_change, double* rec_host);

/* The tracked loss of an EM iteration (varGP utils.py:1958-1962): compute_loglikelihood (utils.py:1243) and
 * compute_KL_div (utils.py:1318-1326) of a posterior (m, V) under K~ as ONE call with one synchronisation.
 *   loglik = A r.lam_m + lambda0 sum r - sum f                                              A = exp(logA)
 *   KL     = -1/2 log|V| + 1/2 log|K~| + 1/2 m^T (K~^-1 m) + 1/2 sum_ij V_ij K~^-1_ij        (no -n/2 term, :1326)
 * tr(V K~^-1) is that elementwise sum because both matrices are symmetric: one pass over the nb^2 elements in place of
 * the nb^3 product of :1318, with m^T K~^-1 m in the same pass.  V is factored for its log-determinant; so is K~,
 * beside it in the same lock-step recursion, unless the caller knows log|K~| (logdet_K_known != 0: logdet_K is taken
 * as it is and K may be NULL).  No inverse factor is formed.
 * Device: m [nb]; V [nb][ldv], K [nb][ldk] (lower triangles read), Kinv [nb][ldki] = the caller's K~^-1, symmetric (the
 * call does not derive it from a factor) -- V and Kinv are read where they are, no padded copy is made; r, f (the
 * caller's rate vector), lam_m [N].  N is not bounded by the context's capacity; round_up(nb, 128) is.
 * out_host[10]: loglik, KL, loglik - KL, log|V|, log|K~|, m^T K~^-1 m, tr(V K~^-1), r.lam_m, sum r, sum f.
 * info_host[2]: LAPACK info of V, of K~ (0 when logdet_K_known).  A V that is not positive definite leaves NaN in
 * slots 1-4, a K~ that is not in slots 1, 2 and 4; loglik and slots 5-9 stay valid.
 * Every sum is formed from per-workgroup partials added in index order (no atomics): the same bits on every run.
 * Runs on the caller's stream, allocates nothing, uses the V work matrices (a cached V factor is dropped).
 * Returns 0, or the positive info of the failed factorisation (V's first; gpfit_last_error() names the matrix).
 * -3, with nothing enqueued and nothing written (before any context is read): a null pointer, N or nb <= 0, a leading
 * dimension < nb, K NULL while logdet_K_known is 0; then: a pending asynchronous evaluation, round_up(nb, 128) above
 * the context's capacity. */
int gpfit_elbo(gpfit_ctx* ctx, void* stream, const double* m, const double* V, int64_t ldv, const double* K, int64_t ldk,
               const double* Kinv, int64_t ldki, int64_t nb, int logdet_K_known, double logdet_K, const double* r,
               const double* f, const double* lam_m, int64_t N, double logA, double lambda0, double* out_host,
               int* info_host);
/* gpfit_elbo for 1 .. GPFIT_ELBO_MAX_UNITS independent units (cells, restarts of one cell) as ONE call: unit u runs on
 * its own context ctxs[u] (pairwise distinct, one device) with its own m[u], V[u], K[u], Kinv[u], r[u], f[u], lam_m[u],
 * leading dimensions, size nb[u], logdet_K_known[u] / logdet_K[u], logA[u] and lambda0[u]; N is shared.  The tables K
 * and ldk may be NULL when every unit knows its log|K~|.  Two chains per unit at most, all in one lock-step recursion;
 * every other stage is one launch for the group.  All units must have the same round_up(nb[u], 128) (nb[u] itself may
 * differ): the recursion's split depends on the padded size.
 * out_host[n_units][10], info_host[n_units][2]: as gpfit_elbo, unit by unit.  Every output of unit u has the bits it has
 * when that unit is called alone (gpfit_elbo is this call with one unit), whatever the other units, their number and
 * their nb; a unit whose factorisation fails stops alone.
 * Returns 0 when the call ran, whatever the info words say; -3, with nothing enqueued and nothing written: n_units
 * outside 1 .. 16, what gpfit_elbo refuses, different padded sizes, contexts on different devices, the same context
 * twice. */
#define GPFIT_ELBO_MAX_UNITS 16
int gpfit_elbo_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* const* m, const double* const* V,
                     const int64_t* ldv, const double* const* K, const int64_t* ldk, const double* const* Kinv,
                     const int64_t* ldki, const int64_t* nb, const int* logdet_K_known, const double* logdet_K,
                     const double* const* r, const double* const* f, const double* const* lam_m, int64_t N,
                     const double* logA, const double* lambda0, double* out_host, int* info_host);

/* The sweeps of a basis rebuild (eigtop.top_eigenpairs: the inner loop of a pass and the inputs of its Rayleigh-Ritz
 * step) as ONE call, for 1 .. GPFIT_ESTEP_CHAIN_MAX_UNITS independent units: unit u runs on its own context ctxs[u]
 * (pairwise distinct, one device) with its own K[u], Q[u], Y[u], W[u], S[u], step count m[u] and shifts sigma[u]; N, k,
 * ldk and the flags are shared.  Everything is enqueued on `stream`, one synchronisation at the end.
 * Device: K[u][N][ldk] symmetric (full); Q[u][N][k] in / out (the block, contiguous); Y[u], W[u] [N][k] caller-owned
 * work blocks (contiguous, distinct from Q[u] and from each other); S[u][k][k] out (read only with WANT_RR; S may be
 * NULL without it).  Host: m[u] >= 0 and sigma[u][0 .. m[u]) (sigma[u] may be NULL when m[u] is 0).
 * N and k multiples of 16, 16 <= k <= N, round_up(k, 128) within every context's capacity.
 * Step j of unit u (j < m[u]):
 *   Y = K Q                       skipped when j == 0 and GPFIT_SWEEPS_Y_READY is set: Y[u] already holds K Q
 *   Y -= sigma[u][j] Q            when sigma[u][j] != 0
 *   G = Y^T Y, G = (G + G^T) / 2, G = L L^T with L^-1 (the factorisation of gpfit_potrf), Y <- Y L^-T: once, and a
 *   second time on the unit's last step; then Q <- Y.
 * Tail (GPFIT_SWEEPS_WANT_RR): Y = K Q, S = Q^T Y, S = (S + S^T) / 2, left in Y[u] and S[u].  Without the flag the
 * contents of Y[u] are unspecified on return; W[u] always is.
 * Every product is the launch gpfit_dgemm makes of it and the factorisation is gpfit_potrf's, so Q, Y and S have the bits
 * of that host loop, and a unit has the same bits alone and in any group.  The factorisations of a round run in lock
 * step, every product of a step is one call on the list of the units that still have that step.
 * rec_host[n_units][2]: {step, info}.  info = 0: every step ran, step = m[u].  Otherwise info is the LAPACK info of the
 * first Gram matrix that was not positive definite and step the step it belongs to, counted from 1 (step - 1 steps were
 * completed); nothing of the failed step or of a later one is written to Q[u], which then holds the block it came with or
 * the block its completed steps left, and Y[u], S[u] are unspecified.  A unit that fails fails alone: the others finish
 * with the bits they have without it.
 * gpfit_subspace_sweeps is the batch call with one unit.
 * Returns 0 when the sweeps ran, whatever rec_host says; -3, with nothing enqueued, on a bad argument. */
#define GPFIT_SWEEPS_Y_READY 1
#define GPFIT_SWEEPS_WANT_RR 2
#define GPFIT_SUBSPACE_SWEEPS_MAX_STEPS 1024
int gpfit_subspace_sweeps(gpfit_ctx* ctx, void* stream, const double* K, int64_t ldk, int64_t N, int64_t k, double* Q,
                          double* Y, double* W, double* S, int m, const double* sigma, int flags, int* rec_host);
int gpfit_subspace_sweeps_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* const* K, int64_t ldk,
                                int64_t N, int64_t k, double* const* Q, double* const* Y, double* const* W,
                                double* const* S, const int* m, const double* const* sigma, int flags, int* rec_host);

/* The projector step of a basis rebuild (eigtop._kept_subspace: the Cayley transform of the k x k Rayleigh quotient
 * matrix and a stretch of the scaled Newton-Schulz sign iteration) as ONE call, for 1 .. GPFIT_ESTEP_CHAIN_MAX_UNITS
 * independent units: unit u runs on its own context ctxs[u] (pairwise distinct, one device) with its own S[u], tau[u],
 * X[u], X2[u], W[u]; k, the flags and the schedule -- n_steps, c[0 .. n_steps), its0 -- are shared.  Everything is
 * enqueued on `stream`, one synchronisation at the end.
 * Device: S[u][k][k] symmetric, read only (only read with GPFIT_SIGN_CAYLEY; S and tau may be NULL without it);
 * X[u], X2[u], W[u] [k][k] caller-owned blocks (contiguous, pairwise distinct).  Host: tau[u], c.
 * k a multiple of 16, 16 <= k, round_up(k, 128) within every context's capacity; 0 <= n_steps <= GPFIT_SIGN_MAX_STEPS.
 * Head (GPFIT_SIGN_CAYLEY): S + tau I = L L^T with L^-1 (the factorisation of gpfit_potrf: the lower triangle of S, the
 *   diagonal with one rounded add), Sinv = L^-T L^-1, X = (S - tau I) Sinv, X = (X + X^T) / 2, left in X[u].  Without
 *   the flag X[u] is the caller's.
 * Step j (j < n_steps):
 *   X2 = X X                      skipped when j == 0 and GPFIT_SIGN_X2_READY is set: X2[u] already holds X X
 *   Xn <- X; Xn = -0.5 c[j]^3 X X2 + 1.5 c[j] Xn (one product with a beta); X <- Xn
 *   X = (X + X^T) / 2             when ((its0 + j) & 7) == 7
 * Tail: X2 = X X, the product a convergence test reads and the first product of a next step.
 * X[u] and W[u] change places with every step and nothing is copied back: on return X stands in X[u] when n_steps is
 * even and in W[u] when it is odd; the other of the two is unspecified.  X2 stands in X2[u].
 * Every product is the launch gpfit_dgemm makes of it and the factorisation is gpfit_potrf's, so X and X2 have the bits
 * of that host loop, and a unit has the same bits alone and in any group.
 * rec_host[n_units][2]: {steps, info}.  info = 0: steps = n_steps.  Otherwise info is the LAPACK info of S + tau I, which
 * was not positive definite, steps = 0, and X[u], X2[u], W[u] are unspecified.  A unit that fails fails alone: the others
 * finish with the bits they have without it.
 * gpfit_sign_steps is the batch call with one unit.
 * Returns 0 when the call ran, whatever rec_host says; -3, with nothing enqueued, on a bad argument (GPFIT_SIGN_X2_READY
 * together with GPFIT_SIGN_CAYLEY is one). */
#define GPFIT_SIGN_CAYLEY 1
#define GPFIT_SIGN_X2_READY 2
#define GPFIT_SIGN_MAX_STEPS 64
int gpfit_sign_steps(gpfit_ctx* ctx, void* stream, const double* S, int64_t k, double tau, double* X, double* X2, double* W,
                     int n_steps, const double* c, int its0, int flags, int* rec_host);
int gpfit_sign_steps_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* const* S, int64_t k,
                           const double* tau, double* const* X, double* const* X2, double* const* W, int n_steps,
                           const double* c, int its0, int flags, int* rec_host);

/* Active-learning utility of nstar candidate stimuli, U = H(r|x,D) - <H(r|f,x)>
 * (nd_utility with nd_p_r_given_xD, nd_lambda_r_mean, nd_mean_noise_entropy, utils.py:413-525;
 * call site one_cell_active_training.ipynb: u2d = nd_utility(logf_var, logf_mean, arange(100))).
 * sigma2, mu: device [nstar] (variance and mean of log f); r: device [nr] response counts;
 * U: device [nstar].  The principal-branch Lambert W (scipy on the host in the reference,
 * utils.py:464-466) is evaluated on the device.  Asynchronous on `stream`. */
int gpfit_nd_utility(void* stream, const double* sigma2, const double* mu, int64_t nstar, const double* r,
                     int nr, double* U);

/* Score a stimulus pool in one call: predictive moments of lambda (lambda_moments_star, utils.py:1476-1500), the
 * firing rate (utils.py:395) and the active-learning utility of P candidate images.  The posterior enters through
 * one vector and one symmetric matrix that the caller forms once per model (utils.fold_posterior):
 *     w   = K~_b^-1 m_b                               [k]
 *     S_b = K~_b^-1 (V_b - K~_b) K~_b^-1, symmetric   [k][k]   (only its lower triangle is read)
 * and per pool row i, with z_i = k*_i B (k*_i when B is NULL: the identity basis, k == nt),
 *     mu_i     = z_i . w
 *     sigma2_i = k**_i + z_i S_b z_i^T            (not clamped; the reference does not clamp it either)
 *     rate_i   = exp(A mu_i + A^2 sigma2_i / 2 + lambda0)
 *     U_i      = the utility of gpfit_nd_utility at (A^2 sigma2_i, A mu_i + lambda0)   (the same kernel, the same bits)
 * which is the reference's formula with the products re-associated: one triangular P x k x k product instead of two
 * dense ones, and no P x k result ever written.
 *   xstar   device [P][ldxs]: already masked (pixels == NULL, d columns) or whole images of d_full pixels of which
 *           the d columns listed in `pixels` (device int [d], ascending as a mask gives them) are gathered
 *   xtilde  device [nt][ldxt], masked inducing images;  C device [d][ldc];  B device [nt][ldb] or NULL
 *   S, w    device, as above;  r device [nr] response counts, or NULL: no utility, U is not touched
 *   mu, sigma2, rate, U   device [P]; rate and U may be NULL
 * The pool is walked in row chunks of min(chunk_rows, capacity) rows (chunk_rows 0: the context's capacity, else a
 * multiple of 128) inside the context's workspace: nothing is allocated, nt, k and d must fit the context (-3
 * otherwise).  Every sum of a row runs over the same terms in the same order wherever the row sits (the dense products
 * of a chunk are launched so that none is cut along k, at any size): results do not depend on the chunking, on the
 * context's capacity, on a row's position in the pool or on the run.  Asynchronous on `stream`; P == 0 returns at once. */
int gpfit_score_pool(gpfit_ctx* ctx, void* stream, double sigma0, const double* xstar, int64_t ldxs, int64_t P,
                     const int* pixels, int64_t d_full, const double* xtilde, int64_t ldxt, int64_t nt, int64_t d,
                     const double* C, int64_t ldc, const double* B, int64_t ldb, int64_t k, const double* S,
                     int64_t lds, const double* w, double A, double lambda0, const double* r, int nr,
                     int64_t chunk_rows, double* mu, double* sigma2, double* rate, double* U);

/* gpfit_score_pool for 1 .. GPFIT_ESTEP_CHAIN_MAX_UNITS independent units (the cells of a population, which all see
 * the same candidate images) as ONE call: unit u runs on its own context ctxs[u] (pairwise distinct, one device) in that
 * context's workspace, and every launch of the call -- the three dense products as pointer batches of n_units problems,
 * the Gram, weights, quadratic-form, finish and utility kernels with a unit index -- carries all units, so the number of
 * launches does not grow with n_units (gpfit_score_pool is this call with one unit).  Per unit, tables indexed by u:
 *   sigma0[u]; xstar[u] with ldxs[u], pixels[u] (the table or an entry may be NULL: that unit's xstar is already masked)
 *   and d_full[u] -- in a population every xstar[u] is the same pool of whole images and only the pixel lists differ;
 *   xtilde[u], ldxt[u], nt[u], d[u];  C[u], ldc[u];  B[u], ldb[u] (B may be NULL: no unit has a basis);  k[u];
 *   S[u], lds[u];  w[u];  A[u], lambda0[u];  the outputs mu[u], sigma2[u], rate[u] (table or entry may be NULL), U[u],
 *   device [P] each.
 * Shared by the call: P, the response counts r / nr (NULL: no utility, no U[u] is touched) and chunk_rows; the chunk is
 * min(chunk_rows or capacity, the smallest capacity among the units' contexts) rows.
 * What lets the units share launches: round_up(d, 32), round_up(nt, 128) and round_up(k, 128) agree, and all units have
 * a basis B or none has; the true d, nt and k may differ.  A disagreement is refused (-3, "unit u: ...", nothing
 * written), as is a unit whose context is too small, repeated, on another device, or has an evaluation pending.
 * For every unit mu, sigma2, rate and U are bit-identical to gpfit_score_pool on that unit's arguments alone, whatever
 * the other units, their number and order, chunk_rows and the contexts' capacities.  No atomics, nothing allocated.
 * Asynchronous on `stream`; P == 0 returns at once. */
int gpfit_score_pool_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* sigma0,
                           const double* const* xstar, const int64_t* ldxs, int64_t P, const int* const* pixels,
                           const int64_t* d_full, const double* const* xtilde, const int64_t* ldxt, const int64_t* nt,
                           const int64_t* d, const double* const* C, const int64_t* ldc, const double* const* B,
                           const int64_t* ldb, const int64_t* k, const double* const* S, const int64_t* lds,
                           const double* const* w, const double* A, const double* lambda0, const double* r, int nr,
                           int64_t chunk_rows, double* const* mu, double* const* sigma2, double* const* rate,
                           double* const* U);

/* The utility of a population: out[i] = sum over rows u of weight[u] * U[u][i], i < P, for U device [n_rows][ldu]
 * (ldu >= P; the rows of utilities that gpfit_score_pool / gpfit_score_pool_batch wrote), weight device [n_rows] or NULL
 * (every weight one), out device [P].  The rows are added in ascending order starting from the first product, with one
 * rounding per multiply and per add (no fused multiply-add): the bits of the loop acc = weight[0] U[0];
 * acc = acc + weight[u] U[u], whatever calls produced the rows.  NaN propagates, nothing is masked; n_rows >= 1 is not
 * limited by GPFIT_ESTEP_CHAIN_MAX_UNITS.  Asynchronous on `stream`; P == 0 returns at once. */
int gpfit_utility_sum(void* stream, const double* U, int64_t ldu, int n_rows, const double* weight, int64_t P, double* out);

/* Posterior covariance of the latents of a shortlist of M candidate images: with the operands of gpfit_score_pool (same
 * meaning: masked rows or whole images with `pixels`, B == NULL for the identity basis, only the lower triangle of S read)
 *     Sigma[i][j] = k(x_i, x_j) + z_i S_b z_j^T   (i != j),   z_i = k*_i B,  k the arc-cosine kernel of gpfit_acosker
 *     Sigma[i][i] = the sigma2_i that gpfit_score_pool writes for the same row, bit for bit (its k**_i + z_i S_b z_i^T
 *                   form, not the "- 1e-7" diagonal of the off-diagonal formula)
 * into Sigma, device [M][ldsig] (ldsig >= M) owned by the caller.  One triangle of tiles is computed and mirrored on the
 * way out: Sigma[i][j] and Sigma[j][i] have the same bits.  The dense products (x* C, K* B, W = Z S_b, W Z^T) go out as
 * pointer batches as in the pool call, so none is cut along k: the bits of an element depend on its two rows and on
 * which of them comes first, not on the context's capacity, on M or on where the rows sit in the shortlist.
 * M, nt, k (rounded up to 128) and d must fit the context (-3 otherwise, "problem larger than the context capacity",
 * nothing written); the whole shortlist is one chunk of the workspace.  Nothing is allocated, no atomics.  Asynchronous on
 * `stream`; M == 0 returns at once. */
int gpfit_pool_covariance(gpfit_ctx* ctx, void* stream, double sigma0, const double* xstar, int64_t ldxs, int64_t M,
                          const int* pixels, int64_t d_full, const double* xtilde, int64_t ldxt, int64_t nt, int64_t d,
                          const double* C, int64_t ldc, const double* B, int64_t ldb, int64_t k, const double* S,
                          int64_t lds, double* Sigma, int64_t ldsig);

/* Pick the n_select images of a round one by one, each conditioned on those already chosen, for 1 .. 16 units (cells)
 * that see the same M candidates.  One more presentation of image i adds A^2 f_i a_i a_i^T to the posterior precision
 * (the E-step's Newton term) and, at the expected response r_i = f_i, leaves the mean where it is: a rank-1 Gaussian
 * conditioning of the latents with pseudo-noise tau_i = 1 / (A^2 f_i).  Step t = 0 .. n_select - 1:
 *   1. U_u[j] = the utility of gpfit_nd_utility at (A_u^2 s_u[j], A_u mu_u[j] + lambda0_u) with s_u the current
 *      conditional variances (the same device code, the arguments rounded as gpfit_score_pool rounds them), and
 *      T[j] = sum_u weight[u] U_u[j] in the order and rounding of gpfit_utility_sum (one unit, no weights: T = U).
 *   2. i = the lowest index among the rows not yet chosen whose T[j] is finite and maximal; picked[t] = i,
 *      utility[t] = T[i].  If no row qualifies, this and every later step write -1 and NaN and do nothing else.
 *   3. per unit: tau = 1 / (A^2 exp(A mu_i + A^2 s_i / 2 + lambda0)), v = s_i + tau,
 *      c_j = Sigma[j][i] - sum_{q<t} G[q][j] G[q][i],  G[t][j] = c_j / sqrt(v),  s_j -= G[t][j]^2  (chosen rows too).
 * With n_select == 1 the call is the argmax of gpfit_score_pool's utility.  The conditional variances are those of exact
 * Gaussian conditioning on the chosen rows with noise diag(tau).
 *   Sigma[u]  device [M][ldsig[u]], symmetric (gpfit_pool_covariance);  mu[u] device [M]
 *   A, lambda0, weight   HOST [n_units]; weight may be NULL (every weight one)
 *   r   device [nr] response counts
 *   work[u]         device [n_select][M]: the factor rows G on return; its prior content is irrelevant
 *   sigma2_cond[u]  device [M]: written by the call -- it starts as the diagonal of Sigma[u] and ends as the
 *                   conditional variances given all picks
 *   picked (int), utility   device [n_select]
 * 2 n_select + 1 small launches ordered by the stream alone: no cooperative launch, no grid-wide barrier, no spin-wait,
 * no atomic, no host synchronisation, nothing allocated; every sum is reduced in a fixed order (bit-reproducible).
 * Refused (-3, nothing written): n_units outside 1 .. 16, n_select outside 1 .. GPFIT_SELECT_MAX, M < 1, null
 * pointers, ldsig[u] < M.  Takes no context.  Asynchronous on `stream`. */
#define GPFIT_SELECT_MAX 128      /* = the block of one gpfit_potrf_append_block step */
int gpfit_select_batch(void* stream, int n_units, const double* const* Sigma, const int64_t* ldsig, int64_t M,
                       const double* const* mu, const double* A, const double* lambda0, const double* weight,
                       const double* r, int nr, int n_select, double* const* work, double* const* sigma2_cond,
                       int* picked, double* utility);

/* Per-launch HIP-event timing of the dominant kernels during gpfit_fit_eval (bench.py's
 * roofline leg; adds two event records per launch, so leave it off when timing throughput).
 * out16: 0 sum of the 128-tile GEMM launch durations [ms] (the dominant kernel family, stream-K
 *        variant included), 1 flops those launches executed, 2 #launches, 3 sum of Cholesky-leaf
 *        durations [ms], 4 #leaves, 5 Gram kernel [ms], 6 its flops, 7 #, 8-10 the same three
 *        figures for the 64/32-tile instances, 11-12 duration [ms] and flops of the single largest
 *        GEMM launch (L^-1 L_V at the headline), 13-15 unused. */
int gpfit_set_profile(gpfit_ctx* ctx, int on);
int gpfit_get_profile(gpfit_ctx* ctx, double* out16);
/* Phase timing (gpfit_set_profile(ctx, 2)): eight HIP events per evaluation and none inside the
 * factorisations, so the timed run is the production schedule.  out8[i] = milliseconds from the start
 * of the last synchronous gpfit_fit_eval (with gradients) to: 0 start, 1 kernel build + moments done
 * (the two factorisation chains start here), 2 Cholesky + inverse of K~ done (main stream), 3 Cholesky
 * of V done (auxiliary stream), 4 T = L^-1 L_V and its norm done, 5 Q = I - T T^T done, 6 two-sided
 * product W done, 7 end (gradient contraction, scalars copied). */
int gpfit_get_phases(gpfit_ctx* ctx, double* out8);
/* Host milliseconds the last gpfit_fit_eval spent enqueuing work (before its final sync). */
double gpfit_last_enqueue_ms(gpfit_ctx* ctx);

/* fp32 instance of the fused unit of work (hyperparameter-grid configuration, BASELINE
 * configs[4]; the reference itself is fp64-only, utils.py:31-33): X, r, m, V and the optional
 * output vectors are float32 device buffers, every factorisation / GEMM runs in fp32 on
 * v_mfma_f32_16x16x4_f32, reductions and the returned scalars are fp64.  Same contract
 * otherwise.  Accuracy against the fp64 path is stated in tests/test_gpu_fp32.py. */
int gpfit_fit_eval_f32(gpfit_ctx* ctx, void* stream, const double* theta, const double* lower,
                       const double* upper, int n_rows, int n_cols, const float* X, int64_t ldx, int64_t N,
                       const float* r, const float* m, const float* V, int64_t ldv, double logA, double lambda0,
                       int want_grad, double* out_host, float* lam_m, float* lam_var, float* f);

/* Roofline probes (no reference counterpart): back-to-back v_mfma_f64_16x16x4_f64 issue
 * (flops = blocks*4 waves*iters*16*2048) and a 16-byte-per-lane stream copy. */
int gpfit_probe_mfma_f64(void* stream, double* scratch, int blocks, int iters);
int gpfit_probe_stream_copy(void* stream, const double* in, double* out, int64_t n_doubles);

/* ---- test hooks ----------------------------------------------------------------------
 * For the test-suite (tests/test_gemm_plans_cpu.py, tests/test_gpu_gemm_schedules.py, tests/test_gpu_potrf.py,
 * tests/test_gpu_elementwise.py), not for applications: the GEMM launcher with every field of its argument struct
 * exposed, host-only queries of what it would do with a launch, the Cholesky recursion and the element-wise launchers
 * on the caller's buffers.  They add no arithmetic of their own. */
typedef struct gpfit_dev_gemm_args {
  const void* A;            /* device operands of element type double (is_f32 = 0) or float (1) */
  const void* B;
  void* C;
  int64_t lda, ldb, ldc;
  int64_t sA, sB, sC;       /* strides (elements) of a strided batch; sC also separates the slabs of split_k */
  double alpha, beta;
  void* sk_ws;              /* caller-owned stream-K workspace, or NULL */
  void* aux;                /* epi 4 */
  double* sumsq;            /* epi 2 */
  const void* const* Ap;    /* nptr > 0: HOST arrays of nptr device pointers each (auxp, sumsqp may be NULL) */
  const void* const* Bp;
  void* const* Cp;
  void* const* auxp;
  double* const* sumsqp;
  int32_t M, N, K;
  int32_t a_kmajor, b_kmajor, out_lower, a_tri, b_tri;
  int32_t batch;            /* problems of a strided batch (0 or 1: one) */
  int32_t split_k;          /* > 1: k slabs, slab z written to C + z sC, beta ignored */
  int32_t tile;             /* 0 automatic, or 128 / 64 / 32 */
  int32_t walk;             /* as gpfit_dgemm_ex */
  int32_t epi;              /* fused epilogue: 0 none, 1 mirror, 2 tile norms, 4 dual update, 8 added matrix (aux read only) */
  int32_t nptr;             /* > 0: pointer batch of nptr problems (at most 32) */
  int32_t k_slabs;          /* > 0: the triangular-operand route (a_tri 2, M == K a multiple of 64): 64-tiles, k in
                             * at most k_slabs fixed slabs, one workgroup per (tile, slab) with a non-empty k range;
                             * slab z of a row panel written to C + z sC, beta ignored; the slabs below a panel's own
                             * k range are not written */
  int32_t b_split;          /* > 0 (a multiple of 128, b_tri 1): op(B) is dense left of this column and lower triangular
                             * from it on, the triangle's origin there; XCD-aware table only, whose tiles are those with
                             * a non-empty k range (the others stay unwritten) */
} gpfit_dev_gemm_args;

typedef struct gpfit_dev_gemm_route_t {
  int32_t rc;               /* 0, or -3: the launch would refuse its arguments (an epilogue it cannot carry, K not a
                             * multiple of the K step, lda / ldb not multiples of 16 bytes, lower with M != N, a pointer
                             * batch of more than 32 or with split_k; a pair that cannot share a launch) */
  int32_t tile;             /* block tile: 128 / 64 / 32 */
  int32_t sk_first;         /* stream-K: -1 not taken, 0 every tile, > 0 tiles of the data-parallel head */
  int32_t xcd;              /* 1: XCD-aware schedule table */
  int32_t stages;           /* LDS stages of the main loop: 2, deep pipeline 4 (64-tiles) / 8 (32-tiles) */
  int32_t half_occ;         /* 1: half-occupancy launch */
  int32_t edge;             /* 1: predicated (ragged) instance */
  int32_t epi;              /* fused epilogue the launch carries */
  int32_t sumsq_entries;    /* entries of sumsq an epi-2 launch writes (per problem) */
  int32_t blocks;           /* workgroups of the (main) launch; pair: tiles of both members */
  int32_t pair;             /* pair query: 1 the two launches can share one */
  int32_t slabs;            /* k_slabs route: live slabs (0: not that route) */
} gpfit_dev_gemm_route_t;

/* What the launcher would do with these arguments (pair_args != NULL: with the two as one pair launch).  Host only,
 * no GPU call, pointers are not dereferenced.  0, or -3 for a malformed query. */
int gpfit_dev_gemm_route(int is_f32, const gpfit_dev_gemm_args* args, const gpfit_dev_gemm_args* pair_args,
                         gpfit_dev_gemm_route_t* out);
/* The plan of a balanced schedule, as the launcher would upload it.  Host only.  kind 2, stream-K:
 *   out[0..7] = first, ntiles, total k-steps, blocks, per_block, nfix, nslot, workspace slots available;
 *   then ntiles records (row0, col0, kbeg, ksteps, prefix) in walk order, fix_tile[nfix] (indices into the
 *   records), fix_ptr[nfix + 1], fix_slot[nslot].
 * kind 1, XCD-aware table: out[0] = length, then the table (ti << 16 | tj, -1 padding).
 * kind 4, the same table with each tile's k range: out[0] = length, then per entry (ti << 16 | tj or -1, kbeg, kend).
 * kind 3, slab plan of the k_slabs route: out[0..3] = items, live slabs, k per slab, tile; then per item in launch
 *   order (row panel, slab, kbeg, kend); every tile column of a panel runs the same items.
 * Returns the number of int32 the plan takes (nothing is written when that exceeds cap), -1 when the launch does
 * not take that schedule, -3 on a bad argument. */
int64_t gpfit_dev_gemm_plan(int is_f32, const gpfit_dev_gemm_args* args, int kind, int32_t* out, int64_t cap);
/* launch_gemm on these arguments, or launch_gemm_pair when pair_args is given.  Return value as gpfit_dgemm. */
int gpfit_dev_gemm(void* stream, int is_f32, const gpfit_dev_gemm_args* args, const gpfit_dev_gemm_args* pair_args);
/* A context's work buffer by its name in the sources -- every floating-point device work buffer of the context: the
 * matrices ("Abuf", "LVbuf", ...), the N x d and d x d blocks, the vectors, the partial arrays, "scal", and the two
 * stream-K workspaces "sk_ws[0]" and "sk_ws[1]"; not the integer buffers, the chain block or pinned host memory: copy
 * `bytes` bytes at byte `offset` to (to_ctx = 0) or from (1) the device pointer `dev`, or fill the whole buffer (the
 * size of its allocation) with one byte value.  Synchronous.  0, or -3 (also while an evaluation is pending). */
int gpfit_dev_ctx_copy(gpfit_ctx* ctx, const char* name, int64_t offset, void* dev, int64_t bytes, int to_ctx);
int gpfit_dev_ctx_fill(gpfit_ctx* ctx, const char* name, int byte);
/* The names those two calls know, by index from 0: writes the NUL-terminated name into out[cap] and returns 0; -3 past
 * the end of the table (or when the name does not fit).  Needs no context and no GPU. */
int gpfit_dev_ctx_buffer_name(int index, char* out, int cap);
/* The Cholesky recursion behind gpfit_potrf and every closure (tests/test_gpu_potrf.py), on the caller's own device
 * buffers: nb chains (1 .. 32) of n x n matrices, n a multiple of 128, element type double (is_f32 = 0) or float (1), all
 * with leading dimension ld (elements; >= n, a multiple of 16 bytes).  A, L, Li, Tmp, info: HOST arrays of nb DEVICE
 * pointers each (matrices of n x ld elements; info: one int per chain, zeroed by the caller).  Chain b factors the lower
 * triangle of A[b] (destroyed) into L[b]; Li[b] receives the inverse of the factor for the chains in the bit mask `need`,
 * the inverses of the two diagonal half blocks (without [L^-1]21) for the chains in `halves`, and for every other chain
 * the inverse of the top block (the first ceil(n / 256) * 128 rows; below it only the diagonal blocks the recursion
 * inverts for its own solves); Tmp[b] is scratch; info[b] receives the
 * LAPACK info (the first failing pivot wins; stays as it was on success).  side_min > 0: blocks of at least that size put
 * the first product of their inverse merge on the context's side stream (the caller's stream waits for it), 0: one
 * stream.  The call only enqueues.  0, or -3 for a refused argument (nothing has touched the device then). */
int gpfit_dev_potrf(gpfit_ctx* ctx, void* stream, int is_f32, int nb, void* const* A, void* const* L, void* const* Li,
                    void* const* Tmp, int* const* info, int64_t ld, int n, uint32_t need, uint32_t halves, int side_min);

/* The launchers of the element-wise and reduction kernels (elementwise.hip; tests/test_gpu_elementwise.py), each on the
 * caller's own device buffers.  One flat argument struct for all of them; the list below names, per op, what the slots
 * p[], ld[], n[] and s[] hold, in the order of the launcher's own arguments.  "(opt)" marks a pointer that may be NULL.
 * Element type: double, or float with is_f32 = 1 where the launcher is instantiated for it (marked f32); scratch and
 * reduction outputs named double below are double in both.
 *
 *   TRMV_LOWER    f32  p: L x y                      ld: ldl        n: np
 *   TRMV_LOWER_T  f32  p: L x z partial(double)      ld: ldl        n: np (a multiple of 64)
 *   SYMV_LOWER         p: A x y                      ld: lda        n: n
 *   GEMV_SUB      f32  p: M x y out                  ld: ldm        n: rows cols
 *   GEMV_T_SUB    f32  p: M x y out partial(double)  ld: ldm        n: rows cols
 *   DOT           f32  p: x y out(double)                           n: n
 *   LOGDET        f32  p: L out(double)              ld: ldl        n: n
 *   LOGDET_PAIR   f32  p: L0 out0 L1 out1            ld: ldl        n: n
 *   FROB_LOWER    f32  p: T out(double) partial      ld: ldt        n: np (a multiple of 128)
 *   FROB_TILES    f32  p: T partial(double)          ld: ldt        n: rows cols (multiples of 128) lower
 *   REDUCE_SLICES f32  p: src dst                    ld: stride count   n: nslice dst_f32 (1, with is_f32 = 0: double
 *                                                                       slices into a float dst)
 *   REDUCE_SLABS  f32  p: src dst                    ld: stride     n: nslab slab_rows rows cols
 *   REDUCE_SLICES_SYM f32  p: src dst                ld: stride     n: nslice n
 *   PACK_LOWER    f32  p: src dst                    ld: lds ldd    n: n np (a multiple of 128)
 *   PACK_TRI           p: src dst                    ld: lds ldd    n: n np
 *   UNPACK_SYM         p: src dst                    ld: lds ldd    n: n
 *   UNPACK_TRI         p: src dst                    ld: lds ldd    n: n
 *   SYMMETRIZE    f32  p: A                          ld: lda        n: n
 *   SYMMETRIZE_AVG     p: A                          ld: lda        n: n
 *   PAD_COPY           p: src dst                    ld: lds ldd    n: rows cols prow pcol
 *   GATHER        f32  p: X Xt pix(opt, int) Xm(opt) ld: ldx ldt ldm   n: n d dp np (dp, np multiples of 32)
 *   ESTEP_BUILD        p: K sv Mb SK Kl              ld: ldk ld     n: n np (a multiple of 128)
 *   ADD_DIAG      f32  p: A                          ld: lda        n: n            s: v
 *   AXPBY_BLOCK   f32  p: dst src                    ld: ldd lds    n: rows cols (even)   s: a b
 *   DEMOTE_BLOCK       p: src(double) dst(float)     ld: lds ldd    n: rows cols
 *   QVEC          f32  p: Xt XCt Kvec q              ld: ld         n: n np dp      s: s0sq
 *   MOMENTS       f32  p: Kvec q Cos V m r lam_m lam_var f wl scal(double) part(double) ticket(int)
 *                                                    ld: ldc ldv    n: n            s: A lambda0
 *   ADJOINT       f32  p: W Cos b q Aout upart vpart sumA_part (the last three double)
 *                                                    ld: ld         n: n np (a multiple of 64)
 *   ADJOINT_REDUCE f32 p: upart vpart sumA_part q wl tvec uq(double) scal_out(double)
 *                                                                   n: n np ntile ntile_tri
 *   ADJOINT_RECT       p: W Cos q1 q2 Aout upart vpart tile_sum t1 t2 uq1 uq2 scal3 extra1(opt)
 *                                                    ld: ldw ldc lda   n: n1 n2 np1 np2 (multiples of 64)
 *   METRIC_CONTRACT f32  p: pix(int) C M grad5(double) part(double) ticket(int)
 *                                                    ld: ldc ldm    n: d n_rows n_cols     theta
 *   DK_SIGMA0          p: Cos q1 q2 dK               ld: ldc ldk    n: n1 n2        s: s0
 *   DQ                 p: Xt XDt q dq(opt) h(opt)    ld: ld         n: n dp
 *   DK_METRIC          p: H Cos q1 q2 dq1 dq2        ld: ldh ldc    n: n1 n2
 *   ESTEP_PREP         p: f r m sv rhs                              n: n np         s: A
 *   ROWSCALE_ADD  f32  p: Y Xm t                     ld: ldy ldm    n: np dp        s: scale
 *
 * op + GPFIT_EW_GROUP is the unit-batched launcher of the same name (double only; TRMV_LOWER, TRMV_LOWER_T, SYMV_LOWER,
 * DOT, LOGDET_PAIR, REDUCE_SLICES, PACK_LOWER, PACK_TRI, SYMMETRIZE, SYMMETRIZE_AVG, PAD_COPY, GATHER, ADD_DIAG, QVEC) for
 * n_units units (1 .. 16).  The slots keep their meaning: up[k] is a HOST array of n_units DEVICE pointers in place of
 * p[k]; where the launcher takes an extent, a leading dimension or a scalar per unit, un[k] / uld[k] / us[k] is a HOST
 * array of n_units values in place of n[k] / ld[k] / s[k] (PACK_LOWER, PACK_TRI: n, lds; PAD_COPY: rows, cols, lds;
 * GATHER: n, d, ldx, and Xm is not written; QVEC: n, s0sq; SYMMETRIZE_AVG, LOGDET_PAIR: n); everything else is common
 * and comes from n[], ld[], s[].
 *
 * The hook fills the launcher's arguments and returns its return code; it adds no arithmetic.  theta: the launcher's
 * Theta as its eight doubles (sigma_0, eps_0x, eps_0y, -2log2beta, -log2rho2, Amp, exp(-2log2beta), exp(-log2rho2)).
 * -3 before any launch: an unknown op, an op without a float instance asked for one, a NULL among the pointers an op
 * requires, an extent below 1, n_units outside 1 .. 16, or an extent that breaks the multiple stated above.  The call
 * only enqueues. */
enum {
  GPFIT_EW_TRMV_LOWER = 0, GPFIT_EW_TRMV_LOWER_T, GPFIT_EW_SYMV_LOWER, GPFIT_EW_GEMV_SUB, GPFIT_EW_GEMV_T_SUB, GPFIT_EW_DOT,
  GPFIT_EW_LOGDET, GPFIT_EW_LOGDET_PAIR, GPFIT_EW_FROB_LOWER, GPFIT_EW_FROB_TILES, GPFIT_EW_REDUCE_SLICES,
  GPFIT_EW_REDUCE_SLABS, GPFIT_EW_REDUCE_SLICES_SYM, GPFIT_EW_PACK_LOWER, GPFIT_EW_PACK_TRI, GPFIT_EW_UNPACK_SYM,
  GPFIT_EW_UNPACK_TRI, GPFIT_EW_SYMMETRIZE, GPFIT_EW_SYMMETRIZE_AVG, GPFIT_EW_PAD_COPY, GPFIT_EW_GATHER,
  GPFIT_EW_ESTEP_BUILD, GPFIT_EW_ADD_DIAG, GPFIT_EW_AXPBY_BLOCK, GPFIT_EW_DEMOTE_BLOCK, GPFIT_EW_QVEC, GPFIT_EW_MOMENTS,
  GPFIT_EW_ADJOINT, GPFIT_EW_ADJOINT_REDUCE, GPFIT_EW_ADJOINT_RECT, GPFIT_EW_METRIC_CONTRACT, GPFIT_EW_DK_SIGMA0,
  GPFIT_EW_DQ, GPFIT_EW_DK_METRIC, GPFIT_EW_ESTEP_PREP, GPFIT_EW_ROWSCALE_ADD, GPFIT_EW_NOPS,
  GPFIT_EW_GROUP = 256
};
typedef struct gpfit_dev_ew_args {
  void* p[16];                /* device pointers */
  int64_t ld[4];              /* leading dimensions, strides, 64-bit counts (elements) */
  int32_t n[4];               /* sizes */
  double s[2];                /* scalars */
  double theta[8];
  int32_t n_units;            /* group forms */
  void* const* up[8];         /* HOST arrays of n_units device pointers */
  const int64_t* uld[4];      /* HOST arrays of n_units values */
  const int32_t* un[4];
  const double* us[2];
} gpfit_dev_ew_args;
int gpfit_dev_elementwise(gpfit_ctx* ctx, void* stream, int op, int is_f32, const gpfit_dev_ew_args* args);

/* The three launchers of skinny.hip (the slab products, their sums and the finish pass of gpfit_potrf_append_block;
 * tests/test_gpu_skinny.py), each on the caller's own device buffers.  The struct carries the fields of the launchers'
 * own argument structs under their own names (kernels.h: SkinnyArgs, SkinnySumArgs; M, kc and tri are common to the
 * two) and the arguments of the finish launcher (Lt, Lit, logdet, with L, ldl, Li, ldi, n of the sum and k = kc):
 *
 *   SLABS   A sam sar  B sbr sbc  O soz som soc  alpha  M K kc tri
 *   SUM     P pz  M kc nslab tri mode  dst;  mode ROWS (1): L ldl Li ldi n;  mode SCHUR (2): Kc ldk n
 *   FINISH  Lt Lit  L ldl Li ldi  n kc  logdet
 *
 * The hook fills the launcher's arguments and returns its return code; it adds no arithmetic.  -3 before any launch: an
 * unknown op, a NULL among the pointers the op (and its mode) reads or writes, M, K, nslab or n below 1, kc outside
 * 1 .. 128, tri outside 0 .. 2, a mode outside 0 .. 2.  The call only enqueues. */
enum { GPFIT_SKINNY_SLABS = 0, GPFIT_SKINNY_SUM, GPFIT_SKINNY_FINISH, GPFIT_SKINNY_NOPS };
typedef struct gpfit_dev_skinny_args {
  const double* A; int64_t sam, sar;
  const double* B; int64_t sbr, sbc;
  double* O; int64_t soz, som, soc;
  double alpha;
  int32_t M, K, kc, tri;
  const double* P; int64_t pz;
  int32_t nslab, mode;
  double* dst;
  double* L; int64_t ldl;
  double* Li; int64_t ldi;
  const double* Kc; int64_t ldk;
  int32_t n;
  const double* Lt; const double* Lit;
  double* logdet;
} gpfit_dev_skinny_args;
int gpfit_dev_skinny(gpfit_ctx* ctx, void* stream, int op, const gpfit_dev_skinny_args* args);

/* The launchers of projected.hip that run behind no chain gate (tests/test_gpu_projected.py), each on the caller's own
 * device buffers.  The five passes of the projected closures are unit-batched: up[k] is a HOST array of n_units
 * (1 .. 16) DEVICE pointers, uA / ulambda0 / un HOST arrays of n_units values, copied into ProjGroupT / PerUnit<>; the
 * three passes of the projected E-step are the single launchers on p[].  Slots, in the order below:
 *
 *   MOMENTS        up: am Kb aV mb Kvec r lam_m lam_var f gm gv part out3     n nb ld   uA ulambda0   (with its sum3)
 *   GA             up: Kb aV gm gv mb Ga                                      n np nb ld
 *   GKB            up: am gv GaKi                                             n np nb ld
 *   GKTB           up: Ki P1 P2 bvec G                                        nb ld
 *   TRACE          up: A out                                                  ld (of A)   un (n per unit)
 *   ESTEP_ROWS     p: a mb f r sv u                                           lda nb n nrows   A
 *   ESTEP_SCALE    p: aL sv u Y aLp(opt) part                                 lda (of aL) ld nb n nrows npc
 *   ESTEP_MOMENTS  p: Z z1 kv0 lam_m lam_var                                  ld nb n
 *
 * The hook fills the launcher's arguments and returns its return code; it adds no arithmetic.  -3 before any launch: an
 * unknown op, n_units outside 1 .. 16, a NULL among the tables or pointers the op requires (aLp may be NULL), an extent
 * below 1, np or nrows below n, nrows no multiple of 32, a leading dimension below its width.  The call only
 * enqueues. */
enum {
  GPFIT_PROJ_MOMENTS = 0, GPFIT_PROJ_GA, GPFIT_PROJ_GKB, GPFIT_PROJ_GKTB, GPFIT_PROJ_TRACE, GPFIT_PROJ_ESTEP_ROWS,
  GPFIT_PROJ_ESTEP_SCALE, GPFIT_PROJ_ESTEP_MOMENTS, GPFIT_PROJ_NOPS
};
typedef struct gpfit_dev_proj_args {
  int32_t n_units, n, np, nb, nrows, npc;
  int64_t ld, lda;
  double A;
  void* const* up[13];        /* HOST arrays of n_units device pointers */
  const double* uA;           /* HOST arrays of n_units values */
  const double* ulambda0;
  const int32_t* un;
  void* p[6];                 /* device pointers of the single launchers */
} gpfit_dev_proj_args;
int gpfit_dev_projected(gpfit_ctx* ctx, void* stream, int op, const gpfit_dev_proj_args* args);

#ifdef __cplusplus
}
#endif
#endif /* GPFIT_MI355X_H */
