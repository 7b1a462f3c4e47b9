// Launchers of the non-GEMM kernels (elementwise / reductions / leaf).  Internal header.
#pragma once
#include "common.h"
#include "lbfgs1d.h"

namespace gpfit {

// Hyperparameters in the reference's dict order (utils.py:824) plus derived constants.
struct Theta {
  double sigma0, eps0x, eps0y, logbeta, logrho, amp;  // as given
  double eb, er;                                      // exp(-2log2beta), exp(-log2rho2)
};

// Per-unit housekeeping of a group of evaluations, one launch for the whole group instead of four small copies /
// fills per unit at the start and two device-to-host copies per unit at the end (each of those is a blit kernel with
// a host round trip behind it: 1.8 ms per group of 16 at the end alone, profiles/r03_group_idle.txt).
// Begin: the masked pixel list from its pinned host copy, info zeroed, the mean zero-padded to np.
// End: the unit's 64 scalars and 4 info words written straight into its pinned (device-visible) host buffers.
template <typename R>
struct GroupPrepT {
  int n_units, n, np;
  const int* pix_host[GEMM_MAXB / 2];
  int* pix[GEMM_MAXB / 2];
  int d[GEMM_MAXB / 2];
  int* info[GEMM_MAXB / 2];
  const R* m[GEMM_MAXB / 2];
  R* mpad[GEMM_MAXB / 2];
};
struct GroupCollectT {
  int n_units;
  const double* scal[GEMM_MAXB / 2];
  const int* info[GEMM_MAXB / 2];
  double* scal_host[GEMM_MAXB / 2];
  int* info_host[GEMM_MAXB / 2];
};
template <typename R>
int launch_group_prepare(const GroupPrepT<R>& g, hipStream_t s);
int launch_group_collect(const GroupCollectT& g, hipStream_t s);

// ---- chol_leaf_reg.hip: the 128 x 128 leaf of the recursive Cholesky, matrix in registers (co-resident with GEMM
// workgroups).  n independent blocks in one launch (one workgroup each): block b factors A[b] (lower triangle) into
// L[b] and its inverse Li[b] and reports the first non-positive pivot (LAPACK info, + info_base) into info[b];
// common leading dimensions and info_base
template <typename R>
struct LeafBatchT {
  const R* A[GEMM_MAXB];
  R* L[GEMM_MAXB];
  R* Li[GEMM_MAXB];
  int* info[GEMM_MAXB];
  int64_t lda, ldl, ldi;
  int info_base;
  int n;
};
template <typename R> int launch_chol_leaf_batch(const LeafBatchT<R>& bt, hipStream_t s);

// ---- skinny.hip: products with at most 128 columns on one side and a long reduction, cut into fixed slabs of the
// reduction across workgroups (gpfit_potrf_append_block).  Stage 1 writes per-slab partials, stage 2 adds them in slab
// order: no atomics, the same bits on every run.
constexpr int SKINNY_SLAB = 256;   // rows of the reduction per slab
constexpr int SKINNY_MT = 64;      // output rows per workgroup
constexpr int SKINNY_LD = 128;     // widest skinny side = leading dimension of the partials and of the n x k work matrices
struct SkinnyArgs {
  const double* A; int64_t sam, sar;   // op(A)(m, r) at A[m sam + r sar]
  const double* B; int64_t sbr, sbc;   // B(r, c) at B[r sbr + c sbc]
  double* O; int64_t soz, som, soc;    // out(z)(m, c) at O[z soz + m som + c soc]
  double alpha;
  int M, K, kc;                        // rows of the output, length of the reduction, columns (1 .. 128)
  int tri;                             // 0 dense; op(A)(m, r) is taken as zero for 1: r > m, 2: r < m
};
inline int skinny_slabs(int K) { return (K + SKINNY_SLAB - 1) / SKINNY_SLAB; }
// does slab z hold anything of the row panel that starts at row mt0 (a multiple of SKINNY_MT)?
__host__ __device__ inline bool skinny_slab_live(int tri, int z, int mt0) {
  if (tri == 1) return z * SKINNY_SLAB < mt0 + SKINNY_MT;
  if (tri == 2) return (z + 1) * SKINNY_SLAB > mt0;
  return true;
}
int launch_skinny_slabs(const SkinnyArgs& a, hipStream_t s);
enum SkinnySumMode {
  SKINNY_SUM_PLAIN = 0,   // dst[m][c] = sum
  SKINNY_SUM_ROWS = 1,    // and L[n + c][m] = sum, L[m][n + c] = Li[m][n + c] = 0   (Y = L^-1 K12: L21 = Y^T)
  SKINNY_SUM_SCHUR = 2,   // dst = the 128 x 128 tile of S = K22 - sum (K22 = rows n .. of Kc, lower triangle), unit diagonal behind k
};
struct SkinnySumArgs {
  const double* P; int64_t pz;   // partial (z)(m, c) at P[z pz + m SKINNY_LD + c]
  int M, kc, nslab, tri, mode;
  double* dst;                   // [.][SKINNY_LD]
  double* L; int64_t ldl; double* Li; int64_t ldi; int n;   // SKINNY_SUM_ROWS
  const double* Kc; int64_t ldk;                             // SKINNY_SUM_SCHUR (and n)
};
int launch_skinny_sum(const SkinnySumArgs& a, hipStream_t s);
// rows n .. n + k - 1, columns n .. of both factors from the leaf's 128-tiles (zero above the diagonal); logdet[0] = 2 sum log diag
int launch_append_block_finish(const double* Lt, const double* Lit, double* L, int64_t ldl, double* Li, int64_t ldi, int n,
                               int k, double* logdet, hipStream_t s);

// ---- elementwise.hip  (templated on the scalar type R = double | float; reductions are always
//      accumulated and returned in fp64)
// Spatial metric C (utils.py:861-914) over the masked pixels pix[d] of an n_rows x n_cols
// grid.  C is written zero-padded to [dp][ldc]; dC (optional) as 5 dense [d][d] matrices in
// the order Amp, -2log2beta, -log2rho2, eps_0x, eps_0y (the reference's dict order, :910).
template <typename R>
int launch_localker(const Theta& th, const int* pix, int d, int dp, int n_rows, int n_cols, R* C, int64_t ldc,
                    R* dC, hipStream_t s);
// Xt[k][n] = X[n][pix[k]] (k-major, zero padded to [dp][ldt]) and optionally the row-major
// masked copy Xm[n][k] ([np][ldm], zero padded).  dp, np: multiples of 32.  Of X only the rows below n and the columns
// the pixel list names are read (pix == nullptr: the first d columns).
template <typename R>
int launch_gather(const R* X, int64_t ldx, int n, const int* pix, int d, int dp, int np, R* Xt, int64_t ldt, R* Xm,
                  int64_t ldm, hipStream_t s);
// h[n] = sum_k Xt[k][n]*XCt[k][n];  Kvec = h + s0^2;  q = sqrt(Kvec)  (Kvec = q = 1 on the padding n .. np: the
// adjoint pass multiplies q's padding by zero, so it has to be finite).  All dp rows, the columns below n only, are read.
template <typename R>
int launch_qvec(const R* Xt, const R* XCt, int64_t ld, int dp, int n, int np, double s0sq, R* Kvec, R* q,
                hipStream_t s);
// dst lower tiles <- src (n x n, ld lds) with identity padding up to np (a multiple of 128).  Whole 128-tiles on and
// below the diagonal are written -- inside a diagonal tile what src holds above its diagonal is copied as it is -- and
// the tiles above the diagonal are left alone.
template <typename R>
int launch_pack_lower(const R* src, int64_t lds, int n, R* dst, int64_t ldd, int np, hipStream_t s);
// mirror the lower triangle of an n x n matrix into its upper triangle (in place)
template <typename R> int launch_symmetrize(R* A, int64_t lda, int n, hipStream_t s);
// out[0] = 2*sum_i log(L_ii), i < n
template <typename R> int launch_logdet(const R* L, int64_t ldl, int n, double* out, hipStream_t s);
template <typename R> int launch_logdet_pair(const R* L0, double* out0, const R* L1, double* out1, int64_t ldl, int n, hipStream_t s);
// out[0] = sum over the lower-triangular tiles of T^2 (T has exact zeros above its diagonal inside the diagonal tiles;
// the tiles above the diagonal are not read).  np: a multiple of 128; partial: np/128 (np/128 + 1) / 2 doubles.
template <typename R>
int launch_frob_lower(const R* T, int64_t ldt, int np, double* out, double* partial, hipStream_t s);
// y = L x (L lower, row-major) ; and z = L^T x.  Only L[i][j], j <= i, is read: what lies above the diagonal may hold
// anything.  All np entries of x are read and of y / z written (a padded factor has the identity there).  The transposed
// form needs np a multiple of 64 and partial: ceil(np / TRMV_ROWS) * np doubles.
template <typename R> int launch_trmv_lower(const R* L, int64_t ldl, int np, const R* x, R* y, hipStream_t s);
template <typename R>
int launch_trmv_lower_t(const R* L, int64_t ldl, int np, const R* x, R* z, double* partial, hipStream_t s);
// the dense off-diagonal block of a factor applied to a vector (M rows x cols, row-major): out = y - M x, and
// out = y - M^T x (cols a multiple of 64; partial: ceil(rows / TRMV_ROWS) * cols doubles).  Deterministic, no atomics.
template <typename R>
int launch_gemv_sub(const R* M, int64_t ldm, int rows, int cols, const R* x, const R* y, R* out, hipStream_t s);
template <typename R>
int launch_gemv_t_sub(const R* M, int64_t ldm, int rows, int cols, const R* x, const R* y, R* out, double* partial,
                      hipStream_t s);
// partial[t] = sum of squares of 128-tile t of a rows x cols block (multiples of 128): all tiles in row-major order,
// or (lower, square) the tiles on / below the diagonal in the order of the GEMM's tile-norm epilogue
template <typename R>
int launch_frob_tiles(const R* T, int64_t ldt, int rows, int cols, int lower, double* partial, hipStream_t s);
// dst (fp32) <- src (fp64) over a rows x cols block
int launch_demote_block(const double* src, int64_t lds, float* dst, int64_t ldd, int rows, int cols, hipStream_t s);
// out[0] = x . y
template <typename R> int launch_dot(const R* x, const R* y, int n, double* out, hipStream_t s);

// Latent moments / rate / likelihood pieces in the full-rank original basis; of Cos and V the diagonals
// alone are read, every vector below n only:
//   lam_m = m ; lam_var = Kvec - K~_ii + V_ii ; f = exp(A lam_m + A^2/2 lam_var + lambda0)
//   scal[0] = r.lam_m  scal[1] = sum r  scal[2] = sum f
//   wl_i = -1/2 A^2 f_i g_i  with g_i = 1 - J_ii - (pi - delta_ii)(1 - c_ii)/pi
template <typename R>
int launch_moments(const R* Kvec, const R* q, const R* Cos, int64_t ldc, const R* V, int64_t ldv, const R* m,
                   const R* r, int n, double A, double lambda0, R* lam_m, R* lam_var, R* f, R* wl, double* scal,
                   double* part, int* ticket, hipStream_t s);   // part: 3 ceil(n / 256) doubles; ticket: 0 between calls

// Adjoint pass over the lower tiles of W (np x np):
//   w = W_ij - 1/2 b_i b_j ; Aw = w (pi - acos c)/pi ; Bm = w sqrt(1-c^2)/pi
//   Aout = Lambda = tril(Aw, -1) + 1/2 diag(Aw) on the lower 64-tiles (Aw = Lambda + Lambda^T; zeros above the
//   diagonal inside the diagonal tiles, zero on padding); the tiles above the diagonal are not written;
//   upart[tj][i] = sum_{j in tile tj} Bm_ij q_j  (+ mirrored contribution -> vpart[ti][j])
//   sumA_part[tile] = sum of Aw over the tile (off-diagonal tiles counted twice)
// np: a multiple of 64.  The canonical lower triangle of W and Cos alone is read, below row and column n (a diagonal
// tile takes (j, i) for i < j).  b is read below n only; q up to np, its padding multiplied by zero: it has to be finite
// (launch_qvec writes 1).  upart, vpart: np/64 * np doubles each, sumA_part: one per lower tile; upart[t][i] is written for
// t <= i / 64 and vpart[t][i] for t > i / 64, and that is all launch_adjoint_reduce reads.
template <typename R>
int launch_adjoint(const R* W, const R* Cos, int64_t ld, const R* b, const R* q, int n, int np, R* Aout,
                   double* upart, double* vpart, double* sumA_part, hipStream_t s);
// u_i = sum_t upart[t][i] + vpart[t][i];  tvec_i = u_i/q_i - wl_i (uq: fp64 scratch [np]);
// scal_out[0] = sum_i u_i/q_i, scal_out[1] = sum_i wl_i, scal_out[2] = sum of sumA_part
// (ntile = np / 64, ntile_tri = the number of lower tiles; q and wl are read below n only; tvec and uq are zero on n .. np)
template <typename R>
int launch_adjoint_reduce(const double* upart, const double* vpart, const double* sumA_part, int ntile,
                          int ntile_tri, const R* q, const R* wl, int n, int np, R* tvec, double* uq,
                          double* scal_out, hipStream_t s);
// Y[n][k] += scale * t[n] * Xm[n][k]  over all np rows and dp columns: the padding of t and Xm is read (zero there)
template <typename R>
int launch_rowscale_add(R* Y, int64_t ldy, const R* Xm, int64_t ldm, const R* t, int np, int dp, hipStream_t s,
                        double scale = 1.0);
// dst = sum_z src[z] (split-K reduction), count elements each; what lies between count and slice_stride is not read
template <typename RI, typename RO>
int launch_reduce_slices(const RI* src, int64_t slice_stride, int nslice, RO* dst, int64_t count, hipStream_t s);
// dst [rows][cols] = sum over the live k slabs of a row, z >= row / slab_rows, of src[z] (GemmArgsT::k_slabs); the
// slabs below a row's own never were written and are not read (rows past the last slab's start take the last slab)
template <typename R>
int launch_reduce_slabs(const R* src, int64_t slab_stride, int nslab, int slab_rows, R* dst, int rows, int cols, hipStream_t s);
// dst = G + G^T, G = sum_z src[z] (n x n)
template <typename R>
int launch_reduce_slices_sym(const R* src, int64_t slice_stride, int nslice, R* dst, int n, hipStream_t s);
// grad5[p] = sum_kl dC_p[k][l] * M[k][l] for the five metric hyperparameters, dC recomputed from C
template <typename R>
int launch_metric_contract(const Theta& th, const int* pix, int d, int n_rows, int n_cols, const R* C, int64_t ldc,
                           const R* M, int64_t ldm, double* grad5, double* part /* >= 160 doubles */,
                           int* ticket /* device int, 0 between calls */, hipStream_t s);
int launch_frob_finish(const double* partial, int nt, double* out, hipStream_t s);
template <typename R> int launch_add_diag(R* A, int64_t lda, int n, double v, hipStream_t s);
template <typename R> int launch_scale_copy(R* dst, const R* src, int n, double alpha, hipStream_t s);
// dst = a * dst + b * src over a rows x cols block (cols even)
template <typename R>
int launch_axpby_block(R* dst, int64_t ldd, const R* src, int64_t lds, int rows, int cols, double a, double b,
                       hipStream_t s);

// rectangular adjoint pass (W[n1][n2] against the analytic dK of acosker(x1, x2)): A_w, the two
// u vectors as t = u/(2q) (+ extra1) and u/q, scal3 = {sum A_w, sum u1/q1, sum u2/q2}
// np1, np2: multiples of 64.  W, Cos, q1, q2 and extra1 are read inside n1 x n2 only; Aout is written over np1 x np2 and
// t1, uq1 / t2, uq2 over np1 / np2, zero on the padding.  upart: np2/64 * np1, vpart: np1/64 * np2, tile_sum: one per tile.
int launch_adjoint_rect(const double* W, int64_t ldw, const double* Cos, int64_t ldc, const double* q1,
                        const double* q2, int n1, int n2, int np1, int np2, double* Aout, int64_t lda, double* upart,
                        double* vpart, double* tile_sum, const double* extra1, double* t1, double* t2, double* uq1,
                        double* uq2, double* scal3, hipStream_t s);

// active-learning utility of nstar candidates (utils.py:413-525), r = list of response counts
int launch_nd_utility(const double* sigma2, const double* mu, int64_t nstar, const double* r, int nr, double* U,
                      hipStream_t s);

// ---- helpers of the general (materialising) acosker / localker entry points
int launch_pad_copy(const double* src, int64_t lds, int rows, int cols, double* dst, int64_t ldd, int prow,
                    int pcol, hipStream_t s);
int launch_symmetrize_avg(double* A, int64_t lda, int n, hipStream_t s);
int launch_dk_sigma0(const double* Cos, int64_t ldc, const double* q1, const double* q2, int n1, int n2,
                     double s0, double* dK, int64_t ldk, hipStream_t s);
int launch_dq(const double* Xt, const double* XDt, int64_t ld, int dp, int n, const double* q, double* dq,
              double* h, hipStream_t s);
int launch_dk_metric(double* H, int64_t ldh, const double* Cos, int64_t ldc, const double* q1, const double* q2,
                     const double* dq1, const double* dq2, int n1, int n2, hipStream_t s);
int launch_fill(double* x, int64_t n, double v, hipStream_t s);

// ---- projected.hip (the element-wise passes of the truncated-rank and sparse closures: ProjGroupT below)
// fused E-step in the projected basis (gpfit_estep_projected): per-row scalars s = A sqrt(f), u = A^2 f (a m) + A (r - f)
// over nrows >= n rows (zero on the padding); then Y = diag(s) aL zero-padded to [nrows][ld] (nrows a multiple of
// 32) with the slice sums of aL^T u in part[nrows / 32][npc]
int launch_estep_proj_rows(const double* a, int64_t lda, int nb, const double* mb, const double* f, const double* r,
                           int n, int nrows, double A, double* sv, double* u, hipStream_t s);
int launch_estep_proj_scale(const double* aL, int64_t ldal, int nb, int n, int nrows, const double* sv, const double* u,
                            double* Y, double* aLp /* or nullptr */, int64_t ld, int npc, double* part, hipStream_t s);
// lam_m = Z z1, lam_var = kv0 + row norms^2 of Z (Z = aL L_W^-T: the moments of lambda behind the update)
int launch_estep_proj_moments(const double* Z, int64_t ld, int nb, const double* z1, const double* kv0, int n,
                              double* lam_m, double* lam_var, hipStream_t s);

// ---- E-step / factorisation / firing-rate helpers
// estep_prep: s = A sqrt(f), rhs = A^2 f m + A (r - f) below n, both zero on n .. np.  estep_build: M = I + diag(s) K diag(s)
// and Kl = K on the lower 128-tiles of np x np (identity / zero padding; the tiles above the diagonal are left alone),
// SK = diag(s) K in full (zero padded).  K is read inside n x n only; sv over all of [0, np): its padding has to be the zero
// estep_prep writes.  np: a multiple of 128.
int launch_estep_prep(const double* f, const double* r, const double* m, int n, int np, double A, double* sv,
                      double* rhs, hipStream_t s);
int launch_estep_build(const double* K, int64_t ldk, int n, int np, const double* sv, double* Mb, double* SK,
                       double* Kl, int64_t ld, hipStream_t s);
// y = A x for a symmetric A stored in its lower triangle: what lies above the diagonal is not read
int launch_symv_lower(const double* A, int64_t lda, int n, const double* x, double* y, hipStream_t s);
// dst (n x n) <- the lower triangle of src, mirrored (unpack_sym) or with zeros above the diagonal (unpack_tri); what src
// holds above its diagonal is not read
int launch_unpack_sym(const double* src, int64_t lds, int n, double* dst, int64_t ldd, hipStream_t s);
int launch_unpack_tri(const double* src, int64_t lds, int n, double* dst, int64_t ldd, hipStream_t s);
// dst [np][ldd] <- the lower triangle of src (n x n; what src holds above its diagonal is not read), zero above the
// diagonal, identity padding up to np: a triangular operand of product, or (launch_symmetrize behind it) a symmetric one
int launch_pack_tri(const double* src, int64_t lds, int n, double* dst, int64_t ldd, int np, hipStream_t s);
int launch_fparam(const double* lam_m, const double* lam_var, const double* r, int n, double A, int closed_form,
                  double lambda0_in, double* f, double* out, hipStream_t s);
// The rate-parameter L-BFGS of an E-step in one launch (one workgroup): out[9] as documented at the kernel.
int launch_fparam_lbfgs(const double* lam_m, const double* lam_var, const double* r, int n, double logA0,
                        int lambda0_mode, double lambda0_fixed, const Lbfgs1dConfig& cfg, double* f, double* out,
                        hipStream_t s);

// ---- chained E-steps (gpfit_estep_chain, gpfit_estep_chain_batch, gpfit_estep_chain_full, gpfit_estep_chain_full_batch):
// nEstep x (Newton update, moments, rate-parameter L-BFGS) enqueued in one go.  What a step hands to the next stays on the device in a ChainBlock;
// no kernel waits on another, every launch that makes a step visible to the caller tests the gate first.
// ONE family of kernels for one chain and for the chains of several independent units in lock step: the single call is
// the group of one.  Every small kernel of a step is one launch for the group, with the unit on a free grid dimension and
// a per-unit table passed by value (as GroupPrepT); a unit's sums run over the same block and thread indices in the same
// order whatever else is in the group, hence the same bits alone and in any group.  Each unit has its own ChainBlock and
// info word, so its gate is its own.
constexpr int CHAIN_MAX_STEPS = 1024;   // GPFIT_ESTEP_CHAIN_MAX_STEPS of the public header
constexpr int CHAIN_REC = 12;           // doubles per step record
enum ChainRecSlot {
  CR_LBFGS = 0,   // 0-8: the nine results of the optimiser (launch_fparam_lbfgs)
  CR_INFO = 9,    // LAPACK info of W = I + L^T G L
  CR_RAN = 10,    // 1: the step ran and was committed; 0: skipped (or its factorisation failed)
  CR_A = 11,      // the A = exp(logA) of the step's Newton update
};
struct ChainBlock {
  double logA;            // what the optimiser of the last committed step left: the next step starts from it
  double lambda0;         // the closed-form lambda0 that step left (its record's slot 1); informational, nothing reads it
  int stop, pad;          // non-zero once a step has failed: nothing is committed from then on
  double rec[CHAIN_MAX_STEPS][CHAIN_REC];
};
// Open while no earlier step has failed and this step's factorisation has not (block-uniform: two scalar loads).  The
// gated kernels build it from their unit's entries of the tables.
struct ChainGate {
  const int* stop;
  const int* info;
  __device__ __forceinline__ bool open() const { return *stop == 0 && *info == 0; }
};
constexpr int CHAIN_MAXU = GEMM_MAXB / 2;   // units per call: one factorisation chain each, half a pointer batch like GroupPrepT
template <typename T>
struct PerUnit {
  T v[CHAIN_MAXU];
  __host__ __device__ __forceinline__ T operator[](int u) const { return v[u]; }
};
// The group as the host describes it once per call; every launcher hands its kernel the tables that kernel reads.
// (The full-rank chain fills what the bookkeeping, the commits and its own three kernels read, with nb = n and
// nrows = npc = round_up(n, 128).)
struct ChainGroupT {
  int n_units, n, nrows, npc, kmax;   // shared: training points, their padding, the padded basis size; the largest nb
  int64_t ld;                         // leading dimension of the work matrices (= npc)
  PerUnit<int> nb;
  PerUnit<const double*> a, aL, L, r, kv0;
  PerUnit<int64_t> lda, ldal, ldl, ldv;
  PerUnit<double*> m, f, V, lam_m, lam_var;
  PerUnit<double> logA0, lambda0;
  PerUnit<ChainBlock*> blk;
  PerUnit<int*> info;                 // the context's four info words; word INFO_K (0) is the chain's
  PerUnit<double*> rec_host;          // the context's pinned, device-visible chain_host
  // the work vectors and matrices of gpfit_estep_projected, per context
  PerUnit<double*> sv, u, t2, z1, z, mo, Y, Lp, Vw, part, aLp, Zm, W, Li, trmv_part;
  // the full-rank chain only: K[n][ldk] of gpfit_estep and the work matrix of S K
  PerUnit<const double*> K;
  PerUnit<int64_t> ldk;
  PerUnit<double*> SK;
};
// block <- (logA0, lambda0, stop = 0) and the first n_steps records zeroed
int launch_chain_init_group(const ChainGroupT& g, int n_steps, hipStream_t s);
// launch_estep_proj_rows with A = exp(blk->logA) formed on the device (the same row body: equal A, equal bits) on m, f;
// rec[step][CR_A] <- A unless the chain has stopped; the four info words zeroed (the first kernel of a step)
int launch_estep_proj_rows_chain_group(const ChainGroupT& g, int step, hipStream_t s);
int launch_estep_proj_scale_group(const ChainGroupT& g, hipStream_t s);
// behind the factorisation (one thread per unit): rec[step][CR_INFO] <- the info word, and the stop word is set when it
// is non-zero
int launch_chain_info_group(const ChainGroupT& g, int step, hipStream_t s);
// the commits of a step, each behind the gate: m <- mo, V <- Vw (launch_unpack_sym), launch_estep_proj_moments
int launch_chain_copy_group(const ChainGroupT& g, hipStream_t s);
int launch_unpack_sym_chain_group(const ChainGroupT& g, hipStream_t s);
int launch_estep_proj_moments_chain_group(const ChainGroupT& g, hipStream_t s);
// launch_fparam_lbfgs behind the gate, started at blk->logA: rec[step][0..8] <- its results and rec[step][CR_RAN] <- 1;
// with status 0 it leaves (logA, lambda0) in the block and the rate in f, otherwise it sets the stop word
// full_step (the damped chain only; null tables elsewhere): a unit whose word *full_step[u] is non-zero -- the info word of
// its V chain: this step was committed as the full step -- gets rec[step][CR_RAN] <- 2 instead
int launch_fparam_lbfgs_chain_group(const ChainGroupT& g, int step, int lambda0_mode, const Lbfgs1dConfig& cfg, hipStream_t s,
                                    PerUnit<const int*> full_step = PerUnit<const int*>{});
// the first n_steps records of every unit into its rec_host (one launch instead of a copy command per unit)
int launch_chain_collect_group(const ChainGroupT& g, int n_steps, hipStream_t s);
// the three kernels of the full-rank step only (gpfit_estep_chain_full, gpfit_estep_chain_full_batch), unit-batched like
// the rest: launch_estep_prep with A = exp(blk->logA) formed on the device (the same body: equal A, equal bits) into
// sv / u (the right-hand side), rec[step][CR_A] <- A unless the chain has stopped, the four info words zeroed;
// launch_estep_build (the same body) from each unit's K / ldk into W (M), SK and Vw (K's lower tiles); and, behind the
// gate, the moments of the original basis, lam_m <- mo, lam_var <- kv0 + diag(Vw) (Vw: the lower-tile work matrix
// holding V)
int launch_estep_prep_chain_group(const ChainGroupT& g, int step, hipStream_t s);
int launch_estep_build_group(const ChainGroupT& g, hipStream_t s);
int launch_estep_full_moments_chain_group(const ChainGroupT& g, hipStream_t s);
// the kernels of the damped step only (gpfit_estep_chain_damped, gpfit_estep_chain_damped_batch), unit-batched like the
// rest.  info_v: each unit's info word of the V chain (P = L^-1 V L^-T), zeroed by the step's first kernel; non-zero
// behind the first factorisation = V is not positive definite = the unit takes the full step in this update.
//   keep2    d0, d1 <- src (count doubles each): W1 before its factorisation, for the blend and for the fallback
//   mean     mo <- alpha mo + (1 - alpha) m over the unit's nb entries (the arithmetic of launch_axpby_block); a unit
//            with *info_v != 0 keeps mo, the full step's mean
//   restore  Wa <- W1c (count doubles) for a unit with *info_v != 0: nothing of the failed P chain stays in W_a
//   moments  behind the gate: lam_m = a m (m: the committed mean), lam_var = kv0 + row norms^2 of Z = aL L_Wa^-T
int launch_chain_keep2_group(int n_units, PerUnit<double*> src, PerUnit<double*> d0, PerUnit<double*> d1, int64_t count,
                             hipStream_t s);
int launch_chain_damped_mean_group(const ChainGroupT& g, PerUnit<const int*> info_v, double alpha, hipStream_t s);
int launch_chain_damped_restore_group(int n_units, PerUnit<const int*> info_v, PerUnit<double*> W1c, PerUnit<double*> Wa,
                                      int64_t count, hipStream_t s);
int launch_estep_damped_moments_chain_group(const ChainGroupT& g, hipStream_t s);
// launch_pack_tri for every unit of a group (the unit's own source, leading dimension and n)
int launch_pack_tri_group(int n_units, PerUnit<const double*> src, PerUnit<int64_t> lds, PerUnit<int> n, PerUnit<double*> dst,
                          int64_t ldd, int np, hipStream_t s);
// the unit-batched forms of the general kernels a step uses (common sizes and leading dimensions unless per unit)
int launch_pack_lower_group(int n_units, PerUnit<const double*> src, PerUnit<int64_t> lds, PerUnit<int> n, PerUnit<double*> dst,
                            int64_t ldd, int np, hipStream_t s);
int launch_add_diag_group(int n_units, PerUnit<double*> A, int64_t lda, int n, double v, hipStream_t s);
int launch_reduce_slices_group(int n_units, PerUnit<double*> src, int64_t slice_stride, int nslice, PerUnit<double*> dst,
                               int64_t count, hipStream_t s);
int launch_trmv_lower_group(int n_units, PerUnit<double*> L, int64_t ldl, int np, PerUnit<double*> x, PerUnit<double*> y,
                            hipStream_t s);
int launch_trmv_lower_t_group(int n_units, PerUnit<double*> L, int64_t ldl, int np, PerUnit<double*> x, PerUnit<double*> z,
                              PerUnit<double*> partial, hipStream_t s);

// ---- the sparse M-step closures of several independent units in one call (gpfit_fit_eval_sparse_batch; the single call
// gpfit_fit_eval_sparse is the group of one): the same rule -- the unit on a free grid dimension, tables by value, the
// single form's body over the same block and thread indices.
// Begin: the masked pixel list from its pinned host copy, the info words zeroed, m_b zero-padded to nb, and the two
// vectors the pull-backs expect cleared (bv, wl over the context's capacity).
struct ClosurePrepT {
  int n_units, nb, cap_max;
  PerUnit<const int*> pix_host;
  PerUnit<int*> pix, info;
  PerUnit<int> d, nk, cap;
  PerUnit<const double*> m_b;
  PerUnit<double*> mpad, bv, wl;
};
int launch_closure_prepare(const ClosurePrepT& g, hipStream_t s);
int launch_zero3_group(int n_units, PerUnit<double*> a, PerUnit<double*> b, PerUnit<double*> c, int64_t count, hipStream_t s);
int launch_pad_copy_group(int n_units, PerUnit<const double*> src, PerUnit<int64_t> lds, int rows, PerUnit<int> cols,
                          PerUnit<double*> dst, int64_t ldd, int prow, int pcol, hipStream_t s);
// the same with the row count per unit (gpfit_score_pool_batch: C and B of cells whose true sizes differ)
int launch_pad_copy_group(int n_units, PerUnit<const double*> src, PerUnit<int64_t> lds, PerUnit<int> rows, PerUnit<int> cols,
                          PerUnit<double*> dst, int64_t ldd, int prow, int pcol, hipStream_t s);
// launch_gather (the k-major copy only) and launch_qvec for unit u of a group: its own images, pixel list (or nullptr),
// true extents n[u], d[u] and sigma_0^2; the padded extents are the group's
int launch_gather_group(int n_units, PerUnit<const double*> X, PerUnit<int64_t> ldx, PerUnit<int> n, PerUnit<const int*> pix,
                        PerUnit<int> d, int dp, int np, PerUnit<double*> Xt, int64_t ldt, hipStream_t s);
int launch_qvec_group(int n_units, PerUnit<const double*> Xt, PerUnit<const double*> XCt, int64_t ld, int dp, PerUnit<int> n,
                      int np, PerUnit<double> s0sq, PerUnit<double*> Kvec, PerUnit<double*> q, hipStream_t s);
// launch_nd_utility for unit u of a group (its own moments and output; the response counts are the call's)
int launch_nd_utility_group(int n_units, PerUnit<const double*> sigma2, PerUnit<const double*> mu, int64_t nstar,
                            const double* r, int nr, PerUnit<double*> U, hipStream_t s);
int launch_symmetrize_group(int n_units, PerUnit<double*> A, int64_t lda, int n, hipStream_t s);
int launch_symmetrize_avg_group(int n_units, PerUnit<double*> A, int64_t lda, PerUnit<int> n, hipStream_t s);
// out0[u] = log|L0[u] L0[u]^T|, out1[u] likewise (launch_logdet_pair per unit, the unit's own n)
int launch_logdet_pair_group(int n_units, PerUnit<const double*> L0, PerUnit<double*> out0, PerUnit<const double*> L1,
                             PerUnit<double*> out1, int64_t ldl, PerUnit<int> n, hipStream_t s);
int launch_symv_lower_group(int n_units, PerUnit<double*> A, int64_t lda, int n, PerUnit<double*> x, PerUnit<double*> y,
                            hipStream_t s);
int launch_dot_group(int n_units, PerUnit<double*> x, PerUnit<double*> y, int n, PerUnit<double*> out, hipStream_t s);
int launch_proj_trace_group(int n_units, PerUnit<double*> A, int64_t lda, PerUnit<int> n, PerUnit<double*> out, hipStream_t s);
// the operands of the element-wise passes of the projected closures (gpfit_fit_eval_projected / _batch: a = B;
// gpfit_fit_eval_sparse / _batch: a = K_b K~_b^-1), per unit -- n training points padded to np rows, the padded basis
// size nb = the leading dimension ld:
//   moments  lam_m = a m_b, lam_var = Kvec - rowsum(a o K_b) + rowsum(aV o a), f, g_m = A (r - f), g_v = -A^2 f / 2;
//            out3 = {r . lam_m, sum r, sum f} through part (3 ceil(n / 4) doubles), added in block order
//   ga       G_a = g_m m_b^T - diag(g_v) K_b + 2 diag(g_v) aV                        (rows >= n zero)
//   gktb     G = 1/2 K~_b^-1 - 1/2 b b^T - 1/2 P1 + P2        (P1 = K~_b^-1 V_b K~_b^-1, P2 = a^T G_a K~_b^-1)
//   gkb      G_Kb = diag(g_v) a - G_a K~_b^-1, in place on GaKi                     (rows >= n zero)
struct ProjGroupT {
  int n_units, n, np, nb;
  int64_t ld;
  PerUnit<const double*> r;
  PerUnit<double> A, lambda0;
  PerUnit<double*> am, Kb, aV, mb, Kvec, lam_m, lam_var, f, gm, gv, part, out3;   // moments (am: a = K_b K~_b^-1, or B)
  PerUnit<double*> Ga, GaKi;                                                      // G_a ; G_a K~_b^-1 -> G_Kb in place
  PerUnit<double*> Ki, P1, P2, bvec, mkm, G;                                      // b = K~_b^-1 m_b, m_b . b ; G_K~b
};
int launch_proj_moments_group(const ProjGroupT& g, hipStream_t s);
int launch_proj_ga_group(const ProjGroupT& g, hipStream_t s);
int launch_proj_gkb_group(const ProjGroupT& g, hipStream_t s);
int launch_proj_gktb_group(const ProjGroupT& g, hipStream_t s);

// ---- the tracked loss of an EM iteration (gpfit_elbo; gpfit_elbo_batch: the single call is the group of one): the
// same rule -- the unit on a free grid dimension, tables by value.  Every sum is formed from per-workgroup partials that
// a finishing launch adds in index order: no floating-point atomics, no hand-off between workgroups, and a unit's
// partials depend on its own sizes only, hence the same bits alone and in any group.
constexpr int ELBO_QUAD_ROWS = 8;   // rows of K~^-1 per workgroup of elbo_quad_group (two per wave)
constexpr int ELBO_ROWS_WG = 32;    // workgroups of elbo_rows_group per unit: a fixed partition of [0, N)
constexpr int ELBO_OUT = 10;        // doubles of a unit's result (include/gpfit_mi355x.h: gpfit_elbo)
// One pass over the rows of Kinv[nb][ldki] beside V[nb][ldv] and m[nb], read where the caller has them:
//   part[2 w] = sum over the rows i of workgroup w of sum_j Kinv_ij V_ij,  part[2 w + 1] = ... of m_i sum_j Kinv_ij m_j
// (w < ceil(nb / ELBO_QUAD_ROWS)).  A row is read in pairs of columns, as one 16-byte load where the row starts on a
// 16-byte boundary and as two 8-byte loads elsewhere, and summed in the same order either way.
int launch_elbo_quad_group(int n_units, PerUnit<const double*> Kinv, PerUnit<int64_t> ldki, PerUnit<const double*> V,
                           PerUnit<int64_t> ldv, PerUnit<const double*> m, PerUnit<int> nb, PerUnit<double*> part,
                           hipStream_t s);
// part[3 b + {0, 1, 2}] = r . lam_m, sum r, sum f over the b-th of ELBO_ROWS_WG equal stretches of [0, n); the unit's
// four info words zeroed (the first kernel of the call)
int launch_elbo_rows_group(int n_units, PerUnit<const double*> r, PerUnit<const double*> f, PerUnit<const double*> lam_m, int n,
                           PerUnit<double*> part, PerUnit<int*> info, hipStream_t s);
// The partials added in index order, the ten results formed and written with the two info words straight into pinned
// host memory.  logdet_V / logdet_K: where launch_logdet_pair_group left them; info_V / info_K: the info words of the two
// chains; known: log|K~| is `given` and no K~ chain ran (its info counts as 0).  NaN into slots 1-4 when V's
// factorisation failed, into 1, 2 and 4 when K~'s did.
struct ElboFinishT {
  int n_units;
  PerUnit<int> nb, known;
  PerUnit<const double*> quad_part, rows_part, logdet_V, logdet_K;
  PerUnit<const int*> info_V, info_K;
  PerUnit<double> given, A, lambda0;
  PerUnit<double*> out_host;              // [ELBO_OUT]
  PerUnit<int*> info_V_host, info_K_host;
};
int launch_elbo_finish_group(const ElboFinishT& g, hipStream_t s);

}  // namespace gpfit
