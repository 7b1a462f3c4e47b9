// Workspace context of the GP fit library.  Internal header.
#pragma once
#include "kernels.h"
#include <vector>

struct gpfit_ctx {
  int device = 0;
  int np_cap = 0, dp_cap = 0, dfull_cap = 0;
  hipStream_t aux = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;

  // N x N work matrices (each np_cap^2 doubles)
  double *Kbuf = nullptr, *Cos = nullptr, *Lbuf = nullptr, *Libuf = nullptr, *Vbuf = nullptr, *LVbuf = nullptr,
         *LiVbuf = nullptr, *Tbuf = nullptr, *Zbuf = nullptr, *Wbuf = nullptr, *Abuf = nullptr, *Tmp = nullptr,
         *TmpV = nullptr;
  // N x d / d x d
  double *Xt = nullptr, *Xm = nullptr, *XCt = nullptr, *Cmat = nullptr, *Ybuf = nullptr, *Mpart = nullptr,
         *Mmat = nullptr, *Xt2 = nullptr, *XCt2 = nullptr, *XDt = nullptr, *XDt2 = nullptr, *dCpad = nullptr;
  // vectors (np_cap each unless noted)
  double *Kvec = nullptr, *q = nullptr, *lam_m = nullptr, *lam_var = nullptr, *fvec = nullptr, *wl = nullptr,
         *yv = nullptr, *bv = nullptr, *tvec = nullptr /* 2 np */, *mpad = nullptr, *rpad = nullptr,
         *q2 = nullptr, *dq1 = nullptr, *dq2 = nullptr, *hvec = nullptr;
  double *upart = nullptr, *vpart = nullptr, *sumA_part = nullptr, *frob_part = nullptr, *trmv_part = nullptr;
  double* rect_part = nullptr;  // (np/64)^2 per-tile sums of the rectangular adjoint
  void* sk_ws[2] = {nullptr, nullptr};  // stream-K partial-tile workspaces (main stream / side stream)
  // look-ahead: the first product of every inverse merge (tmp = L21 Li11) runs on the side stream
  // while the second half of the block is being factored (fit.hip:potrf_lockstep)
  hipStream_t side = nullptr;
  std::vector<hipEvent_t> side_ev;
  int side_ev_next = 0;
  double* scal = nullptr;       // device scalars [64]
  double* scal_host = nullptr;  // pinned [SCAL_HOST_COUNT]: the copy of scal, then slots only the device writes
  int* pix = nullptr;           // device [dfull_cap]
  int* pix_host = nullptr;      // pinned
  int* info = nullptr;          // device [4]
  int* info_host = nullptr;     // pinned [4]
  gpfit::ChainBlock* chain = nullptr;  // device: the state and step records of gpfit_estep_chain
  double* chain_host = nullptr;        // pinned [CHAIN_MAX_STEPS][CHAIN_REC]: the records, one copy at the chain's end
  std::vector<void*> allocs;
  int split_k_M = 32;

  // optional per-launch event timing of the dominant kernels (bench.py roofline leg)
  int profile = 0;
  struct ProfRec { hipEvent_t a, b; double flops; int kind; };  // kind 0 gemm T=128, 1 leaf, 2 gram, 3 gemm T<128
  std::vector<ProfRec> prof;
  std::vector<hipEvent_t> ev_pool;
  double prof_out[16] = {0};
  // profile == 2: phase timing only (eight events per fit, none inside the factorisations): 0 start,
  // 1 kernel build + moments done (fork), 2 K~'s solves done, 3 V factored, 4 T and its
  // norm done, 5 Q = I - T T^T done, 6 two-sided product done, 7 end
  hipEvent_t phase_ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool phase_valid = false;
  double last_enqueue_ms = 0.0;  // host time spent enqueuing the last fit_eval
  // evaluation enqueued but not yet collected (gpfit_fit_eval with the async flag / _finish)
  // done: recorded behind the result copies of a group (gpfit_fit_eval_batch), so that collecting a unit waits for
  // ITS group only and a second group can already run on the same stream (the single-unit call syncs the stream)
  struct Pending { bool active = false; hipStream_t stream = nullptr; double A = 0, lambda0 = 0, sigma0 = 0;
                   int n = 0, np = 0, d = 0, want_grad = 0, elem_bytes = 8; hipEvent_t done = nullptr;
                   bool use_done = false; } pend;

  // cached state of the last upload / evaluation (used by estep / predict entry points)
  int cur_n = 0, cur_np = 0, cur_d = 0, cur_dp = 0;
  bool lv_valid = false;  // LVbuf / scal[S_LOGDET_V] hold the factor and log-det of the last V
  bool lv32_valid = false;  // Vbuf holds the single-precision copy of that factor (mixed-precision mode)
  int lv_n = 0;
  int lv_bytes = 0;       // element size the cached factor was computed in
};

namespace gpfit {

// A stream-K workspace belongs to the stream its launches run on, so the two travel together: the caller's (main)
// stream pairs with the context's sk_ws[0] -- in a group, the leader's -- and the side stream with sk_ws[1].
struct Lane { hipStream_t s; void* sk_ws; };
inline Lane main_lane(const gpfit_ctx* c, hipStream_t s) { return {s, c->sk_ws[0]}; }
inline Lane side_lane(const gpfit_ctx* c) { return {c->side, c->sk_ws[1]}; }
int ensure_side_stream(gpfit_ctx* c);   // fit.hip: the side stream is created on first use

// ---- names of the numbered slots
// gpfit_ctx::scal (64 doubles) / scal_host (its copy, then the slots from 64 on), with who writes each
enum ScalSlot {
  S_RLAM = 0, S_SUMR = 1, S_SUMF = 2,   // likelihood sums r . lam_m, sum r, sum f (launch_moments / launch_proj_moments_group)
  S_LOGDET_K = 3,                       // log|K~| (launch_logdet / launch_logdet_pair)
  S_TRACE = 5,                          // ||T||_F^2 (launch_frob_finish / launch_frob_lower) or tr(K~_b^-1 V_b) (launch_proj_trace_group)
  S_MKM = 6,                            // m^T K~^-1 m (launch_dot)
  S_ADJ = 7, S_ADJ_WL = 8, S_ADJ_SUMA = 9,   // adjoint sums: sum u/q (S_ADJ), sum wl, sum A_w (launch_adjoint_reduce)
  S_METRIC = 10,                        // 10-14: the contraction with dC_p (launch_metric_contract), in the order ...
  S_D_AMP = 10, S_D_BETA = 11, S_D_RHO = 12, S_D_EPSX = 13, S_D_EPSY = 14,   // ... Amp, -2log2beta, -log2rho2, eps_0x, eps_0y
  S_RECT = 20, S_RECT_U1 = 21, S_RECT_U2 = 22,   // rectangular adjoint: sum A_w (S_RECT), sum u1/q1, sum u2/q2 (launch_adjoint_rect)
  S_FPARAM = 32,                        // 32-38, scal_host only: launch_fparam writes them directly (gpfit_fparam_eval)
  S_LOGDET_V = 40,                      // log|V| (launch_logdet / launch_logdet_pair); kept while lv_valid
  S_APPEND = 48, S_APPEND_LAMBDA = 49,  // gpfit_potrf_append: l . l, the new diagonal entry
  S_APPEND_LOGDET = 50,                 // gpfit_potrf_append_block: 2 sum log diag L22
  S_LBFGS = 52,                         // 52-60, scal_host only: launch_fparam_lbfgs writes them directly
  S_ELBO = 64,                          // 64-73, scal_host only (behind the copy of scal): launch_elbo_finish_group writes them directly
  SCAL_HOST_COUNT = 80,
};
// gpfit_ctx::info / info_host (4 ints)
enum InfoWord {
  INFO_K = 0, INFO_V = 1,   // LAPACK info of the two Cholesky chains (chol_leaf_reg.hip; gpfit_potrf_append: word 0)
  INFO_MOMENTS = 2,         // ticket of launch_moments' last-block reduction (0 between calls)
  INFO_METRIC = 3,          // ticket of launch_metric_contract (0 between calls)
};
// the tile walks of the large launches, in the order GPFIT_WALKS lists them (fit.hip: walk())
enum Walk { W_TRSM, W_TMP, W_MERGE, W_T, W_Q, W_RBASE, W_H, W_COUNT };
// out_host[16] of the fused closures (assemble_out; include/gpfit_mi355x.h documents them; engine.py reads by index)
enum OutSlot {
  OUT_LOSS = 0, OUT_LOGLIK = 1, OUT_KL = 2, OUT_GRAD = 3 /* 3-8 */, OUT_LOGDET_K = 9, OUT_LOGDET_V = 10, OUT_TRACE = 11,
  OUT_MKM = 12, OUT_D = 13, OUT_INFO_K = 14, OUT_INFO_V = 15, OUT_COUNT = 16,
};

// Every context entry point runs on the context's device whatever the caller's current device is,
// and restores the caller's device on return.
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) == hipSuccess && prev != device) switched = (hipSetDevice(device) == hipSuccess);
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};
// First statements of a context entry point (after its argument check): refuse to touch the
// workspace of an evaluation that is still in flight, then pin the device.
#define GP_PENDING_REFUSAL \
  "an asynchronous evaluation is pending on this context (collect it with gpfit_fit_eval_finish first)"
#define GP_CTX_ENTER(c, name)                         \
  if ((c)->pend.active) {                             \
    gpfit::set_error(name ": " GP_PENDING_REFUSAL);   \
    return -3;                                        \
  }                                                   \
  gpfit::DeviceGuard _device_guard((c)->device)

// profiling scope: when a context with profile=1 is evaluating, launches are bracketed by events
void prof_begin(gpfit_ctx* c);
void prof_end(gpfit_ctx* c);   // synchronises and fills c->prof_out
struct ProfScope {
  hipStream_t s; double flops; int kind; hipEvent_t a = nullptr;
  ProfScope(hipStream_t s, double flops, int kind);
  ~ProfScope();
};
template <typename R> double gemm_flops(const GemmArgsT<R>& g, int tile);

// Recursive blocked Cholesky of one or several matrices of the same size, factored in lock step
// (fit.hip:potrf_lockstep): chain b factors A[b] (lower triangle, destroyed) into L[b] with the inverse blocks in
// Li[b], scratch Tmp[b], LAPACK info in info[b].
template <typename R>
struct CholBatchT {
  int nb = 0;
  R* A[GEMM_MAXB];
  R* L[GEMM_MAXB];
  R* Li[GEMM_MAXB];
  R* Tmp[GEMM_MAXB];
  int* info[GEMM_MAXB];
  int64_t ld = 0;
  gpfit_ctx* ctx = nullptr;  // look-ahead resources (this context's side stream), or nullptr: one stream
  int side_min = 0;          // blocks of at least this size put their merge product on the side stream
};
// The n x n diagonal block at offset r0 (n a multiple of 128).  need: bit b = chain b needs the full inverse of
// its block (L^-1 costs n^3/3 more); the diagonal sub-block inverses every chain's solves need are always formed
// (n^3/12).  halves: bit b = chain b needs the inverses of the two diagonal half blocks but not the off-diagonal
// block [L^-1]21 (for callers that apply L^-1 block-wise, n^3/8 less than need); read at this node only.
// A chain in neither mask gets its factor and, of the inverse, the top block -- from first halves of VSOLVE_MIN on
// (fit.hip) only the two diagonal halves of that block: its row solve substitutes block-wise.
template <typename R>
int potrf_lockstep(const CholBatchT<R>& B, int r0, int n, uint32_t need, Lane lane, uint32_t halves = 0);

}  // namespace gpfit
