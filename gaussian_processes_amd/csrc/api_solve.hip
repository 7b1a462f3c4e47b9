// C-ABI entry points built on the recursive MFMA Cholesky: a standalone factorisation
// (log_det, general solves of the drop-in module), the fused E-step Newton update and the
// one-pass firing-rate-parameter evaluation.
#include "units.h"
#include "gpfit_mi355x.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

using namespace gpfit;

// the context's K~ work matrices as a batch of one chain for potrf_lockstep, on the caller's stream only (no
// look-ahead side stream)
static CholBatchT<double> one_chain(gpfit_ctx* c, int64_t ld) {
  CholBatchT<double> b;
  add_k_chain(b, c);
  b.ld = ld;
  return b;
}

// The full-rank Newton update of gpfit_estep and of every step of gpfit_estep_chain_full / _batch, on the work matrices
// of every context of the list (M = I + S K S in Kbuf, S K in Zbuf, K's lower tiles in Wbuf; ld = np), in two halves:
// the chain records the factorisation's info word between them.  One unit or several: one lock-step recursion and one
// product per line for the list, so a unit has the same bits alone and in any group.
// From np = 2 TILE on T = L_M^-1 (S K) is formed block-wise, so that the off-diagonal block of L_M^-1 is never formed
// (N^3/4 less):   T1 = [L^-1]11 B1 ,  T2 = [L^-1]22 (B2 - L21 T1)        with B = S K ; n1 rows in the top block
static int full_update_split(int np) {
  if (np < 2 * TILE) return 0;   // one leaf with its full inverse
  const int kt = np / TILE;
  const int n1 = ((kt + 1) / 2) * TILE;
  return n1;
}
static int full_update_factor(const Units& U, int np, Lane lane) {
  CholBatchT<double> b;
  for (int i = 0; i < U.cnt; ++i) add_k_chain(b, U.ctx[i]);
  b.ld = np;
  if (full_update_split(np)) return potrf_lockstep(b, 0, np, 0u, lane, U.chains());   // [L^-1]11 and [L^-1]22 only
  return potrf_lockstep(b, 0, np, U.chains(), lane);
}
static int full_update_products(const Units& U, int np, Lane lane) {
  const int64_t ld = np;
  const auto Li = &gpfit_ctx::Libuf, L = &gpfit_ctx::Lbuf, SK = &gpfit_ctx::Zbuf, T = &gpfit_ctx::Abuf, Kl = &gpfit_ctx::Wbuf;
  // T = L_M^-1 (S K)          lower x dense                         N^3
  if (const int n1 = full_update_split(np)) {
    const int n2 = np - n1;
    GP_TRY(product(lane, {n1, np, n1}, 1.0, plain(tril(U.mats(Li, ld))), plain(U.mats(SK, ld)), into(U.mats(T, ld)), 1));
    GP_TRY(product(lane, {n2, np, n1}, -1.0, plain(U.mats(L, ld, n1)), plain(U.mats(T, ld)), into(U.mats(SK, ld, n1), 1.0)));
    GP_TRY(product(lane, {n2, np, n2}, 1.0, plain(tril(U.mats(Li, ld, n1, n1))), plain(U.mats(SK, ld, n1)), into(U.mats(T, ld, n1)), 1));
  } else {
    GP_TRY(product(lane, {np, np, np}, 1.0, plain(tril(U.mats(Li, ld))), plain(U.mats(SK, ld)), into(U.mats(T, ld)), 1));
  }
  // V = K - T^T T             lower tiles only                      N^3
  return product(lane, {np, np, np}, -1.0, trans(U.mats(T, ld)), plain(U.mats(T, ld)), into_lower(U.mats(Kl, ld), 1.0));
}

namespace {
// y_i = sum_{j <= i} M[i][j] x_j for a lower-triangular row-major M (one wave per row)
__global__ __launch_bounds__(256) void append_trmv_kernel(const double* __restrict__ M, int64_t ld, int n,
                                                           const double* __restrict__ x, double* __restrict__ y) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  double acc = 0.0;
  for (int j = lane; j <= row; j += 64) acc += M[(int64_t)row * ld + j] * x[j];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
  if (lane == 0) y[row] = acc;
}
// w_j = sum_{i >= j} M[i][j] l_i (a 64-column strip per workgroup, rows walked in four interleaved
// groups, summed in a fixed order: deterministic); also out[0] = l . l from workgroup 0
__global__ __launch_bounds__(256) void append_trmv_t_kernel(const double* __restrict__ M, int64_t ld, int n,
                                                             const double* __restrict__ l, double* __restrict__ w,
                                                             double* __restrict__ out) {
  __shared__ double part[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
  double acc = 0.0;
  if (c < n)
    for (int i = c + g; i < n; i += 4) acc += M[(int64_t)i * ld + c] * l[i];
  part[g][threadIdx.x & 63] = acc;
  __syncthreads();
  if (g == 0 && c < n) w[c] = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
  if (blockIdx.x == 0) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += l[i] * l[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
  }
}
// row n of both factors: L[n][:] = (l, lambda), Linv[n][:] = (-w / lambda, 1 / lambda); column n zeroed above
__global__ __launch_bounds__(256) void append_write_kernel(double* __restrict__ L, int64_t ldl, double* __restrict__ Li,
                                                            int64_t ldi, int n, const double* __restrict__ l,
                                                            const double* __restrict__ w, const double* __restrict__ kcol,
                                                            double* __restrict__ out, int* __restrict__ info) {
  const double p = kcol[n] - out[0];           // Schur complement of the new diagonal entry
  const bool bad = !(p > 0.0);
  const double lam = bad ? 1.0 : sqrt(p);
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j == 0) {
    out[1] = lam;
    if (bad) atomicCAS(info, 0, n + 1);
  }
  if (j < n) {
    L[(int64_t)n * ldl + j] = l[j];
    Li[(int64_t)n * ldi + j] = -w[j] / lam;
    L[(int64_t)j * ldl + n] = 0.0;
    Li[(int64_t)j * ldi + n] = 0.0;
  } else if (j == n) {
    L[(int64_t)n * ldl + n] = lam;
    Li[(int64_t)n * ldi + n] = 1.0 / lam;
  }
}

// the pass of one evaluation on host arrays (gpfit_fparam_lbfgs_host), sums in index order
struct FparamHostPass {
  const double* lam_m;
  const double* lam_var;
  int64_t n;
  double sr, srm;
  double A, se, sg;
  void pass(double logA) {
    A = std::exp(logA);
    se = 0.0;
    sg = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      const double e = std::exp(A * lam_m[i] + 0.5 * A * A * lam_var[i]);
      se += e;
      sg += (lam_m[i] + A * lam_var[i]) * e;
    }
  }
  double lambda0_closed() const { return std::log(sr) - std::log(se); }
  FparamValues values(double lambda0_used) const {
    const double el0 = std::exp(lambda0_used);
    const double sf = se * el0;
    return FparamValues{A * srm + lambda0_used * sr - sf, A * (srm - sg * el0), sf};
  }
};
}  // namespace

// history of the device optimiser: 4 * history_size doubles of dynamic LDS next to the 17 of the block sums
static const int kFparamLbfgsMaxHistory = (64 * 1024 - 256) / 32;

static int fparam_lbfgs_config(const char* name, int max_iter, int history_size, double lr, double tol_grad,
                               double tol_change, Lbfgs1dConfig* cfg) {
  // max_iter = 0: the first evaluation only (torch's step() evaluates before its loop); a history pair is only
  // stored from the second iteration on
  if (max_iter < 0 || history_size < 0 || (max_iter > 1 && history_size < 1) || !(lr >= 0.0)) {
    set_error(std::string(name) + ": bad argument (max_iter >= 0, history_size >= 1 when max_iter > 1, lr >= 0)");
    return -3;
  }
  if (history_size > kFparamLbfgsMaxHistory) {
    set_error(std::string(name) + ": history_size " + std::to_string(history_size) + " does not fit the " +
              std::to_string(kFparamLbfgsMaxHistory) + " pairs of the workgroup's LDS");
    return -3;
  }
  cfg->lr = lr;
  cfg->tolerance_grad = tol_grad;
  cfg->tolerance_change = tol_change;
  cfg->max_iter = max_iter;
  cfg->max_eval = max_iter * 5 / 4;  // torch's default max_eval
  cfg->history_size = history_size;
  return 0;
}

static_assert(GPFIT_ESTEP_CHAIN_MAX_STEPS == CHAIN_MAX_STEPS, "the header states the cap of the chain block");
static_assert(GPFIT_ESTEP_CHAIN_MAX_UNITS == CHAIN_MAXU, "the header states the units of a group call");
static_assert(GPFIT_ESTEP_CHAIN_FULL_MAX_UNITS == CHAIN_MAXU, "the header states the units of a group call");

// The skeleton of the chained E-steps: what the projected chain (estep_chain_group_impl) and the full-rank chain
// (estep_chain_full_group_impl) have in common -- n_steps x (a Newton update, its moments, the rate-parameter optimiser)
// for every unit on its own context, all on the caller's stream with one synchronisation at the end.  A kind of chain
// hands over its own operands' checks (admit), adds its work matrices to the group (group) and supplies the three
// stretches of a step that differ (run); everything else -- the shared arguments and their refusals, the bookkeeping
// fields of the ChainGroupT, the init, the info word, the gated commits of m and V, the optimiser, the collect and the
// records -- is here once.
struct ChainCall {
  // (in the order of the entry points' argument lists)
  const char* name; gpfit_ctx* const* ctxs; int n_units; void* stream; int64_t N;
  const double *const *r, *const *kv0;
  double *const *m, *const *f, *const *V; const int64_t* ldv; double *const *lam_m, *const *lam_var;
  const double* logA0; int lambda0_mode; const double* lambda0_fixed;
  int n_steps, max_iter, history_size; double lr, tol_grad, tol_change; double* rec_host;
  Lbfgs1dConfig cfg;   // (admit fills it)
  PerUnit<const int*> full_step{};   // (the damped chain fills it: the words that turn a record's slot 10 into 2)

  // Every refusal of the call, before anything is enqueued.  tables: the kind's own argument tables are there;
  // operands(u): so are unit u's entries of them; sizes(u): the unit's sizes and leading dimensions are in order;
  // fits(u): what the kind asks of the unit's context beyond the shared checks -- the sentence of a refusal, or empty.
  template <typename Operands, typename Sizes, typename Fits>
  int admit(bool tables, Operands&& operands, Sizes&& sizes, Fits&& fits) {
    const Refuse refuse{name};
    if (n_units < 1 || n_units > CHAIN_MAXU) return refuse("1 .. " + std::to_string(CHAIN_MAXU) + " units per call");
    if (n_steps < 1 || n_steps > CHAIN_MAX_STEPS)
      return refuse("n_steps " + std::to_string(n_steps) + " is not within 1 .. " + std::to_string(CHAIN_MAX_STEPS));
    if (!tables || !ctxs || !r || !kv0 || !m || !f || !V || !ldv || !lam_m || !lam_var || !logA0 ||
        (lambda0_mode && !lambda0_fixed) || !rec_host || N <= 0 || N > INT32_MAX)
      return refuse("bad argument");
    GP_TRY(fparam_lbfgs_config(name, max_iter, history_size, lr, tol_grad, tol_change, &cfg));
    for (int u = 0; u < n_units; ++u) {
      const std::string unit = unit_prefix(n_units, u);
      if (!ctxs[u] || !r[u] || !kv0[u] || !m[u] || !f[u] || !V[u] || !lam_m[u] || !lam_var[u] || !operands(u))
        return refuse(unit + "bad argument: null context or operand");
      if (!sizes(u)) return refuse(unit + "bad argument: bad size or leading dimension");
      if (const char* why = unit_context_refusal(ctxs, u)) return refuse(why);
      const std::string why = fits(u);
      if (!why.empty()) return refuse(unit + why);
    }
    return 0;
  }
  // The group with what both kinds fill the same way: n training points padded to nrows, the padded basis size npc =
  // the leading dimension of the work matrices, the caller's arrays, each context's chain block, info words and records.
  ChainGroupT group(int nrows, int npc) const {
    const Units U = Units::all(ctxs, n_units);
    ChainGroupT g{};
    g.n_units = n_units; g.n = (int)N; g.nrows = nrows; g.npc = npc; g.ld = npc;
    g.r = U.from(r); g.kv0 = U.from(kv0); g.ldv = U.from(ldv);
    g.m = U.from(m); g.f = U.from(f); g.V = U.from(V); g.lam_m = U.from(lam_m); g.lam_var = U.from(lam_var);
    g.logA0 = U.from(logA0);
    g.lambda0 = U.table<double>([&](int u) { return lambda0_mode ? lambda0_fixed[u] : 0.0; });
    g.blk = U.of(&gpfit_ctx::chain); g.info = U.of(&gpfit_ctx::info); g.rec_host = U.of(&gpfit_ctx::chain_host);
    return g;
  }
  // THE chain loop.  Of a step the kind supplies: before_factor(step), from the first kernel of the step (the only
  // reader of m and f in it, ahead of all of the step's writers; the damped step reads m once more there, for its
  // blend) up to and including the factorisation -- the last one, where a step has two; after_info(), the inputs of the
  // commits (mo and Vw); moments(), the moments of lambda behind the update.
  template <typename Before, typename After, typename Moments>
  int run(const ChainGroupT& g, Before&& before_factor, After&& after_info, Moments&& moments) const {
    DeviceGuard device_guard(ctxs[0]->device);
    hipStream_t s = (hipStream_t)stream;
    GP_TRY(launch_chain_init_group(g, n_steps, s));
    for (int step = 0; step < n_steps; ++step) {
      GP_TRY(before_factor(step));
      GP_TRY(launch_chain_info_group(g, step, s));
      // from here on a failed or skipped step only writes workspace: every write to the caller's arrays is gated
      GP_TRY(after_info());
      GP_TRY(launch_chain_copy_group(g, s));
      GP_TRY(launch_unpack_sym_chain_group(g, s));
      GP_TRY(moments());
      GP_TRY(launch_fparam_lbfgs_chain_group(g, step, lambda0_mode ? 1 : 0, cfg, s, full_step));
    }
    GP_TRY(launch_chain_collect_group(g, n_steps, s));
    GP_HIP(hipStreamSynchronize(s));
    for (int u = 0; u < n_units; ++u)
      for (int i = 0; i < n_steps * CHAIN_REC; ++i) rec_host[(size_t)u * n_steps * CHAIN_REC + i] = ctxs[u]->chain_host[i];
    return 0;
  }
};

// The stages gpfit_estep_projected and gpfit_estep_projected_damped share, on the work vectors and matrices of one
// context (ld = npc): the same launches in the same order for both callers.
struct ProjStep {
  gpfit_ctx* c;
  hipStream_t s;
  Lane lane;
  int n, k, nrows, npc;
  int64_t ld;
  double *sv, *u, *t2, *z1, *z, *mo, *Y, *Lp, *P, *V, *part, *aLp, *Zm;
  Mat<double> M(double* X) const { return mat(X, ld); }
};
static ProjStep proj_step(gpfit_ctx* c, hipStream_t s, int64_t N, int64_t nb) {
  ProjStep w{};
  w.c = c; w.s = s; w.lane = main_lane(c, s);
  w.n = (int)N; w.k = (int)nb; w.nrows = (int)round_up(N, TILE); w.npc = (int)round_up(nb, TILE);
  w.ld = w.npc;
  w.sv = c->yv; w.u = c->bv; w.t2 = c->tvec; w.z1 = c->mpad; w.z = c->rpad; w.mo = c->hvec;
  w.Y = c->Tbuf; w.Lp = c->Wbuf; w.P = c->Abuf; w.V = c->Zbuf; w.part = c->TmpV; w.aLp = c->LiVbuf; w.Zm = c->Cos;
  return w;
}
// t2 = (a L)^T u and W = I + Y^T Y in Kbuf (lower tiles, identity on the padding); with_aLp: the padded copy of aL too
static int proj_step_w(const ProjStep& w, const double* a, int64_t lda, const double* aL, int64_t ldal, const double* r,
                       const double* m, const double* f, double A, bool with_aLp) {
  gpfit_ctx* c = w.c;
  GP_TRY(launch_estep_proj_rows(a, lda, w.k, m, f, r, w.n, w.nrows, A, w.sv, w.u, w.s));
  GP_TRY(launch_estep_proj_scale(aL, ldal, w.k, w.n, w.nrows, w.sv, w.u, w.Y, with_aLp ? w.aLp : nullptr, w.ld, w.npc, w.part, w.s));
  GP_TRY((launch_reduce_slices<double, double>(w.part, w.npc, w.nrows / 32, w.t2, w.npc, w.s)));   // t2 = (a L)^T u
  // W = I + Y^T Y  (= I + L^T G L, G = A^2 a^T diag(f) a), lower tiles, identity on the padding
  GP_TRY(product(w.lane, {w.npc, w.npc, w.nrows}, 1.0, trans(w.M(w.Y)), plain(w.M(w.Y)), into_lower(w.M(c->Kbuf))));
  return launch_add_diag(c->Kbuf, w.ld, w.npc, 1.0, w.s);
}
// mo = L W^-1 (a L)^T u from W's inverse factor in Libuf; leaves L packed in Lp
static int proj_step_mean(const ProjStep& w, const double* L, int64_t ldl) {
  gpfit_ctx* c = w.c;
  GP_TRY(launch_trmv_lower(c->Libuf, w.ld, w.npc, w.t2, w.z1, w.s));
  GP_TRY(launch_trmv_lower_t(c->Libuf, w.ld, w.npc, w.z1, w.z, c->trmv_part, w.s));
  GP_TRY(launch_pack_lower(L, ldl, w.k, w.Lp, w.ld, w.npc, w.s));
  return launch_trmv_lower(w.Lp, w.ld, w.npc, w.z, w.mo, w.s);
}
// V (lower tiles) = P P^T, P = L Li^T with Li the inverse factor of the matrix whose inverse V is in L's coordinates
static int proj_step_cov(const ProjStep& w, double* Li) {
  GP_TRY(product(w.lane, {w.npc, w.npc, w.npc}, 1.0, plain(tril(w.M(w.Lp))), trans(tril(w.M(Li))), into(w.M(w.P))));
  return product(w.lane, {w.npc, w.npc, w.npc}, 1.0, plain(w.M(w.P)), trans(w.M(w.P)), into_lower(w.M(w.V)));
}

static_assert(GPFIT_ELBO_MAX_UNITS == CHAIN_MAXU, "the header states the units of a group call");
static_assert(2 * CHAIN_MAXU <= GEMM_MAXB, "two chains per unit in one lock-step batch");

// ONE body for gpfit_elbo (the group of one) and gpfit_elbo_batch (header: gpfit_elbo).  Per unit: V packed into the V
// chain's work matrix and, unless log|K~| is given, K~ into the K chain's; all chains of all units are one lock-step
// recursion that forms no full inverse; the two passes over the caller's arrays (elbo_rows_group, elbo_quad_group) read
// them where they are.  Partials: upart (the quadratic forms, 2 ceil(nb / 8) <= np / 4 doubles) and vpart (the three
// likelihood sums, 96 doubles); both hold at least 2 np doubles at any capacity.  Everything on the caller's stream, one
// synchronisation; a unit's launches, partials and sums do not depend on the other units: the same bits alone and in
// any group.
struct ElboCall {
  // (in the order of the entry points' argument lists)
  const char* name; gpfit_ctx* const* ctxs; int n_units; void* stream;
  const double *const *m, *const *V; const int64_t* ldv; const double* const* K; const int64_t* ldk;
  const double* const* Kinv; const int64_t *ldki, *nb; const int* known; const double* logdet_K;
  const double *const *r, *const *f, *const *lam_m; int64_t N; const double *logA, *lambda0;
  double* out_host; int* info_host;
};
static int elbo_group_impl(const ElboCall& a) {
  const Refuse refuse{a.name};
  gpfit_ctx* const* ctxs = a.ctxs;
  const int nu = a.n_units;
  // every refusal of the call, before anything is enqueued; those of the arguments before any context is read
  if (nu < 1 || nu > CHAIN_MAXU) return refuse("1 .. " + std::to_string(CHAIN_MAXU) + " units per call");
  if (!ctxs || !a.m || !a.V || !a.ldv || !a.Kinv || !a.ldki || !a.nb || !a.known || !a.logdet_K || !a.r || !a.f || !a.lam_m ||
      !a.logA || !a.lambda0 || !a.out_host || !a.info_host)
    return refuse("bad argument: null table or output");
  if (a.N <= 0 || a.N > INT32_MAX) return refuse("bad argument: N must be positive");
  auto K_of = [&](int u) { return a.K ? a.K[u] : nullptr; };
  for (int u = 0; u < nu; ++u) {
    const std::string unit = unit_prefix(nu, u);
    if (!ctxs[u] || !a.m[u] || !a.V[u] || !a.Kinv[u] || !a.r[u] || !a.f[u] || !a.lam_m[u])
      return refuse(unit + "bad argument: null context or operand");
    if (a.nb[u] <= 0) return refuse(unit + "bad argument: nb must be positive");
    if (!a.known[u] && !K_of(u)) return refuse(unit + "bad argument: K is needed unless logdet_K_known is set");
    if (a.ldv[u] < a.nb[u] || a.ldki[u] < a.nb[u] || (!a.known[u] && (!a.ldk || a.ldk[u] < a.nb[u])))
      return refuse(unit + "bad argument: a leading dimension is smaller than nb");
    // the recursion's split depends on the padded size: only equal padded sizes give the bits of the single call
    if (round_up(a.nb[u], TILE) != round_up(a.nb[0], TILE))
      return refuse(unit + "round_up(nb, 128) = " + std::to_string(round_up(a.nb[u], TILE)) + " differs from unit 0's " +
                    std::to_string(round_up(a.nb[0], TILE)) + " (group the units by padded size)");
  }
  for (int u = 0; u < nu; ++u) {
    const std::string unit = unit_prefix(nu, u);
    if (const char* why = unit_context_refusal(ctxs, u)) return refuse(unit + why);
    if (round_up(a.nb[u], TILE) > ctxs[u]->np_cap) return refuse(unit + "round_up(nb, 128) is larger than the context capacity");
  }
  DeviceGuard device_guard(ctxs[0]->device);
  hipStream_t s = (hipStream_t)a.stream;
  const Units U = Units::all(ctxs, nu);
  Units UK;   // the units whose K~ is factored here
  for (int u = 0; u < nu; ++u) {
    if (!a.known[u]) UK.add(ctxs[u], u);
    ctxs[u]->lv_valid = false; ctxs[u]->lv32_valid = false;   // the V work matrices are reused
  }
  const int n = (int)a.N, npc = (int)round_up(a.nb[0], TILE);
  const int64_t ld = npc;
  const auto nb_of = [&](int u) { return (int)a.nb[u]; };
  const PerUnit<int> nbt = U.table<int>(nb_of);
  const Lane lane = main_lane(ctxs[0], s);   // every launch on the caller's stream with the leader's workspace
  // the likelihood sums first: its kernel also zeroes the info words
  GP_TRY(launch_elbo_rows_group(nu, U.from(a.r), U.from(a.f), U.from(a.lam_m), n, U.of(&gpfit_ctx::vpart), U.of(&gpfit_ctx::info), s));
  GP_TRY(launch_elbo_quad_group(nu, U.from(a.Kinv), U.from(a.ldki), U.from(a.V), U.from(a.ldv), U.from(a.m), nbt,
                                U.of(&gpfit_ctx::upart), s));
  GP_TRY(launch_pack_lower_group(nu, U.from(a.V), U.from(a.ldv), nbt, U.of(&gpfit_ctx::Vbuf), ld, npc, s));
  if (UK.cnt)
    GP_TRY(launch_pack_lower_group(UK.cnt, UK.from(a.K), UK.from(a.ldk), UK.table<int>(nb_of), UK.of(&gpfit_ctx::Kbuf), ld, npc, s));
  CholBatchT<double> cb;
  for (int i = 0; i < U.cnt; ++i) add_v_chain(cb, U.ctx[i]);
  for (int i = 0; i < UK.cnt; ++i) add_k_chain(cb, UK.ctx[i]);
  cb.ld = ld;
  GP_TRY(potrf_lockstep(cb, 0, npc, 0u, lane));   // the factors only: no full inverse of either
  // log|V| and log|K~| (a unit whose log|K~| is given reads its V factor twice; the finishing launch takes the given one)
  GP_TRY(launch_logdet_pair_group(nu, U.cof(&gpfit_ctx::LVbuf), U.scal(S_LOGDET_V),
                                  U.table<const double*>([&](int u) { return a.known[u] ? ctxs[u]->LVbuf : ctxs[u]->Lbuf; }),
                                  U.scal(S_LOGDET_K), ld, nbt, s));
  ElboFinishT fin{};
  fin.n_units = nu; fin.nb = nbt;
  fin.known = U.table<int>([&](int u) { return a.known[u] ? 1 : 0; });
  fin.quad_part = U.cof(&gpfit_ctx::upart); fin.rows_part = U.cof(&gpfit_ctx::vpart);
  fin.logdet_V = U.table<const double*>([&](int u) { return ctxs[u]->scal + S_LOGDET_V; });
  fin.logdet_K = U.table<const double*>([&](int u) { return ctxs[u]->scal + S_LOGDET_K; });
  fin.info_V = U.table<const int*>([&](int u) { return ctxs[u]->info + INFO_V; });
  fin.info_K = U.table<const int*>([&](int u) { return ctxs[u]->info + INFO_K; });
  fin.given = U.from(a.logdet_K);
  fin.A = U.table<double>([&](int u) { return std::exp(a.logA[u]); });
  fin.lambda0 = U.from(a.lambda0);
  fin.out_host = U.of(&gpfit_ctx::scal_host, S_ELBO);
  fin.info_V_host = U.of(&gpfit_ctx::info_host, INFO_V); fin.info_K_host = U.of(&gpfit_ctx::info_host, INFO_K);
  GP_TRY(launch_elbo_finish_group(fin, s));
  GP_HIP(hipStreamSynchronize(s));
  for (int u = 0; u < nu; ++u) {
    for (int i = 0; i < ELBO_OUT; ++i) a.out_host[(size_t)u * ELBO_OUT + i] = ctxs[u]->scal_host[S_ELBO + i];
    a.info_host[2 * u] = ctxs[u]->info_host[INFO_V];
    a.info_host[2 * u + 1] = ctxs[u]->info_host[INFO_K];
  }
  return 0;
}

extern "C" {

int gpfit_elbo(gpfit_ctx* c, void* stream, const double* m, const double* V, int64_t ldv, const double* K, int64_t ldk,
               const double* Kinv, int64_t ldki, int64_t nb, int logdet_K_known, double logdet_K, const double* r,
               const double* f, const double* lam_m, int64_t N, double logA, double lambda0, double* out_host,
               int* info_host) {
  // the group of one (elbo_group_impl): a unit's numbers are the same alone and in any group
  GP_TRY(elbo_group_impl({"gpfit_elbo", &c, 1, stream, &m, &V, &ldv, &K, &ldk, &Kinv, &ldki, &nb, &logdet_K_known, &logdet_K,
                          &r, &f, &lam_m, N, &logA, &lambda0, out_host, info_host}));
  if (info_host[0] != 0) {
    set_error("gpfit_elbo: V is not positive definite");
    return info_host[0];
  }
  if (info_host[1] != 0) {
    set_error("gpfit_elbo: K_tilde is not positive definite");
    return info_host[1];
  }
  return 0;
}

int gpfit_elbo_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* const* m, const double* const* V,
                     const int64_t* ldv, const double* const* K, const int64_t* ldk, const double* const* Kinv,
                     const int64_t* ldki, const int64_t* nb, const int* logdet_K_known, const double* logdet_K,
                     const double* const* r, const double* const* f, const double* const* lam_m, int64_t N,
                     const double* logA, const double* lambda0, double* out_host, int* info_host) {
  return elbo_group_impl({"gpfit_elbo_batch", ctxs, n_units, stream, m, V, ldv, K, ldk, Kinv, ldki, nb, logdet_K_known, logdet_K,
                          r, f, lam_m, N, logA, lambda0, out_host, info_host});
}

int gpfit_potrf_append(gpfit_ctx* c, void* stream, double* L, int64_t ldl, double* Linv, int64_t ldi, int64_t n,
                       const double* kcol, double* logdet_inout_host, int* info_host) {
  if (!c || !L || !Linv || !kcol || n <= 0 || ldl <= n || ldi <= n) {
    set_error("gpfit_potrf_append: bad argument (the factors need room for row and column n: ld > n)");
    return -3;
  }
  GP_CTX_ENTER(c, "gpfit_potrf_append");
  hipStream_t s = (hipStream_t)stream;
  if (n + 1 > c->np_cap) {
    set_error("gpfit_potrf_append: matrix larger than the context capacity");
    return -3;
  }
  const int ni = (int)n;
  double* l = c->yv;       // L^-1 k
  double* w = c->bv;       // L^-T l
  GP_HIP(hipMemsetAsync(c->info, 0, 4 * sizeof(int), s));
  hipLaunchKernelGGL(append_trmv_kernel, dim3((ni + 3) / 4), dim3(256), 0, s, Linv, ldi, ni, kcol, l);
  hipLaunchKernelGGL(append_trmv_t_kernel, dim3((ni + 63) / 64), dim3(256), 0, s, Linv, ldi, ni, l, w, c->scal + S_APPEND);
  hipLaunchKernelGGL(append_write_kernel, dim3((ni + 256) / 256), dim3(256), 0, s, L, ldl, Linv, ldi, ni, l, w, kcol,
                     c->scal + S_APPEND, c->info + INFO_K);
  GP_HIP(hipGetLastError());
  GP_HIP(hipMemcpyAsync(c->scal_host + S_APPEND, c->scal + S_APPEND, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  GP_HIP(hipMemcpyAsync(c->info_host, c->info, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
  GP_HIP(hipStreamSynchronize(s));
  if (info_host) *info_host = c->info_host[INFO_K];
  if (c->info_host[INFO_K] != 0) {
    set_error("gpfit_potrf_append: the extended matrix is not positive definite");
    return c->info_host[INFO_K];
  }
  if (logdet_inout_host) *logdet_inout_host += 2.0 * std::log(c->scal_host[S_APPEND_LAMBDA]);
  return 0;
}

// The block step (k rows at once; skinny.hip has the two reductions over n), nine launches whatever n and k:
//   Y = L^-1 K12           slabs + sum   (the sum also writes L21 = Y^T and zeroes columns n .. of the rows above)
//   S = K22 - Y^T Y        slabs + sum   (into a 128-tile with a unit diagonal behind k)
//   L22, L22^-1            the register-resident leaf on that tile (info_base = n: pivot j reports n + j + 1; the padding
//                          pivots are 1 and never reported)
//   W = L^-T Y             slabs + sum   (the triangular extent only)
//   [L^-1]21 = -L22^-1 W^T one slab (the reduction is k <= 128 long), stored transposed and negated as it is formed
//   the two k x k diagonal blocks and the log-det
// Work matrices: Tmp (partials), TmpV (Y), Kbuf (W), Abuf / Lbuf / Libuf (the three tiles) -- none of them carries
// anything between calls (Vbuf, LVbuf and the lv_valid state are not touched).
int gpfit_potrf_append_block(gpfit_ctx* c, void* stream, double* L, int64_t ldl, double* Linv, int64_t ldi, int64_t n,
                             int64_t k, const double* Kcols, int64_t ldk, double* logdet_inout_host, int* info_host) {
  auto refuse = [&](const std::string& why) {
    set_error("gpfit_potrf_append_block: " + why);
    return -3;
  };
  if (!c || !L || !Linv || !Kcols) return refuse("bad argument: null context or operand");
  if (n < 1) return refuse("bad argument: n < 1");
  if (k < 1 || k > SKINNY_LD) return refuse("k = " + std::to_string(k) + " is not within 1 .. " + std::to_string(SKINNY_LD));
  if (ldl < n + k || ldi < n + k || ldk < k)
    return refuse("bad argument: the factors need room for rows and columns n .. n + k - 1 (ldl, ldi >= n + k; ldk >= k)");
  GP_CTX_ENTER(c, "gpfit_potrf_append_block");
  if (n + k > c->np_cap) return refuse("matrix larger than the context capacity");
  hipStream_t s = (hipStream_t)stream;
  const int ni = (int)n, ki = (int)k;
  const int nslab = skinny_slabs(ni);
  const int64_t cap = (int64_t)c->np_cap * c->np_cap, pz = (int64_t)ni * SKINNY_LD;
  if (nslab * pz > cap || nslab * (int64_t)ki * SKINNY_LD > cap) return refuse("the partials do not fit the context's work matrix");
  double *P = c->Tmp, *Y = c->TmpV, *W = c->Kbuf, *St = c->Abuf, *Lt = c->Lbuf, *Lit = c->Libuf;
  GP_HIP(hipMemsetAsync(c->info, 0, 4 * sizeof(int), s));
  SkinnyArgs g{};
  SkinnySumArgs r{};
  g.alpha = 1.0; g.kc = ki;
  r.P = P; r.kc = ki; r.L = L; r.ldl = ldl; r.Li = Linv; r.ldi = ldi; r.n = ni; r.Kc = Kcols; r.ldk = ldk;
  // Y = L^-1 K12
  g.A = Linv; g.sam = ldi; g.sar = 1; g.tri = 1; g.M = ni; g.K = ni;
  g.B = Kcols; g.sbr = ldk; g.sbc = 1;
  g.O = P; g.soz = pz; g.som = SKINNY_LD; g.soc = 1;
  GP_TRY(launch_skinny_slabs(g, s));
  r.pz = pz; r.M = ni; r.nslab = nslab; r.tri = 1; r.mode = SKINNY_SUM_ROWS; r.dst = Y;
  GP_TRY(launch_skinny_sum(r, s));
  // S = K22 - Y^T Y
  g.A = Y; g.sam = 1; g.sar = SKINNY_LD; g.tri = 0; g.M = ki; g.K = ni;
  g.B = Y; g.sbr = SKINNY_LD; g.sbc = 1;
  g.soz = (int64_t)ki * SKINNY_LD;
  GP_TRY(launch_skinny_slabs(g, s));
  r.pz = g.soz; r.M = ki; r.tri = 0; r.mode = SKINNY_SUM_SCHUR; r.dst = St;
  GP_TRY(launch_skinny_sum(r, s));
  // L22 and its inverse
  LeafBatchT<double> bt{};
  bt.A[0] = St; bt.L[0] = Lt; bt.Li[0] = Lit; bt.info[0] = c->info + INFO_K;
  bt.lda = bt.ldl = bt.ldi = SKINNY_LD; bt.info_base = ni; bt.n = 1;
  GP_TRY(launch_chol_leaf_batch(bt, s));
  // W = L^-T Y
  g.A = Linv; g.sam = 1; g.sar = ldi; g.tri = 2; g.M = ni; g.K = ni;
  g.soz = pz;
  GP_TRY(launch_skinny_slabs(g, s));
  r.pz = pz; r.M = ni; r.tri = 2; r.mode = SKINNY_SUM_PLAIN; r.dst = W;
  GP_TRY(launch_skinny_sum(r, s));
  // [L^-1]21 = -L22^-1 W^T: out(m = column j, c = row a) = -sum_b W[j][b] L22^-1[a][b]
  g.A = W; g.sam = SKINNY_LD; g.sar = 1; g.tri = 0; g.M = ni; g.K = ki;
  g.B = Lit; g.sbr = 1; g.sbc = SKINNY_LD;
  g.O = Linv + n * ldi; g.soz = 0; g.som = 1; g.soc = ldi; g.alpha = -1.0;
  GP_TRY(launch_skinny_slabs(g, s));
  GP_TRY(launch_append_block_finish(Lt, Lit, L, ldl, Linv, ldi, ni, ki, c->scal + S_APPEND_LOGDET, s));
  GP_HIP(hipMemcpyAsync(c->scal_host + S_APPEND_LOGDET, c->scal + S_APPEND_LOGDET, sizeof(double), hipMemcpyDeviceToHost, s));
  GP_HIP(hipMemcpyAsync(c->info_host, c->info, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
  GP_HIP(hipStreamSynchronize(s));
  if (info_host) *info_host = c->info_host[INFO_K];
  if (c->info_host[INFO_K] != 0) {
    set_error("gpfit_potrf_append_block: the extended matrix is not positive definite");
    return c->info_host[INFO_K];
  }
  if (logdet_inout_host) *logdet_inout_host += c->scal_host[S_APPEND_LOGDET];
  return 0;
}

int gpfit_potrf(gpfit_ctx* c, void* stream, const double* A, int64_t lda, int64_t n, double* L, int64_t ldl,
                double* Linv, int64_t ldi, double* logdet_host, int* info_host) {
  if (!c || !A || n <= 0) {
    set_error("gpfit_potrf: bad argument");
    return -3;
  }
  GP_CTX_ENTER(c, "gpfit_potrf");
  hipStream_t s = (hipStream_t)stream;
  const int np = (int)round_up(n, TILE);
  if (np > c->np_cap) {
    set_error("gpfit_potrf: matrix larger than the context capacity");
    return -3;
  }
  const int64_t ld = np;
  GP_HIP(hipMemsetAsync(c->info, 0, 4 * sizeof(int), s));
  GP_TRY(launch_pack_lower(A, lda, (int)n, c->Kbuf, ld, np, s));
  const CholBatchT<double> b = one_chain(c, ld);
  GP_TRY(potrf_lockstep(b, 0, np, Linv != nullptr ? 1u : 0u, main_lane(c, s)));
  GP_TRY(launch_logdet(c->Lbuf, ld, (int)n, c->scal + S_LOGDET_K, s));
  if (L) GP_TRY(launch_unpack_tri(c->Lbuf, ld, (int)n, L, ldl, s));
  if (Linv) GP_TRY(launch_unpack_tri(c->Libuf, ld, (int)n, Linv, ldi, s));
  GP_HIP(hipMemcpyAsync(c->scal_host, c->scal, 8 * sizeof(double), hipMemcpyDeviceToHost, s));
  GP_HIP(hipMemcpyAsync(c->info_host, c->info, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
  GP_HIP(hipStreamSynchronize(s));
  if (logdet_host) *logdet_host = c->scal_host[S_LOGDET_K];
  if (info_host) *info_host = c->info_host[INFO_K];
  if (c->info_host[INFO_K] != 0) {
    set_error("gpfit_potrf: matrix is not positive definite");
    return c->info_host[INFO_K];
  }
  return 0;
}

int gpfit_estep(gpfit_ctx* c, void* stream, const double* K, int64_t ldk, int64_t N, const double* r,
                const double* m, const double* f, double logA, double* m_new, double* V_new, int64_t ldv) {
  if (!c || !K || !r || !m || !f || !m_new || !V_new || N <= 0) {
    set_error("gpfit_estep: bad argument");
    return -3;
  }
  GP_CTX_ENTER(c, "gpfit_estep");
  hipStream_t s = (hipStream_t)stream;
  const int n = (int)N, np = (int)round_up(N, TILE);
  if (np > c->np_cap) {
    set_error("gpfit_estep: problem larger than the context capacity");
    return -3;
  }
  const int64_t ld = np;
  const double A = std::exp(logA);
  double* sv = c->yv;
  double* rhs = c->bv;
  GP_HIP(hipMemsetAsync(c->info, 0, 4 * sizeof(int), s));
  GP_TRY(launch_estep_prep(f, r, m, n, np, A, sv, rhs, s));
  // M = I + S K S (lower), SK = S K (dense), Kl = K (lower)
  GP_TRY(launch_estep_build(K, ldk, n, np, sv, c->Kbuf, c->Zbuf, c->Wbuf, ld, s));
  const Lane lane = main_lane(c, s);
  const Units one = Units::all(&c, 1);
  GP_TRY(full_update_factor(one, np, lane));
  GP_TRY(full_update_products(one, np, lane));
  // m_new = V (A^2 f o m + A (r - f))                                utils.py:1431
  GP_TRY(launch_symv_lower(c->Wbuf, ld, n, rhs, c->tvec, s));
  GP_HIP(hipMemcpyAsync(m_new, c->tvec, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
  GP_TRY(launch_unpack_sym(c->Wbuf, ld, n, V_new, ldv, s));  // symmetric by construction (utils.py:1438)
  GP_HIP(hipMemcpyAsync(c->info_host, c->info, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
  GP_HIP(hipStreamSynchronize(s));
  if (c->info_host[INFO_K] != 0) {
    set_error("gpfit_estep: I + S K S is not positive definite (is K_tilde symmetric positive definite?)");
    return c->info_host[INFO_K];
  }
  return 0;
}

int gpfit_estep_projected(gpfit_ctx* c, void* stream, const double* a, int64_t lda, const double* aL, int64_t ldal,
                          const double* L, int64_t ldl, int64_t N, int64_t nb, const double* r, const double* m,
                          const double* f, double logA, double* m_new, double* V_new, int64_t ldv, const double* kv0,
                          double* lam_m_out, double* lam_var_out) {
  const bool want_moments = kv0 && lam_m_out && lam_var_out;
  if (!c || !a || !aL || !L || !r || !m || !f || !m_new || !V_new || N <= 0 || nb <= 0 || lda < nb || ldal < nb ||
      ldl < nb || ldv < nb || (!want_moments && (kv0 || lam_m_out || lam_var_out))) {
    set_error("gpfit_estep_projected: bad argument");
    return -3;
  }
  GP_CTX_ENTER(c, "gpfit_estep_projected");
  hipStream_t s = (hipStream_t)stream;
  const ProjStep w = proj_step(c, s, N, nb);
  if (w.nrows > c->np_cap || w.npc > c->np_cap) {
    set_error("gpfit_estep_projected: problem larger than the context capacity");
    return -3;
  }
  c->lv_valid = false; c->lv32_valid = false;   // the V work matrices are reused
  GP_HIP(hipMemsetAsync(c->info, 0, 4 * sizeof(int), s));
  GP_TRY(proj_step_w(w, a, lda, aL, ldal, r, m, f, std::exp(logA), want_moments));
  GP_TRY(potrf_lockstep(one_chain(c, w.ld), 0, w.npc, 1u, w.lane));
  // m_new = L W^-1 (a L)^T u
  GP_TRY(proj_step_mean(w, L, ldl));
  // V_new = P P^T, P = L L_W^-T  (= (K~^-1 + G)^-1 = solve(I + K~ G, K~), utils.py:1430)
  GP_TRY(proj_step_cov(w, c->Libuf));
  GP_HIP(hipMemcpyAsync(m_new, w.mo, (size_t)w.k * sizeof(double), hipMemcpyDeviceToDevice, s));
  GP_TRY(launch_unpack_sym(w.V, w.ld, w.k, V_new, ldv, s));   // symmetric by construction (utils.py:1438)
  if (want_moments) {
    // the moments of lambda the caller evaluates next (utils.py:1090, 1101), from Z = aL L_W^-T: a V_new a^T = Z Z^T
    GP_TRY(product(w.lane, {w.nrows, w.npc, w.npc}, 1.0, plain(w.M(w.aLp)), trans(tril(w.M(c->Libuf))), into(w.M(w.Zm))));
    GP_TRY(launch_estep_proj_moments(w.Zm, w.ld, w.k, w.z1, kv0, w.n, lam_m_out, lam_var_out, s));
  }
  GP_HIP(hipMemcpyAsync(c->info_host, c->info, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
  GP_HIP(hipStreamSynchronize(s));
  if (c->info_host[INFO_K] != 0) {
    set_error("gpfit_estep_projected: I + L^T G L is not positive definite (NaN or negative firing rates?)");
    return c->info_host[INFO_K];
  }
  return 0;
}

// The damped update (header: gpfit_estep_projected_damped).  Work matrices beyond those of the full step, all ld = npc:
//   Zbuf  L^-1 packed (lower, identity padding)     Abuf  V symmetric, identity padding     Wbuf  L^-1 V
//   Vbuf  P = L^-1 V L^-T (lower tiles): the V chain's matrix, factored beside W1 (the K chain) in one lock-step call
//   Cos   the copy of W1 taken before its factorisation, then W_a = (1 - a) P^-1 + a W1 in place (the product's beta)
// Zbuf, Abuf and Wbuf are free again once P is formed: the full step's stages use them as they always do (Lp, P, V).
// W_a is factored on the K chain's L / L^-1 / scratch matrices, after the mean has read W1's inverse factor there.
int gpfit_estep_projected_damped(gpfit_ctx* c, void* stream, const double* a, int64_t lda, const double* aL, int64_t ldal,
                                 const double* L, int64_t ldl, const double* Linv, int64_t ldli, const double* V,
                                 int64_t ldv_in, int64_t N, int64_t nb, const double* r, const double* m, const double* f,
                                 double logA, double alpha, double* m_new, double* V_new, int64_t ldv, int* info_v_host) {
  const Refuse refuse{"gpfit_estep_projected_damped"};
  if (!c || !a || !aL || !L || !Linv || !V || !r || !m || !f || !m_new || !V_new)
    return refuse("bad argument: null context or operand");
  if (N <= 0 || nb <= 0) return refuse("bad argument: N and nb must be positive");
  if (lda < nb || ldal < nb || ldl < nb || ldli < nb || ldv_in < nb || ldv < nb)
    return refuse("bad argument: a leading dimension is smaller than nb");
  if (!std::isfinite(alpha) || !(alpha > 0.0) || alpha > 1.0)
    return refuse("bad argument: the step size alpha must lie in (0, 1]");
  GP_CTX_ENTER(c, "gpfit_estep_projected_damped");
  hipStream_t s = (hipStream_t)stream;
  const ProjStep w = proj_step(c, s, N, nb);
  if (w.nrows > c->np_cap || w.npc > c->np_cap) return refuse("problem larger than the context capacity");
  const int npc = w.npc;
  const int64_t ld = w.ld;
  double *Lip = c->Zbuf, *Vs = c->Abuf, *LiV = c->Wbuf, *Wa = c->Cos, *mpad = c->dq1;
  c->lv_valid = false; c->lv32_valid = false;   // the V work matrices are reused
  GP_HIP(hipMemsetAsync(c->info, 0, 4 * sizeof(int), s));
  GP_TRY(proj_step_w(w, a, lda, aL, ldal, r, m, f, std::exp(logA), false));
  GP_HIP(hipMemcpyAsync(Wa, c->Kbuf, (size_t)npc * npc * sizeof(double), hipMemcpyDeviceToDevice, s));   // W1, kept
  // P = L^-1 V L^-T, lower tiles, identity on the padding (positive definite iff V is)
  GP_TRY(launch_pack_tri(Linv, ldli, w.k, Lip, ld, npc, s));
  GP_TRY(launch_pack_tri(V, ldv_in, w.k, Vs, ld, npc, s));
  GP_TRY(launch_symmetrize(Vs, ld, npc, s));
  GP_TRY(product(w.lane, {npc, npc, npc}, 1.0, plain(tril(w.M(Lip))), plain(w.M(Vs)), into(w.M(LiV))));
  GP_TRY(product(w.lane, {npc, npc, npc}, 1.0, plain(w.M(LiV)), trans(tril(w.M(Lip))), into_lower(w.M(c->Vbuf))));
  // W1 and P in lock step, both with their full inverse factors
  CholBatchT<double> two;
  add_k_chain(two, c);
  add_v_chain(two, c);
  two.ld = ld;
  GP_TRY(potrf_lockstep(two, 0, npc, 3u, w.lane));
  // m_new = (1 - a) m + a L W1^-1 (a L)^T u: the full step's mean, damped.  The same vector as utils.py:1436, since
  // m - (I + K~ G)^-1 (m - K~ g) = (I + K~ G)^-1 K~ (G m + g)
  GP_TRY(proj_step_mean(w, L, ldl));
  GP_HIP(hipMemsetAsync(mpad, 0, (size_t)npc * sizeof(double), s));
  GP_HIP(hipMemcpyAsync(mpad, m, (size_t)w.k * sizeof(double), hipMemcpyDeviceToDevice, s));
  GP_TRY(launch_axpby_block<double>(w.mo, ld, mpad, ld, 1, npc, alpha, 1.0 - alpha, s));
  // W_a = (1 - a) P^-1 + a W1 (lower tiles), P^-1 = L_P^-T L_P^-1; then its factor with the full inverse
  GP_TRY(product(w.lane, {npc, npc, npc}, 1.0 - alpha, trans(tril(w.M(c->LiVbuf))), plain(tril(w.M(c->LiVbuf))),
                 into_lower(w.M(Wa), alpha)));
  CholBatchT<double> one;
  add_chain(one, Wa, c->Lbuf, c->Libuf, c->Tmp, c->info + INFO_K);
  one.ld = ld;
  GP_TRY(potrf_lockstep(one, 0, npc, 1u, w.lane));
  // V_new = P P^T, P = L L_Wa^-T  (V_new^-1 = (1 - a) V^-1 + a (K~^-1 + G) = L^-T W_a L^-1)
  GP_TRY(proj_step_cov(w, c->Libuf));
  GP_HIP(hipMemcpyAsync(m_new, w.mo, (size_t)w.k * sizeof(double), hipMemcpyDeviceToDevice, s));
  GP_TRY(launch_unpack_sym(w.V, ld, w.k, V_new, ldv, s));   // symmetric by construction
  GP_HIP(hipMemcpyAsync(c->info_host, c->info, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
  GP_HIP(hipStreamSynchronize(s));
  if (info_v_host) *info_v_host = c->info_host[INFO_V];
  if (c->info_host[INFO_V] != 0) {
    set_error("gpfit_estep_projected_damped: V is not positive definite (the damped update needs a positive definite V)");
    return c->info_host[INFO_V];
  }
  if (c->info_host[INFO_K] != 0) {
    set_error("gpfit_estep_projected_damped: I + L^T G L is not positive definite (NaN or negative firing rates?)");
    return c->info_host[INFO_K];
  }
  return 0;
}

int gpfit_fparam_eval(gpfit_ctx* c, void* stream, const double* lam_m, const double* lam_var, const double* r,
                      int64_t N, double logA, int closed_form_lambda0, double lambda0_in, double* f_out,
                      double* out_host) {
  if (!c || !lam_m || !lam_var || !r || !out_host || N <= 0) {
    set_error("gpfit_fparam_eval: bad argument");
    return -3;
  }
  GP_CTX_ENTER(c, "gpfit_fparam_eval");
  hipStream_t s = (hipStream_t)stream;
  // the seven results go straight to the context's pinned, device-mapped scalars (no copy command behind the kernel:
  // the L-BFGS of the rate parameters calls this ~6 times per E-step and waits for every answer)
  GP_TRY(launch_fparam(lam_m, lam_var, r, (int)N, std::exp(logA), closed_form_lambda0, lambda0_in, f_out,
                       c->scal_host + S_FPARAM, s));
  GP_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < 7; ++i) out_host[i] = c->scal_host[S_FPARAM + i];
  return 0;
}

int gpfit_fparam_lbfgs(gpfit_ctx* c, void* stream, const double* lam_m, const double* lam_var, const double* r,
                       int64_t N, double logA0, int lambda0_mode, double lambda0_fixed, int max_iter,
                       int history_size, double lr, double tol_grad, double tol_change, double* f_out,
                       double* out_host) {
  if (!c || !lam_m || !lam_var || !r || !out_host || N <= 0 || N > INT32_MAX) {
    set_error("gpfit_fparam_lbfgs: bad argument");
    return -3;
  }
  Lbfgs1dConfig cfg;
  GP_TRY(fparam_lbfgs_config("gpfit_fparam_lbfgs", max_iter, history_size, lr, tol_grad, tol_change, &cfg));
  GP_CTX_ENTER(c, "gpfit_fparam_lbfgs");
  hipStream_t s = (hipStream_t)stream;
  // one launch, one wait: the nine results go straight to pinned, device-mapped scalars no other entry point uses
  GP_TRY(launch_fparam_lbfgs(lam_m, lam_var, r, (int)N, logA0, lambda0_mode ? 1 : 0, lambda0_fixed, cfg, f_out,
                             c->scal_host + S_LBFGS, s));
  GP_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < 9; ++i) out_host[i] = c->scal_host[S_LBFGS + i];
  return 0;
}

// ONE body for gpfit_estep_chain (the group of one) and gpfit_estep_chain_batch: every step runs the update of
// gpfit_estep_projected, product for product on the same work vectors and matrices, and its moments, inside the
// skeleton of ChainCall.  The factorisations of all units are one lock-step recursion, every product goes through
// product on the list of units, every small kernel is its unit-batched form: a unit runs the same products in the same
// order with the same reduction order whatever else is in the group, so its outputs have the same bits alone and in any
// group.
static int estep_chain_group_impl(ChainCall call, const double* const* a, const int64_t* lda, const double* const* aL,
                                  const int64_t* ldal, const double* const* L, const int64_t* ldl, const int64_t* nb) {
  gpfit_ctx* const* ctxs = call.ctxs;
  const int nrows = (int)round_up(call.N, TILE);
  GP_TRY(call.admit(
      a && lda && aL && ldal && L && ldl && nb, [&](int u) { return a[u] && aL[u] && L[u]; },
      [&](int u) { return nb[u] > 0 && lda[u] >= nb[u] && ldal[u] >= nb[u] && ldl[u] >= nb[u] && call.ldv[u] >= nb[u]; },
      [&](int u) -> std::string {
        // the recursion's split depends on the padded size: only equal padded sizes give the bits of the single call
        if (round_up(nb[u], TILE) != round_up(nb[0], TILE))
          return "round_up(nb, 128) = " + std::to_string(round_up(nb[u], TILE)) + " differs from unit 0's " +
                 std::to_string(round_up(nb[0], TILE)) + " (group the units by padded size)";
        if (nrows > ctxs[u]->np_cap || round_up(nb[u], TILE) > ctxs[u]->np_cap) return "problem larger than the context capacity";
        return std::string();
      }));
  hipStream_t s = (hipStream_t)call.stream;
  const Units U = Units::all(ctxs, call.n_units);
  const int nu = U.cnt, npc = (int)round_up(nb[0], TILE);
  const int64_t ld = npc;
  ChainGroupT g = call.group(nrows, npc);
  g.nb = U.table<int>([&](int u) { return (int)nb[u]; });
  for (int u = 0; u < nu; ++u) {
    g.kmax = std::max(g.kmax, g.nb[u]);
    ctxs[u]->lv_valid = false; ctxs[u]->lv32_valid = false;   // the V work matrices are reused
  }
  g.a = U.from(a); g.aL = U.from(aL); g.L = U.from(L); g.lda = U.from(lda); g.ldal = U.from(ldal); g.ldl = U.from(ldl);
  // the work vectors and matrices of gpfit_estep_projected
  g.sv = U.of(&gpfit_ctx::yv); g.u = U.of(&gpfit_ctx::bv); g.t2 = U.of(&gpfit_ctx::tvec); g.z1 = U.of(&gpfit_ctx::mpad);
  g.z = U.of(&gpfit_ctx::rpad); g.mo = U.of(&gpfit_ctx::hvec); g.Y = U.of(&gpfit_ctx::Tbuf); g.Lp = U.of(&gpfit_ctx::Wbuf);
  g.Vw = U.of(&gpfit_ctx::Zbuf); g.part = U.of(&gpfit_ctx::TmpV); g.aLp = U.of(&gpfit_ctx::LiVbuf); g.Zm = U.of(&gpfit_ctx::Cos);
  g.W = U.of(&gpfit_ctx::Kbuf); g.Li = U.of(&gpfit_ctx::Libuf); g.trmv_part = U.of(&gpfit_ctx::trmv_part);
  CholBatchT<double> cb;
  for (int u = 0; u < nu; ++u) add_k_chain(cb, ctxs[u]);
  cb.ld = ld;
  const Lane lane = main_lane(ctxs[0], s);   // every launch on the caller's stream with the leader's workspace
  const Mat<double> Y = U.mats(&gpfit_ctx::Tbuf, ld), W = U.mats(&gpfit_ctx::Kbuf, ld), Lp = U.mats(&gpfit_ctx::Wbuf, ld),
                    Li = U.mats(&gpfit_ctx::Libuf, ld), P = U.mats(&gpfit_ctx::Abuf, ld), Vw = U.mats(&gpfit_ctx::Zbuf, ld),
                    aLp = U.mats(&gpfit_ctx::LiVbuf, ld), Zm = U.mats(&gpfit_ctx::Cos, ld);
  return call.run(
      g,
      [&](int step) -> int {
        // L does not change over the chain: packed once
        if (step == 0) GP_TRY(launch_pack_lower_group(nu, g.L, g.ldl, g.nb, g.Lp, ld, npc, s));
        // m and f are updated in place: this kernel is the only reader of both in a step and runs before any of the
        // step's writers (the gated copy into m, the optimiser's rate), all on one stream
        GP_TRY(launch_estep_proj_rows_chain_group(g, step, s));
        GP_TRY(launch_estep_proj_scale_group(g, s));
        GP_TRY(launch_reduce_slices_group(nu, g.part, npc, nrows / 32, g.t2, npc, s));   // t2 = (a L)^T u
        // W = I + Y^T Y  (= I + L^T G L, G = A^2 a^T diag(f) a), lower tiles, identity on the padding
        GP_TRY(product(lane, {npc, npc, nrows}, 1.0, trans(Y), plain(Y), into_lower(W)));
        GP_TRY(launch_add_diag_group(nu, g.W, ld, npc, 1.0, s));
        return potrf_lockstep(cb, 0, npc, U.chains(), lane);
      },
      [&]() -> int {
        // m_new = L W^-1 (a L)^T u
        GP_TRY(launch_trmv_lower_group(nu, g.Li, ld, npc, g.t2, g.z1, s));
        GP_TRY(launch_trmv_lower_t_group(nu, g.Li, ld, npc, g.z1, g.z, g.trmv_part, s));
        GP_TRY(launch_trmv_lower_group(nu, g.Lp, ld, npc, g.z, g.mo, s));
        // V_new = P P^T, P = L L_W^-T
        GP_TRY(product(lane, {npc, npc, npc}, 1.0, plain(tril(Lp)), trans(tril(Li)), into(P)));
        return product(lane, {npc, npc, npc}, 1.0, plain(P), trans(P), into_lower(Vw));
      },
      [&]() -> int {
        // from Z = aL L_W^-T
        GP_TRY(product(lane, {nrows, npc, npc}, 1.0, plain(aLp), trans(tril(Li)), into(Zm)));
        return launch_estep_proj_moments_chain_group(g, s);
      });
}

// ONE body for gpfit_estep_chain_damped (the group of one) and gpfit_estep_chain_damped_batch: every step runs the update
// of gpfit_estep_projected_damped, stage for stage and product for product, then the moments of the committed state,
// inside the skeleton of ChainCall.  Per unit and step, on the 13 work matrices (all ld = npc; nothing is kept from one
// step to the next, L^-1, L and aL are packed again from the caller's arrays):
//   Tbuf   Y = diag(s) aL                      -> the second copy of W1 (Y is dead once W1 is formed)
//   TmpV   the slice sums of aL^T u            -> scratch of the V chain
//   Kbuf   W1 = I + Y^T Y, the K chain's matrix (destroyed by it)          -> aL zero-padded, for the moments
//   Cos    the first copy of W1                -> W_a = (1 - a) P^-1 + a W1 in place, factored by the second recursion
//   Zbuf   L^-1 packed                         -> V_new (lower tiles), the source of the gated commit
//   Abuf   V symmetric, identity padding       -> L L_Wa^-T
//   Wbuf   L^-1 V                              -> L packed (behind the first recursion)
//   Vbuf   P = L^-1 V L^-T, the V chain's matrix (destroyed by it)         -> Z = aL L_Wa^-T, for the moments
//   Lbuf / Libuf / Tmp    the K chain: W1's factor and inverse factor (read by the mean), then W_a's
//   LVbuf / LiVbuf        the V chain: P's factor and inverse factor
// The first recursion factors W1 and P of all units in lock step (2 x units chains).  Its info word of the K chain is
// latched into the record, and stops the unit when non-zero, before the second recursion reports into the same word.
// The fallback is decided on the device, per unit, by the info word of the V chain (zeroed by the step's first kernel,
// written by the first recursion only): non-zero = V is not positive definite = this update is the full step.  Such a
// unit keeps the full step's mean (the blend skips it), and behind the blend of W_a -- which ran for it like for the
// others, on whatever the failed chain left -- the whole of W_a is overwritten with the second copy of W1, so that its
// second factorisation is W1's and the group stays in lock step; its record's slot 10 reads 2.  No launch, grid or
// operand of the other units depends on it.
static int estep_chain_damped_group_impl(ChainCall call, const double* const* a, const int64_t* lda, const double* const* aL,
                                         const int64_t* ldal, const double* const* L, const int64_t* ldl,
                                         const double* const* Linv, const int64_t* ldli, const int64_t* nb, double alpha) {
  gpfit_ctx* const* ctxs = call.ctxs;
  const int nrows = (int)round_up(call.N, TILE);
  if (!std::isfinite(alpha) || !(alpha > 0.0) || alpha > 1.0)
    return Refuse{call.name}("bad argument: the step size alpha must lie in (0, 1]");
  GP_TRY(call.admit(
      a && lda && aL && ldal && L && ldl && Linv && ldli && nb, [&](int u) { return a[u] && aL[u] && L[u] && Linv[u]; },
      [&](int u) {
        return nb[u] > 0 && lda[u] >= nb[u] && ldal[u] >= nb[u] && ldl[u] >= nb[u] && ldli[u] >= nb[u] && call.ldv[u] >= nb[u];
      },
      [&](int u) -> std::string {
        // the recursion's split depends on the padded size: only equal padded sizes give the bits of the single call
        if (round_up(nb[u], TILE) != round_up(nb[0], TILE))
          return "round_up(nb, 128) = " + std::to_string(round_up(nb[u], TILE)) + " differs from unit 0's " +
                 std::to_string(round_up(nb[0], TILE)) + " (group the units by padded size)";
        if (nrows > ctxs[u]->np_cap || round_up(nb[u], TILE) > ctxs[u]->np_cap) return "problem larger than the context capacity";
        return std::string();
      }));
  hipStream_t s = (hipStream_t)call.stream;
  const Units U = Units::all(ctxs, call.n_units);
  const int nu = U.cnt, npc = (int)round_up(nb[0], TILE);
  const int64_t ld = npc, count = (int64_t)npc * npc;
  ChainGroupT g = call.group(nrows, npc);
  g.nb = U.table<int>([&](int u) { return (int)nb[u]; });
  for (int u = 0; u < nu; ++u) {
    g.kmax = std::max(g.kmax, g.nb[u]);
    ctxs[u]->lv_valid = false; ctxs[u]->lv32_valid = false;   // the V work matrices are reused
  }
  g.a = U.from(a); g.aL = U.from(aL); g.L = U.from(L); g.lda = U.from(lda); g.ldal = U.from(ldal); g.ldl = U.from(ldl);
  // the work vectors of gpfit_estep_projected; the work matrices as laid out above (aLp stays null: no copy of aL here)
  g.sv = U.of(&gpfit_ctx::yv); g.u = U.of(&gpfit_ctx::bv); g.t2 = U.of(&gpfit_ctx::tvec); g.z1 = U.of(&gpfit_ctx::mpad);
  g.z = U.of(&gpfit_ctx::rpad); g.mo = U.of(&gpfit_ctx::hvec); g.Y = U.of(&gpfit_ctx::Tbuf); g.Lp = U.of(&gpfit_ctx::Wbuf);
  g.Vw = U.of(&gpfit_ctx::Zbuf); g.part = U.of(&gpfit_ctx::TmpV); g.Zm = U.of(&gpfit_ctx::Vbuf);
  g.W = U.of(&gpfit_ctx::Kbuf); g.Li = U.of(&gpfit_ctx::Libuf); g.trmv_part = U.of(&gpfit_ctx::trmv_part);
  const PerUnit<const int*> info_v = U.table<const int*>([&](int u) { return ctxs[u]->info + INFO_V; });
  call.full_step = info_v;
  const PerUnit<double*> W1c = U.of(&gpfit_ctx::Tbuf), Wa_t = U.of(&gpfit_ctx::Cos), Lip_t = U.of(&gpfit_ctx::Zbuf),
                         Vs_t = U.of(&gpfit_ctx::Abuf), aLp_t = U.of(&gpfit_ctx::Kbuf);
  const PerUnit<const double*> Linv_t = U.from(Linv), Vin_t = U.table<const double*>([&](int u) { return call.V[u]; });
  const PerUnit<int64_t> ldli_t = U.from(ldli);
  CholBatchT<double> two, one;   // W1 and P of every unit; then W_a of every unit on the K chain's matrices
  for (int u = 0; u < nu; ++u) {
    add_k_chain(two, ctxs[u]);
    add_v_chain(two, ctxs[u]);
    add_chain(one, ctxs[u]->Cos, ctxs[u]->Lbuf, ctxs[u]->Libuf, ctxs[u]->Tmp, ctxs[u]->info + INFO_K);
  }
  two.ld = one.ld = ld;
  const uint32_t all_two = (uint32_t)((1ull << (2 * nu)) - 1ull);
  const Lane lane = main_lane(ctxs[0], s);   // every launch on the caller's stream with the leader's workspace
  const Mat<double> Y = U.mats(&gpfit_ctx::Tbuf, ld), W = U.mats(&gpfit_ctx::Kbuf, ld), Lp = U.mats(&gpfit_ctx::Wbuf, ld),
                    Li = U.mats(&gpfit_ctx::Libuf, ld), P = U.mats(&gpfit_ctx::Abuf, ld), Vw = U.mats(&gpfit_ctx::Zbuf, ld),
                    Lip = U.mats(&gpfit_ctx::Zbuf, ld), Vs = U.mats(&gpfit_ctx::Abuf, ld), LiV = U.mats(&gpfit_ctx::Wbuf, ld),
                    Pv = U.mats(&gpfit_ctx::Vbuf, ld), LiP = U.mats(&gpfit_ctx::LiVbuf, ld), Wa = U.mats(&gpfit_ctx::Cos, ld),
                    aLp = U.mats(&gpfit_ctx::Kbuf, ld), Zm = U.mats(&gpfit_ctx::Vbuf, ld);
  return call.run(
      g,
      [&](int step) -> int {
        // m and f are updated in place: of f this kernel is the only reader in a step, of m it and the blend below, and
        // both run before any of the step's writers (the gated copy into m, the optimiser's rate), all on one stream
        GP_TRY(launch_estep_proj_rows_chain_group(g, step, s));
        GP_TRY(launch_estep_proj_scale_group(g, s));
        GP_TRY(launch_reduce_slices_group(nu, g.part, npc, nrows / 32, g.t2, npc, s));   // t2 = (a L)^T u
        GP_TRY(product(lane, {npc, npc, nrows}, 1.0, trans(Y), plain(Y), into_lower(W)));
        GP_TRY(launch_add_diag_group(nu, g.W, ld, npc, 1.0, s));
        GP_TRY(launch_chain_keep2_group(nu, g.W, Wa_t, W1c, count, s));   // W1, kept twice
        // P = L^-1 V L^-T, lower tiles, identity on the padding (positive definite iff V is); V: what the caller gave
        // (step 0) or what the last committed step left there
        GP_TRY(launch_pack_tri_group(nu, Linv_t, ldli_t, g.nb, Lip_t, ld, npc, s));
        GP_TRY(launch_pack_tri_group(nu, Vin_t, g.ldv, g.nb, Vs_t, ld, npc, s));
        GP_TRY(launch_symmetrize_group(nu, Vs_t, ld, npc, s));
        GP_TRY(product(lane, {npc, npc, npc}, 1.0, plain(tril(Lip)), plain(Vs), into(LiV)));
        GP_TRY(product(lane, {npc, npc, npc}, 1.0, plain(LiV), trans(tril(Lip)), into_lower(Pv)));
        // W1 and P in lock step, both with their full inverse factors
        GP_TRY(potrf_lockstep(two, 0, npc, all_two, lane));
        // W1's info word into the record (and the stop word) before the second recursion reports into the same word
        GP_TRY(launch_chain_info_group(g, step, s));
        // the full step's mean L W1^-1 (a L)^T u, then its blend with m (not for a unit that falls back)
        GP_TRY(launch_trmv_lower_group(nu, g.Li, ld, npc, g.t2, g.z1, s));
        GP_TRY(launch_trmv_lower_t_group(nu, g.Li, ld, npc, g.z1, g.z, g.trmv_part, s));
        GP_TRY(launch_pack_lower_group(nu, g.L, g.ldl, g.nb, g.Lp, ld, npc, s));
        GP_TRY(launch_trmv_lower_group(nu, g.Lp, ld, npc, g.z, g.mo, s));
        GP_TRY(launch_chain_damped_mean_group(g, info_v, alpha, s));
        // W_a = (1 - a) P^-1 + a W1 (lower tiles), P^-1 = L_P^-T L_P^-1; W1 itself where V was not positive definite
        GP_TRY(product(lane, {npc, npc, npc}, 1.0 - alpha, trans(tril(LiP)), plain(tril(LiP)), into_lower(Wa, alpha)));
        GP_TRY(launch_chain_damped_restore_group(nu, info_v, W1c, Wa_t, count, s));
        return potrf_lockstep(one, 0, npc, U.chains(), lane);
      },
      [&]() -> int {
        // V_new = P P^T, P = L L_Wa^-T
        GP_TRY(product(lane, {npc, npc, npc}, 1.0, plain(tril(Lp)), trans(tril(Li)), into(P)));
        return product(lane, {npc, npc, npc}, 1.0, plain(P), trans(P), into_lower(Vw));
      },
      [&]() -> int {
        // from Z = aL L_Wa^-T and the committed mean
        GP_TRY(launch_pad_copy_group(nu, g.aL, g.ldal, g.n, g.nb, aLp_t, ld, nrows, npc, s));
        GP_TRY(product(lane, {nrows, npc, npc}, 1.0, plain(aLp), trans(tril(Li)), into(Zm)));
        return launch_estep_damped_moments_chain_group(g, s);
      });
}

// ONE body for gpfit_estep_chain_full (the group of one) and gpfit_estep_chain_full_batch.  The full-rank chain: the
// update of gpfit_estep (full_update_factor / full_update_products) in place of the projected one, on the bookkeeping of
// the projected chain -- a ChainGroupT with nb = n, so that the init, the info word, the gated commits of m and V, the
// optimiser and the collect are the launches of ChainCall::run.  One lock-step recursion, every product on the list of
// units, every small kernel in its unit-batched form: the same bits alone and in any group.
static int estep_chain_full_group_impl(ChainCall call, const double* const* K, const int64_t* ldk) {
  gpfit_ctx* const* ctxs = call.ctxs;
  const int64_t N = call.N;
  const int n = (int)N, np = (int)round_up(N, TILE);
  GP_TRY(call.admit(
      K && ldk, [&](int u) { return K[u] != nullptr; }, [&](int u) { return ldk[u] >= N && call.ldv[u] >= N; },
      [&](int u) { return np > ctxs[u]->np_cap ? std::string("problem larger than the context capacity") : std::string(); }));
  hipStream_t s = (hipStream_t)call.stream;
  const Units U = Units::all(ctxs, call.n_units);
  const int nu = U.cnt;
  const int64_t ld = np;
  ChainGroupT g = call.group(np, np);
  g.kmax = n;
  g.nb = U.same(n);
  g.K = U.from(K); g.ldk = U.from(ldk);
  // the work vectors and matrices of gpfit_estep
  g.sv = U.of(&gpfit_ctx::yv); g.u = U.of(&gpfit_ctx::bv); g.mo = U.of(&gpfit_ctx::tvec);
  g.W = U.of(&gpfit_ctx::Kbuf); g.SK = U.of(&gpfit_ctx::Zbuf); g.Vw = U.of(&gpfit_ctx::Wbuf);
  const Lane lane = main_lane(ctxs[0], s);   // every launch on the caller's stream with the leader's workspace
  return call.run(
      g,
      [&](int step) -> int {
        // m and f are updated in place: this kernel is the only reader of both in a step and runs before any of the
        // step's writers (the gated copy into m, the optimiser's rate), all on one stream
        GP_TRY(launch_estep_prep_chain_group(g, step, s));
        // M = I + S K S (lower), SK = S K (dense), Kl = K (lower): Kl is overwritten by V, so it is rebuilt every step
        GP_TRY(launch_estep_build_group(g, s));
        return full_update_factor(U, np, lane);
      },
      [&]() -> int {
        GP_TRY(full_update_products(U, np, lane));
        return launch_symv_lower_group(nu, g.Vw, ld, n, g.u, g.mo, s);
      },
      [&]() -> int { return launch_estep_full_moments_chain_group(g, s); });
}

int gpfit_estep_chain(gpfit_ctx* c, void* stream, const double* a, int64_t lda, const double* aL, int64_t ldal,
                      const double* L, int64_t ldl, int64_t N, int64_t nb, const double* r, const double* kv0, double* m,
                      double* f, double* V_out, int64_t ldv, double* lam_m, double* lam_var, double logA0,
                      int lambda0_mode, double lambda0_fixed, int n_steps, int max_iter, int history_size, double lr,
                      double tol_grad, double tol_change, double* rec_host) {
  // the group of one (estep_chain_group_impl): a unit's numbers are the same alone and in any group
  return estep_chain_group_impl({"gpfit_estep_chain", &c, 1, stream, N, &r, &kv0, &m, &f, &V_out, &ldv, &lam_m, &lam_var, &logA0,
                                 lambda0_mode, &lambda0_fixed, n_steps, max_iter, history_size, lr, tol_grad, tol_change, rec_host},
                                &a, &lda, &aL, &ldal, &L, &ldl, &nb);
}

int gpfit_estep_chain_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* const* a, const int64_t* lda,
                            const double* const* aL, const int64_t* ldal, const double* const* L, const int64_t* ldl,
                            int64_t N, const int64_t* nb, const double* const* r, const double* const* kv0,
                            double* const* m, double* const* f, double* const* V, const int64_t* ldv,
                            double* const* lam_m, double* const* lam_var, const double* logA0, int lambda0_mode,
                            const double* lambda0_fixed, int n_steps, int max_iter, int history_size, double lr,
                            double tol_grad, double tol_change, double* rec_host) {
  return estep_chain_group_impl({"gpfit_estep_chain_batch", ctxs, n_units, stream, N, r, kv0, m, f, V, ldv, lam_m, lam_var, logA0,
                                 lambda0_mode, lambda0_fixed, n_steps, max_iter, history_size, lr, tol_grad, tol_change, rec_host},
                                a, lda, aL, ldal, L, ldl, nb);
}

int gpfit_estep_chain_damped(gpfit_ctx* c, void* stream, const double* a, int64_t lda, const double* aL, int64_t ldal,
                             const double* L, int64_t ldl, const double* Linv, int64_t ldli, int64_t N, int64_t nb,
                             const double* r, const double* kv0, double* m, double* f, double* V, int64_t ldv, double* lam_m,
                             double* lam_var, double logA0, double alpha, int lambda0_mode, double lambda0_fixed, int n_steps,
                             int max_iter, int history_size, double lr, double tol_grad, double tol_change, double* rec_host) {
  // the group of one (estep_chain_damped_group_impl): a unit's numbers are the same alone and in any group
  return estep_chain_damped_group_impl({"gpfit_estep_chain_damped", &c, 1, stream, N, &r, &kv0, &m, &f, &V, &ldv, &lam_m, &lam_var,
                                        &logA0, lambda0_mode, &lambda0_fixed, n_steps, max_iter, history_size, lr, tol_grad,
                                        tol_change, rec_host},
                                       &a, &lda, &aL, &ldal, &L, &ldl, &Linv, &ldli, &nb, alpha);
}

int gpfit_estep_chain_damped_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* const* a,
                                   const int64_t* lda, const double* const* aL, const int64_t* ldal, const double* const* L,
                                   const int64_t* ldl, const double* const* Linv, const int64_t* ldli, int64_t N,
                                   const int64_t* nb, const double* const* r, const double* const* kv0, double* const* m,
                                   double* const* f, double* const* V, const int64_t* ldv, double* const* lam_m,
                                   double* const* lam_var, const double* logA0, double alpha, int lambda0_mode,
                                   const double* lambda0_fixed, int n_steps, int max_iter, int history_size, double lr,
                                   double tol_grad, double tol_change, double* rec_host) {
  return estep_chain_damped_group_impl({"gpfit_estep_chain_damped_batch", ctxs, n_units, stream, N, r, kv0, m, f, V, ldv, lam_m,
                                        lam_var, logA0, lambda0_mode, lambda0_fixed, n_steps, max_iter, history_size, lr, tol_grad,
                                        tol_change, rec_host},
                                       a, lda, aL, ldal, L, ldl, Linv, ldli, nb, alpha);
}

int gpfit_estep_chain_full(gpfit_ctx* c, void* stream, const double* K, int64_t ldk, int64_t N, const double* r,
                           const double* kv0, double* m, double* f, double* V_out, int64_t ldv, double* lam_m,
                           double* lam_var, double logA0, int lambda0_mode, double lambda0_fixed, int n_steps,
                           int max_iter, int history_size, double lr, double tol_grad, double tol_change,
                           double* rec_host) {
  // the group of one (estep_chain_full_group_impl): a unit's numbers are the same alone and in any group
  return estep_chain_full_group_impl({"gpfit_estep_chain_full", &c, 1, stream, N, &r, &kv0, &m, &f, &V_out, &ldv, &lam_m, &lam_var,
                                      &logA0, lambda0_mode, &lambda0_fixed, n_steps, max_iter, history_size, lr, tol_grad, tol_change,
                                      rec_host},
                                     &K, &ldk);
}

int gpfit_estep_chain_full_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* const* K,
                                 const int64_t* ldk, int64_t N, const double* const* r, const double* const* kv0,
                                 double* const* m, double* const* f, double* const* V, const int64_t* ldv,
                                 double* const* lam_m, double* const* lam_var, const double* logA0, int lambda0_mode,
                                 const double* lambda0_fixed, int n_steps, int max_iter, int history_size, double lr,
                                 double tol_grad, double tol_change, double* rec_host) {
  return estep_chain_full_group_impl({"gpfit_estep_chain_full_batch", ctxs, n_units, stream, N, r, kv0, m, f, V, ldv, lam_m, lam_var,
                                      logA0, lambda0_mode, lambda0_fixed, n_steps, max_iter, history_size, lr, tol_grad, tol_change,
                                      rec_host},
                                     K, ldk);
}

int gpfit_fparam_lbfgs_host(const double* lam_m, const double* lam_var, const double* r, int64_t N, double logA0,
                            int lambda0_mode, double lambda0_fixed, int max_iter, int history_size, double lr,
                            double tol_grad, double tol_change, double* f_out, double* out_host) {
  if (!lam_m || !lam_var || !r || !out_host || N <= 0) {
    set_error("gpfit_fparam_lbfgs_host: bad argument");
    return -3;
  }
  Lbfgs1dConfig cfg;
  GP_TRY(fparam_lbfgs_config("gpfit_fparam_lbfgs_host", max_iter, history_size, lr, tol_grad, tol_change, &cfg));
  FparamClosure<FparamHostPass> obj{};
  obj.ev = FparamHostPass{lam_m, lam_var, N, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = 0; i < N; ++i) {
    obj.ev.sr += r[i];
    obj.ev.srm += r[i] * lam_m[i];
  }
  obj.fixed = lambda0_mode ? 1 : 0;
  obj.lambda0_fixed = lambda0_fixed;
  std::vector<double> hist(4 * (size_t)history_size + 1);
  double* h = hist.data();
  const Lbfgs1dResult res = lbfgs1d_step<Lbfgs1dHostSlots>(
      obj, logA0, cfg, Lbfgs1dStorage{h, h + history_size, h + 2 * history_size, h + 3 * history_size});
  double lambda0 = std::nan("");
  if (res.status == 0) {
    obj.ev.pass(res.x);
    lambda0 = obj.ev.lambda0_closed();
    if (f_out)
      for (int64_t i = 0; i < N; ++i)
        f_out[i] = std::exp(obj.ev.A * lam_m[i] + 0.5 * obj.ev.A * obj.ev.A * lam_var[i] + lambda0);
  }
  const double o[9] = {res.x, lambda0, res.first_loss, res.last_loss, (double)res.n_evals, (double)res.n_iter,
                       (double)res.status, res.status ? obj.fail_x : 0.0, res.status ? obj.fail_lambda0 : 0.0};
  for (int i = 0; i < 9; ++i) out_host[i] = o[i];
  return 0;
}

}  // extern "C"
