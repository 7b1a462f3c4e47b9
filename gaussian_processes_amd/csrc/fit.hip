// Host-side orchestration of the GP fit path on one MI355X: workspace context, the recursive
// blocked Cholesky built from MFMA GEMMs, and the fused unit of work (one evaluation of the
// reference's M-step closure, utils.py:2017-2112) in the original-basis Cholesky formulation
// (DESIGN.md section 3).  The fused entry points -- gpfit_fit_eval, gpfit_fit_eval_batch,
// gpfit_grad_pullback, gpfit_fit_eval_projected and gpfit_fit_eval_sparse with their group forms
// gpfit_fit_eval_projected_batch / gpfit_fit_eval_sparse_batch (one body each) -- are each a short sequence of
// the shared stages defined once below ("shared stages of the fused closures": admission, kernel build,
// the vectors behind the factor, the mixed-precision hand-over, the pull-back to the metric, the
// n_kept x n_kept algebra of the truncated-rank closures, the host assembly of the 16 outputs); what
// differs between the entry points is which stages they call and what they launch in between.
#include "units.h"
#include "gemm_core.h"
#include "gpfit_mi355x.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

namespace gpfit {

// ------------------------------------------------------------------ per-launch profiling
static thread_local gpfit_ctx* g_prof = nullptr;

// tile-walk choices of the large launches (tuning knob GPFIT_WALKS = trsm,tmp,merge,T,Q,Rbase,H)
static int walk(Walk which) {
  static int w[W_COUNT] = {3, 2, 1, 9, 9, 2, 2};  // bit 3 = XCD-aware macro-tile schedule where the launch is large enough
                                                // (gemm_sched.hip), else the walk in the low bits
  static bool init = false;
  if (!init) {
    init = true;
    if (const char* e = getenv("GPFIT_WALKS")) {
      int v[W_COUNT];
      if (sscanf(e, "%d,%d,%d,%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6]) == 7)
        for (int i = 0; i < W_COUNT; ++i) w[i] = v[i];
    }
  }
  return w[which];
}

static hipEvent_t prof_event(gpfit_ctx* c) {
  hipEvent_t e;
  if (!c->ev_pool.empty()) {
    e = c->ev_pool.back();
    c->ev_pool.pop_back();
    return e;
  }
  (void)hipEventCreate(&e);
  return e;
}

void prof_begin(gpfit_ctx* c) {
  if (c->profile == 1) {
    g_prof = c;
    c->prof.clear();
  }
}

void prof_end(gpfit_ctx* c) {
  if (g_prof != c) return;
  g_prof = nullptr;
  (void)hipDeviceSynchronize();
  double ms[4] = {0, 0, 0, 0}, fl[4] = {0, 0, 0, 0}, cnt[4] = {0, 0, 0, 0};
  double big_ms = 0, big_fl = 0;
  for (auto& r : c->prof) {
    float t = 0.f;
    (void)hipEventElapsedTime(&t, r.a, r.b);
    if (r.kind == 0 && r.flops > big_fl) { big_fl = r.flops; big_ms = t; }
    ms[r.kind] += t;
    fl[r.kind] += r.flops;
    cnt[r.kind] += 1;
    c->ev_pool.push_back(r.a);
    c->ev_pool.push_back(r.b);
  }
  c->prof.clear();
  c->prof_out[0] = ms[0]; c->prof_out[1] = fl[0]; c->prof_out[2] = cnt[0];
  c->prof_out[3] = ms[1]; c->prof_out[4] = cnt[1];
  c->prof_out[5] = ms[2]; c->prof_out[6] = fl[2]; c->prof_out[7] = cnt[2];
  c->prof_out[8] = ms[3]; c->prof_out[9] = fl[3]; c->prof_out[10] = cnt[3];
  c->prof_out[11] = big_ms; c->prof_out[12] = big_fl;
}

ProfScope::ProfScope(hipStream_t s_, double flops_, int kind_) : s(s_), flops(flops_), kind(kind_) {
  if (g_prof) {
    a = prof_event(g_prof);
    (void)hipEventRecord(a, s);
  }
}
ProfScope::~ProfScope() {
  if (g_prof && a) {
    hipEvent_t b = prof_event(g_prof);
    (void)hipEventRecord(b, s);
    g_prof->prof.push_back({a, b, flops, kind});
  }
}

// flops actually executed by one GEMM launch on T-tiles (the route's tile; whole tiles over each tile's k range)
template <typename R>
double gemm_flops(const GemmArgsT<R>& g, int T) {
  const int tm = (g.M + T - 1) / T, tn = (g.N + T - 1) / T, r = TILE / T;
  double steps = 0;
  for (int ti = 0; ti < tm; ++ti)
    for (int tj = 0; tj < tn; ++tj) {
      if (g.out_lower && tj / r > ti / r) continue;
      const KRange kr = gemm_tile_k_range(g.a_tri, g.b_tri, g.K, ti * T, tj * T, T, g.b_split);
      if (kr.end > kr.beg) steps += (kr.end - kr.beg);
    }
  return 2.0 * T * T * steps * (g.nptr > 0 ? g.nptr : (g.batch > 0 ? g.batch : 1));
}

// ------------------------------------------------------------------ GEMM convenience
// tuning aid: GPFIT_GEMM_LOG=k lists every GEMM launch of the k-th evaluation of the process on stderr (shape,
// structure flags, problems in the batch, block tile, executed flops), in launch order -- to be paired with a
// kernel trace of the same run (scripts/trace_gemm_rates.py)
static int g_eval_count = 0;
static int gemm_log_eval() {
  static const int v = getenv("GPFIT_GEMM_LOG") ? atoi(getenv("GPFIT_GEMM_LOG")) : -1;
  return v;
}
static bool gemm_logging() { return gemm_log_eval() >= 0 && g_eval_count == gemm_log_eval(); }
// the fields of a log line behind its head: scalars, leading dimensions, walk, split-k, k slabs
template <typename R>
static void gemm_log_tail(const char* tag, const GemmArgsT<R>& g, const char* end) {
  fprintf(stderr, "%s alpha %g beta %g lda %lld ldb %lld ldc %lld walk %d split %d slabs %d%s", tag, g.alpha, g.beta, (long long)g.lda,
          (long long)g.ldb, (long long)g.ldc, g.reverse, g.split_k, g.k_slabs, end);
}

// launch g on its route r = gemm_route(g).  Every product of fit.hip, api_solve.hip and api_kernel.hip is logged here; a
// profile entry is made only while a fit_eval-family evaluation has a profile open (g_prof): never for the latter two
template <typename R>
int run_gemm(hipStream_t s, const GemmArgsT<R>& g, const GemmRoute& r) {
  if (gemm_logging()) {
    fprintf(stderr, "[gpfit gemm] M %d N %d K %d atri %d btri %d lower %d nb %d tile %d ak %d bk %d epi %d flops %.6e", g.M, g.N, g.K,
            g.a_tri, g.b_tri, g.out_lower, g.nptr > 0 ? g.nptr : 1, r.tile, g.a_kmajor, g.b_kmajor, g.epi, gemm_flops(g, r.tile));
    gemm_log_tail("", g, "");
    if (g.b_split > 0) fprintf(stderr, " bsplit %d", g.b_split);
    fprintf(stderr, "\n");
  }
  // profile kind 0: the 128-tile kernel family (the dominant kernel), 3: the small-tile instances
  ProfScope ps(s, g_prof ? gemm_flops(g, r.tile) : 0.0, (g_prof && r.tile != TILE) ? 3 : 0);
  return launch_gemm(g, r, s);
}
template int run_gemm<double>(hipStream_t, const GemmArgsT<double>&, const GemmRoute&);
template int run_gemm<float>(hipStream_t, const GemmArgsT<float>&, const GemmRoute&);

// slabs so that a product with few output tiles still launches about one and a half rounds of 128-tile workgroups,
// each with a k range of at least 256
static int splitk_for(int M, int N, int K) {
  const long tiles = (long)((M + TILE - 1) / TILE) * ((N + TILE - 1) / TILE);
  if (tiles >= 384) return 1;
  long sp = (768 + tiles - 1) / tiles;
  sp = std::min<long>(sp, std::max(1, K / 256));
  return (int)std::max<long>(1, sp);
}
// C = alpha op(A) op(B) for every problem of a list, the k range of each cut into splitk_for slabs: the shapes of the
// truncated-rank closures whose output has few tiles but a long k (K_b = K~ B: 8192 x 512 x 8192; B^T X: 512 x 512 x
// 8192) fill the chip with 128-tiles only this way.  A problem's slabs go to its own scratch partial[i] (splits x M x ld
// elements; as many slabs as it holds) and are added in slab order by one pass (deterministic; C must be the contiguous
// block [M][ld]).  A product that takes slabs for one problem is issued problem by problem -- a 128-tile launch fills the
// chip alone; where no problem takes slabs the list goes through product, which decides about batching as ever.
template <typename R>
static int gemm_splitk_list(Lane lane, Dims d, double alpha, const Operand<R>& a, const Operand<R>& b, const Mat<R>& C,
                            R* const* partial, const int64_t* partial_elems) {
  static const bool off = getenv("GPFIT_NO_SPLITK") != nullptr;   // tuning knob
  const int64_t slab = (int64_t)d.M * C.ld;
  int splits[GEMM_MAXB];
  bool any = false;
  for (int i = 0; i < C.cnt; ++i) {
    splits[i] = (off || !partial[i]) ? 1 : (int)std::min<int64_t>(splitk_for(d.M, d.N, d.K), partial_elems[i] / std::max<int64_t>(1, slab));
    any = any || splits[i] > 1;
  }
  if (!any) return product(lane, d, alpha, a, b, into(C));
  for (int i = 0; i < C.cnt; ++i) {
    Operand<R> ai = a, bi = b;
    ai.m.cnt = bi.m.cnt = 1;
    ai.m.p[0] = a.m.p[i]; bi.m.p[0] = b.m.p[i];
    if (splits[i] <= 1) {
      GP_TRY(product(lane, d, alpha, ai, bi, into(mat(C.p[i], C.ld))));
      continue;
    }
    GemmArgsT<R> g = product_args(lane, d, alpha, ai, bi, into(mat(partial[i], C.ld)));
    g.split_k = splits[i];
    g.sC = slab;
    g.tile = TILE;
    GP_TRY(run_gemm(lane.s, g));
    GP_TRY(launch_reduce_slices(partial[i], slab, splits[i], C.p[i], slab, lane.s));
  }
  return 0;
}

// tuning knob (bit mask, default all): fused GEMM epilogues -- 1 Q's symmetrisation, 2 T's norm (without it T21 and
// T22 stay two launches), 4 the H / Z21 update of the two-sided product, 8 LV21 added in S's launch
static int fused_epilogues() {
  static const int v = getenv("GPFIT_FUSED_EPI") ? atoi(getenv("GPFIT_FUSED_EPI")) : 15;
  return v;
}

// One product for every problem of a list (product.h).  e: fused epilogue wanted; e->carried says whether the launches
// carried it -- all of them or none (the caller runs the separate passes otherwise); e->sumsq_entries: what the route
// of one such launch says.
template <typename R>
int product(Lane lane, Dims d, double alpha, const Operand<R>& a, const Operand<R>& b, const Output<R>& c, int walk, Epilogue<R>* e) {
  const int cnt = c.m.cnt, epi = e ? e->which : 0;
  if (e) { e->carried = false; e->sumsq_entries = 0; }
  if (cnt <= 0) return 0;
  if (cnt > GEMM_MAXB) {
    set_error("product: more problems than a pointer batch holds");
    return -3;
  }
  GemmArgsT<R> g = product_args(lane, d, alpha, a, b, c, walk);
  static const bool no_batch = getenv("GPFIT_NO_BATCH") != nullptr;   // tuning knob: every product on its own
  if (cnt == 1 || gemm_pick_tile(g) == TILE || no_batch) {
    auto problem = [&](int i, bool fused) {
      g.A = a.m.p[i]; g.B = b.m.p[i]; g.C = c.m.p[i]; g.B2 = b.split > 0 ? b.p2[i] : nullptr;
      g.epi = fused ? epi : 0; g.aux = fused ? e->aux[i] : nullptr; g.sumsq = fused ? e->sumsq[i] : nullptr;
    };
    GemmRoute routes[GEMM_MAXB];
    bool fused = epi != 0;
    for (int i = 0; i < cnt && fused; ++i) {
      problem(i, true);
      routes[i] = gemm_route(g);
      fused = routes[i].epi != 0;
    }
    for (int i = 0; i < cnt; ++i) {
      problem(i, fused);
      GP_TRY(fused ? run_gemm(lane.s, g, routes[i]) : run_gemm(lane.s, g));
    }
    if (e) e->carried = fused;
    if (fused) e->sumsq_entries = routes[0].sumsq_entries;
    return 0;
  }
  g = batch_args(lane, d, alpha, a, b, c, walk, e);
  GemmRoute r = gemm_route(g);
  if (epi && r.epi == 0) {   // the batch cannot carry it: without
    g.epi = 0;
    r = gemm_route(g);
  }
  if (e) { e->carried = g.epi != 0; e->sumsq_entries = r.sumsq_entries; }
  return run_gemm(lane.s, g, r);
}
template int product<double>(Lane, Dims, double, const Operand<double>&, const Operand<double>&, const Output<double>&, int,
                             Epilogue<double>*);
template int product<float>(Lane, Dims, double, const Operand<float>&, const Operand<float>&, const Output<float>&, int,
                            Epilogue<float>*);

// ------------------------------------------------------------------ recursive Cholesky (+ inverse), in lock step
// Recursive blocked Cholesky built entirely from the MFMA GEMM and the 128 x 128 leaf, for nb matrices of the same
// size at once (CholBatchT, context.h): one matrix (gpfit_potrf, the E-steps, a unit whose V factor is reused), the
// K~ and V chains of one unit, or the chains of several independent units.  Every level whose launches cannot fill
// the chip -- the leaves and the products of the small blocks, i.e. the latency-bound bottom of the recursion -- is
// ONE launch for all chains (a pointer batch, GemmArgsT::nptr / LeafBatchT): the number of kernel boundaries on the
// critical path does not grow with the number of chains and every small launch has nb times the workgroups.
// Products that are 128-tile launches for a single chain are issued chain by chain through the ordinary launcher,
// with its stream-K / XCD-aware schedules (product above).  A chain therefore gets the same bits whatever else is in
// the batch: its launches are the same products in the same order, stream-K only ever applies to 128-tile launches of
// a single problem, and every data-parallel instance sums k in ascending order per element whatever block tile the
// launcher picks.
//
// A chain in neither `need` nor `halves` (V's chain of the closures: the factor only) reads the inverse of a node's first
// half in one place, the row solve L21 = A21 L11^-T.  From first halves of VSOLVE_MIN on that solve is a block
// substitution with the inverses of the first half's own two halves (three products, the same flops), and the first
// half's recursion skips the chain's merge [L11^-1]21: 2 h1^2 h2 flops and two launches off the critical path.
// Smaller first halves keep the single product: there the merge rides in launches the other chains need anyway and
// two more dependent launches cost more than it (one size down, first halves of 2048: profiles/r27_top_node.txt).
// Tuning knob GPFIT_VSOLVE_MIN (0: never).
constexpr int VSOLVE_MIN = 4096;
static int vsolve_min() {
  static const int v = getenv("GPFIT_VSOLVE_MIN") ? atoi(getenv("GPFIT_VSOLVE_MIN")) : VSOLVE_MIN;
  return v;
}

template <typename R>
int potrf_lockstep(const CholBatchT<R>& B, int r0, int n, uint32_t need, Lane lane, uint32_t halves) {
  const int64_t ld = B.ld;
  const hipStream_t s = lane.s;
  const uint32_t all = (B.nb >= 32) ? 0xffffffffu : ((1u << B.nb) - 1u);
  auto off = [&](int r, int c) { return (int64_t)r * ld + c; };
  // block (r, c) of matrix X of every chain in `mask`
  auto blk = [&](uint32_t mask, R* const* X, int r, int c) {
    Mat<R> m{};
    m.ld = ld;
    for (int b = 0; b < B.nb; ++b)
      if (mask & (1u << b)) m.p[m.cnt++] = X[b] + off(r, c);
    return m;
  };
  if (n == TILE) {
    ProfScope ps(s, 0.0, 1);
    LeafBatchT<R> bt{};
    bt.n = B.nb;
    for (int b = 0; b < B.nb; ++b) {
      bt.A[b] = B.A[b] + off(r0, r0); bt.L[b] = B.L[b] + off(r0, r0); bt.Li[b] = B.Li[b] + off(r0, r0);
      bt.info[b] = B.info[b];
    }
    bt.lda = bt.ldl = bt.ldi = ld;
    bt.info_base = r0;
    return launch_chol_leaf_batch(bt, s);
  }
  const int k = n / TILE;
  const int n1 = ((k + 1) / 2) * TILE, n2 = n - n1;
  const int r1 = r0 + n1;
  // the chains whose first half is read by this node's row solve alone (neither `need` nor `halves`): from
  // VSOLVE_MIN on they substitute with the first half's own blocks and that half skips their merge
  const uint32_t sub = (vsolve_min() > 0 && n1 >= vsolve_min() && n1 >= 2 * TILE) ? (all & ~(need | halves)) : 0u;
  const uint32_t full = all & ~sub;
  GP_TRY(potrf_lockstep<R>(B, r0, n1, full, lane, sub));
  // L21 = A21 L11^-T       (trsm as a GEMM against the explicit inverse)
  if (full)
    GP_TRY(product(lane, {n2, n1, n1}, 1.0, plain(blk(full, B.A, r1, r0)), trans(tril(blk(full, B.Li, r0, r0))),
                   into(blk(full, B.L, r1, r0)), walk(W_TRSM)));
  if (sub) {
    // the same solve against L11 = [P 0; R S] with P^-1 and S^-1 only (the first half's split h1 + h2):
    //   Z1 = Y1 P^-T ;  Y2 -= Z1 R^T (in A, which the factorisation destroys anyway) ;  Z2 = Y2 S^-T
    const int h1 = ((n1 / TILE + 1) / 2) * TILE, h2 = n1 - h1;
    // A half-width solve that is a 128-tile launch of less than two rounds of the chip (4096 x 2048: 512 tiles for 512
    // workgroup slots) takes as long as its longest tile, the whole k range -- the time of the dense product, which has
    // twice its flops (profiles/r27_top_node.txt).  On 64-tiles it is four rounds, heavy tiles first.  The one shape
    // this rests on is the headline's; the bits do not depend on the tile.
    auto half_solve = [&](Dims d, const Operand<R>& y, const Operand<R>& li, const Output<R>& z) -> int {
      const bool one_round = gemm_pick_tile(product_args(lane, d, 1.0, y, li, z, walk(W_TRSM))) == TILE &&
                             (long)(d.M / TILE) * (d.N / TILE) < 2 * SK_SLOTS;
      return product(lane, d, 1.0, y, li, one_round ? on_tiles(z, 64) : z, walk(W_TRSM));
    };
    GP_TRY(half_solve({n2, h1, h1}, plain(blk(sub, B.A, r1, r0)), trans(tril(blk(sub, B.Li, r0, r0))), into(blk(sub, B.L, r1, r0))));
    GP_TRY(product(lane, {n2, h2, h1}, -1.0, plain(blk(sub, B.L, r1, r0)), trans(blk(sub, B.L, r0 + h1, r0)),
                   into(blk(sub, B.A, r1, r0 + h1), 1.0)));
    GP_TRY(half_solve({n2, h2, h2}, plain(blk(sub, B.A, r1, r0 + h1)), trans(tril(blk(sub, B.Li, r0 + h1, r0 + h1))),
                      into(blk(sub, B.L, r1, r0 + h1))));
  }
  // the two products that only need L21 and L11^-1:  A22 -= L21 L21^T (syrk, lower tiles only) for every chain, and
  // tmp = L21 Li11, the first product of the inverse merge, for the chains in `need`
  const Operand<R> L21 = plain(blk(all, B.L, r1, r0)), L21t = trans(blk(all, B.L, r1, r0));
  const Output<R> A22 = into_lower(blk(all, B.A, r1, r1), 1.0);
  const Operand<R> L21n = plain(blk(need, B.L, r1, r0)), Li11 = plain(tril(blk(need, B.Li, r0, r0)));
  const Output<R> tmp = into(blk(need, B.Tmp, r1, r0));
  const Dims syrk{n2, n2, n1}, merge1{n2, n1, n1};
  // Look-ahead: tmp needs nothing from the second half, so it runs on the context's side stream while that half is
  // being factored (its leaves are latency-bound and leave the chip to it).  Possible because the leaf shares a CU
  // with GEMM workgroups.
  hipEvent_t joined = nullptr;
  if (need && B.ctx && B.side_min > 0 && n >= B.side_min && B.ctx->side) {
    gpfit_ctx* c = B.ctx;
    auto next_event = [&]() {
      if (c->side_ev_next == (int)c->side_ev.size()) {
        hipEvent_t e = nullptr;
        (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
        c->side_ev.push_back(e);
      }
      return c->side_ev[c->side_ev_next++];
    };
    hipEvent_t fork = next_event();
    joined = next_event();
    GP_HIP(hipEventRecord(fork, s));
    GP_HIP(hipStreamWaitEvent(c->side, fork, 0));
    GP_TRY(product(side_lane(c), merge1, 1.0, L21n, Li11, tmp, walk(W_TMP)));
    GP_HIP(hipEventRecord(joined, c->side));
  }
  // On the latency-bound levels tmp rides in the syrk's launch: one launch boundary less per node.
  bool merged = false;
  if (need && !joined) {
    static const bool no_batch = getenv("GPFIT_NO_BATCH") != nullptr;
    const GemmArgsT<R> g2 = batch_args(lane, syrk, -1.0, L21, L21t, A22);
    const GemmArgsT<R> g3 = batch_args(lane, merge1, 1.0, L21n, Li11, tmp, walk(W_TMP));
    const GemmRoute pr = no_batch ? GemmRoute{} : gemm_pair_shape(g2, g3);
    if (!no_batch && pr.rc == 0) {
      if (gemm_logging()) {
        fprintf(stderr, "[gpfit gemm] pair: M %d N %d K %d lower 1 nb %d + M %d N %d K %d btri 1 nb %d tile %d flops %.6e", g2.M, g2.N,
                g2.K, g2.nptr, g3.M, g3.N, g3.K, g3.nptr, pr.tile, gemm_flops(g2, pr.tile) + gemm_flops(g3, pr.tile));
        gemm_log_tail(" a:", g2, "");
        gemm_log_tail(" b:", g3, "\n");
      }
      ProfScope ps(s, g_prof ? gemm_flops(g2, pr.tile) + gemm_flops(g3, pr.tile) : 0.0, 3);
      GP_TRY(launch_gemm_pair(g2, g3, pr, s));
      merged = true;
    }
  }
  if (!merged) GP_TRY(product(lane, syrk, -1.0, L21, L21t, A22));
  GP_TRY(potrf_lockstep<R>(B, r1, n2, need | halves, lane));
  if (need) {
    // Li21 = -Li22 (L21 Li11)
    if (joined) GP_HIP(hipStreamWaitEvent(s, joined, 0));
    else if (!merged) GP_TRY(product(lane, merge1, 1.0, L21n, Li11, tmp, walk(W_TMP)));
    GP_TRY(product(lane, {n2, n1, n2}, -1.0, plain(tril(blk(need, B.Li, r1, r1))), plain(blk(need, B.Tmp, r1, r0)),
                   into(blk(need, B.Li, r1, r0)), walk(W_MERGE)));
  }
  return 0;
}

template int potrf_lockstep<double>(const CholBatchT<double>&, int, int, uint32_t, Lane, uint32_t);
template int potrf_lockstep<float>(const CholBatchT<float>&, int, int, uint32_t, Lane, uint32_t);

// ------------------------------------------------------------------ two-sided triangular product
// Wout (lower) = 1/2 Li^T Q Li on the n x n diagonal block at r0, Q symmetric (stored in full),
// Li lower triangular.  The direct route R = Q Li, W = Li^T R costs 4/3 n^3; splitting once,
//   Li = [A 0; B C],  H = Q21 A + 1/2 Q22 B,
//   W11 = A^T Q11 A + B^T H + H^T B,   W21 = C^T (H + 1/2 Q22 B),   W22 = C^T Q22 C,
// costs 3/4 n^3 plus the two half-size products (LAPACK's sygst idea), i.e. 13/12 n^3 with
// one level; blocks of n >= min_split (4096) are split again: 1.02 n^3 at n = 8192.  Z and H are n x n scratch matrices with the same leading dimension.
// L: the matrix whose 21 block holds the factor's own L21 (two_sided_top only).
template <typename R>
struct TwoSidedBufs { R* Q; const R* Li; R *W, *Z, *H; const R* L; int64_t ld; int min_split; };   // (Q: overwritten by two_sided_top)
// block (r0[i] + dr, r0[i] + dc) of matrix X of every problem (r0 == nullptr: the blocks sit at the origin)
template <typename R, typename P>
static Mat<P> ts_blk(int cnt, const TwoSidedBufs<R>* b, const int* r0, P* TwoSidedBufs<R>::*X, int dr, int dc) {
  return mats(cnt, b[0].ld, [&](int i) { const int o = r0 ? r0[i] : 0; return b[i].*X + (int64_t)(o + dr) * b[i].ld + o + dc; });
}
// H = alpha op(A) op(B) + Z ;  Z = H + Z  for every problem of the list (H and Z M x N): one launch with the dual-update
// epilogue; where the launch cannot carry it, a copy, the product with beta = 1 and an axpby pass -- the same arithmetic.
template <typename R>
static int dual_update_list(Lane lane, Dims d, double alpha, const Operand<R>& a, const Operand<R>& b, const Mat<R>& H,
                            const Mat<R>& Z, int wk) {
  const int cnt = H.cnt;
  const int64_t ld = H.ld;
  Epilogue<R> e{4};
  for (int i = 0; i < cnt; ++i) e.aux[i] = Z.p[i];
  // would the fused launch be possible?  (asked first: the unfused route must copy Z into H beforehand)
  bool fused = false;
  if (fused_epilogues() & 4) {
    GemmArgsT<R> g = product_args(lane, d, alpha, a, b, into(H), wk);
    g.epi = 4; g.aux = Z.p[0];
    static const bool no_batch = getenv("GPFIT_NO_BATCH") != nullptr;
    if (cnt > 1 && gemm_pick_tile(g) != TILE && !no_batch) { g.nptr = cnt; g.batch = cnt; }
    fused = gemm_route(g).epi != 0;
  }
  if (fused) {
    GP_TRY(product(lane, d, alpha, a, b, into(H), wk, &e));
    if (!e.carried) {
      set_error("two_sided: the dual-update epilogue was announced but not carried");
      return -100;
    }
    return 0;
  }
  for (int i = 0; i < cnt; ++i)
    GP_HIP(hipMemcpy2DAsync(H.p[i], (size_t)ld * sizeof(R), Z.p[i], (size_t)ld * sizeof(R), (size_t)d.N * sizeof(R), (size_t)d.M,
                            hipMemcpyDeviceToDevice, lane.s));
  GP_TRY(product(lane, d, alpha, a, b, into(H, 1.0), wk));
  for (int i = 0; i < cnt; ++i) GP_TRY(launch_axpby_block<R>(Z.p[i], ld, H.p[i], ld, d.M, d.N, 1.0, 1.0, lane.s));
  return 0;
}

// cnt diagonal blocks of size n (block i of problem b[i] at offset r0[i]) in lock step: the two half-size
// two-sided products a split leaves behind (W11's A^T Q11 A and W22) depend on nothing else of their level, so
// they -- and the sub-blocks of several units -- share their launches (product): two 2048-sized problems
// are one 128-tile launch of 512 workgroups instead of two 64-tile launches.  Same products, same order per
// block: bit-identical to the block-by-block recursion.
template <typename R>
static int two_sided_list(Lane lane, int cnt, const TwoSidedBufs<R>* b, const int* r0, int n) {
  if (cnt <= 0) return 0;
  using TS = TwoSidedBufs<R>;
  auto blk = [&](auto X, int dr, int dc) { return ts_blk(cnt, b, r0, X, dr, dc); };
  const int k = n / TILE;
  if (n < b[0].min_split || k < 2) {
    static const int wbase_walk = getenv("GPFIT_WBASE_WALK") ? atoi(getenv("GPFIT_WBASE_WALK")) : 0;
    // Z = Q Li (Q is symmetric: read k-major) ;  W = 1/2 Li^T Z (lower tiles)
    GP_TRY(product(lane, {n, n, n}, 1.0, trans(blk(&TS::Q, 0, 0)), plain(tril(blk(&TS::Li, 0, 0))), into(blk(&TS::Z, 0, 0)),
                   walk(W_RBASE)));
    return product(lane, {n, n, n}, 0.5, trans(tril(blk(&TS::Li, 0, 0))), plain(blk(&TS::Z, 0, 0)),
                   into_lower(blk(&TS::W, 0, 0)), wbase_walk);
  }
  const int n1 = ((k + 1) / 2) * TILE, n2 = n - n1;
  auto diagonal_blocks = [&]() -> int {
    // 1/2 A^T Q11 A (into W11) and W22 = 1/2 C^T Q22 C, all of them in lock step when the halves are equal
    TwoSidedBufs<R> bb[GEMM_MAXB];
    int rr[GEMM_MAXB];
    if (n1 == n2 && 2 * cnt <= GEMM_MAXB) {
      for (int i = 0; i < cnt; ++i) {
        bb[2 * i] = b[i]; rr[2 * i] = r0[i];
        bb[2 * i + 1] = b[i]; rr[2 * i + 1] = r0[i] + n1;
      }
      return two_sided_list<R>(lane, 2 * cnt, bb, rr, n1);
    }
    for (int i = 0; i < cnt; ++i) rr[i] = r0[i] + n1;
    GP_TRY(two_sided_list<R>(lane, cnt, b, r0, n1));
    return two_sided_list<R>(lane, cnt, b, rr, n2);
  };
  // Z21 = 1/2 Q22 B
  GP_TRY(product(lane, {n2, n1, n2}, 0.5, trans(blk(&TS::Q, n1, n1)), plain(blk(&TS::Li, n1, 0)), into(blk(&TS::Z, n1, 0))));
  // H = Q21 A + Z21 ;  Z21 = H + 1/2 Q22 B
  GP_TRY(dual_update_list(lane, {n2, n1, n1}, 1.0, plain(blk(&TS::Q, n1, 0)), plain(tril(blk(&TS::Li, 0, 0))), blk(&TS::H, n1, 0),
                          blk(&TS::Z, n1, 0), walk(W_H)));
  // W21 = 1/2 C^T Z21
  static const int w21_walk = getenv("GPFIT_W21_WALK") ? atoi(getenv("GPFIT_W21_WALK")) : 0;
  GP_TRY(product(lane, {n2, n1, n2}, 0.5, trans(tril(blk(&TS::Li, n1, n1))), plain(blk(&TS::Z, n1, 0)),
                 into(blk(&TS::W, n1, 0)), w21_walk));
  GP_TRY(diagonal_blocks());
  // W11 += 1/2 (B^T H + H^T B)   (lower tiles)
  GP_TRY(product(lane, {n1, n1, n2}, 0.5, trans(blk(&TS::Li, n1, 0)), plain(blk(&TS::H, n1, 0)), into_lower(blk(&TS::W, 0, 0), 1.0)));
  return product(lane, {n1, n1, n2}, 0.5, trans(blk(&TS::H, n1, 0)), plain(blk(&TS::Li, n1, 0)), into_lower(blk(&TS::W, 0, 0), 1.0));
}

// Smallest padded size whose closure works on the top node's blocks (A = L11^-1, C = L22^-1 and L21) instead of the
// full inverse factor: the recursion then skips the merge [L^-1]21 = -C (L21 A), 2 n1^2 n2 flops on the critical
// path, and T, W and the mean's solves substitute with L21 at the same flop count -- but in 3 (T), 11 instead of 2-7
// (W) and 8 instead of 3 (vectors) launches of half the size.  Measured, full form | block form, ms per fit (fp64,
// single unit, MI355X): N = 512 0.47 | 0.55, 1024 0.78 | 0.86, 2048 1.88 | 2.01, 2560 2.75 | 2.76, 3072 3.61 | 3.65,
// 4096 6.05-6.09 | 5.99-6.02, 8192 29.64-29.66 | 27.76-27.90; groups of 16 x N = 4096 261 | 250 ms, mixed-precision
// groups of 16 x N = 8192 (per 512 points) 7.75 | 6.82 s.  Below 2048 the launches cost far more than the merge
// (latency-bound sizes: 12 us per extra dependent launch); a single unit's break-even lies between 3072 and 4096.
// The threshold sits at 2048, the size from which tests/test_gpu_top_inverse.py checks that the merge's flops are
// gone: between 2048 and 3072 the block form gives 0.13 ... 0.03 ms (7 ... 1 %) back to the full form (W's eleven
// launches of half-size blocks on 64-tiles against two; DESIGN.md section 7, open item 0).
// The all-fp32 instance: N = 4096 3.74-3.76 | 3.77-3.79, 8192 16.28-16.32 | 15.43-15.46.  Its merge runs at twice the
// rate against the same launch costs, which puts its break-even 2^(1/3) above fp64's: 5120.
// elem_bytes: of the chains being factored (a mixed-precision unit factors in fp64).
constexpr int TOP_BLOCKS_MIN = 2048, TOP_BLOCKS_MIN_F32 = 5120;
static bool top_in_blocks(int np, size_t elem_bytes) { return np >= (elem_bytes == 4 ? TOP_BLOCKS_MIN_F32 : TOP_BLOCKS_MIN); }

// The top level of W = 1/2 L^-T Q L^-1 for cnt units, written with the factor's own off-diagonal block L21 (b[i].L: the
// matrix whose 21 block holds it) and the inverses A = L11^-1, C = L22^-1 of the diagonal halves: the closure never
// forms [L^-1]21 = -C L21 A (potrf_lockstep's `halves`).  With R = C^T Q21:
//   W22 = 1/2 C^T Q22 C                    two_sided_list on the block, then completed in both triangles
//   Z21 = 1/2 R ;  H = Z21 - W22 L21 ;  J = Z21 + H = R - W22 L21          (dual update)
//   W21 = H A                                                  ( = 1/2 (R - 2 W22 L21) A )
//   M   = Q11 - L21^T J - J^T L21         in place over Q11, lower tiles, then completed
//   W11 = 1/2 A^T M A                      two_sided_list on the block
// The same flops as the split with the explicit [L^-1]21 (two_sided_list); W11 needs W22, so the two diagonal blocks
// of this level do not share launches.  No step reads a block an earlier step of the stage has overwritten.
template <typename R>
static int two_sided_top(Lane lane, int cnt, const TwoSidedBufs<R>* b, int n) {
  if (cnt <= 0) return 0;
  using TS = TwoSidedBufs<R>;
  const hipStream_t s = lane.s;
  const int64_t ld = b[0].ld;
  auto blk = [&](auto X, int r, int c) { return ts_blk(cnt, b, (const int*)nullptr, X, r, c); };
  int rr[GEMM_MAXB];
  const int k = n / TILE;
  const int n1 = ((k + 1) / 2) * TILE, n2 = n - n1;   // (top_in_blocks: both halves exist)
  for (int i = 0; i < cnt; ++i) rr[i] = n1;
  GP_TRY(two_sided_list<R>(lane, cnt, b, rr, n2));
  for (int i = 0; i < cnt; ++i) GP_TRY(launch_symmetrize(b[i].W + (int64_t)n1 * ld + n1, ld, n2, s));
  // Z21 = 1/2 C^T Q21
  static const int w21_walk = getenv("GPFIT_W21_WALK") ? atoi(getenv("GPFIT_W21_WALK")) : 0;
  GP_TRY(product(lane, {n2, n1, n2}, 0.5, trans(tril(blk(&TS::Li, n1, n1))), plain(blk(&TS::Q, n1, 0)),
                 into(blk(&TS::Z, n1, 0)), w21_walk));
  // H = -W22 L21 + Z21 ;  Z21 = J = H + Z21
  GP_TRY(dual_update_list(lane, {n2, n1, n2}, -1.0, plain(blk(&TS::W, n1, n1)), plain(blk(&TS::L, n1, 0)), blk(&TS::H, n1, 0),
                          blk(&TS::Z, n1, 0), 0));
  // W21 = H A
  GP_TRY(product(lane, {n2, n1, n1}, 1.0, plain(blk(&TS::H, n1, 0)), plain(tril(blk(&TS::Li, 0, 0))), into(blk(&TS::W, n1, 0)),
                 walk(W_H)));
  // M = Q11 - L21^T J - J^T L21   (lower tiles, then both triangles: the block products below read M in full)
  GP_TRY(product(lane, {n1, n1, n2}, -1.0, trans(blk(&TS::L, n1, 0)), plain(blk(&TS::Z, n1, 0)), into_lower(blk(&TS::Q, 0, 0), 1.0)));
  GP_TRY(product(lane, {n1, n1, n2}, -1.0, trans(blk(&TS::Z, n1, 0)), plain(blk(&TS::L, n1, 0)), into_lower(blk(&TS::Q, 0, 0), 1.0)));
  for (int i = 0; i < cnt; ++i) GP_TRY(launch_symmetrize(b[i].Q, ld, n1, s));
  for (int i = 0; i < cnt; ++i) rr[i] = 0;
  return two_sided_list<R>(lane, cnt, b, rr, n1);
}

// ------------------------------------------------------------------ host pieces of localker
static double lin_pm1_host(int i, int n) {
  if (n <= 1) return -1.0;
  const double step = 2.0 / (double)(n - 1);
  return (i < n / 2) ? std::fma(step, (double)i, -1.0) : std::fma(-step, (double)(n - 1 - i), 1.0);
}

static int compute_mask(const double* theta, int n_rows, int n_cols, uint8_t* mask, int* pix) {
  const double eb = std::exp(theta[3]);
  int d = 0;
  for (int p = 0; p < n_rows * n_cols; ++p) {
    const double x = lin_pm1_host(p % n_cols, n_cols), y = lin_pm1_host(p / n_cols, n_rows);
    const double dx = x - theta[1], dy = y - theta[2];
    const double alpha = std::exp(-eb * (dx * dx + dy * dy));  // utils.py:880-881
    const bool keep = alpha >= 0.001;                          // utils.py:883
    if (mask) mask[p] = keep ? 1 : 0;
    if (keep) {
      if (pix) pix[d] = p;
      ++d;
    }
  }
  return d;
}

static Theta make_theta(const double* t) {
  Theta th;
  th.sigma0 = t[0]; th.eps0x = t[1]; th.eps0y = t[2]; th.logbeta = t[3]; th.logrho = t[4]; th.amp = t[5];
  th.eb = std::exp(t[3]);
  th.er = std::exp(t[4]);
  return th;
}

static int check_limits(const double* theta, const double* lower, const double* upper) {
  static const char* names[6] = {"sigma_0", "eps_0x", "eps_0y", "-2log2beta", "-log2rho2", "Amp"};
  for (int i = 0; i < 6; ++i) {
    if (!(lower[i] <= theta[i] && theta[i] <= upper[i])) {  // utils.py:866, 2023 (NaN fails too)
      char buf[256];
      snprintf(buf, sizeof buf, "%s = %.4f is not within the limits of %g and %g", names[i], theta[i], lower[i],
               upper[i]);
      set_error(buf);
      return -2;
    }
  }
  return 0;
}

// Side stream of the factorisation's look-ahead products: off the critical path, lowest priority.  Created when a
// synchronous evaluation first wants it -- contexts that only ever serve grouped / asynchronous evaluations never
// do, and every stream a process creates is one more claimant of the few hardware queues.
int ensure_side_stream(gpfit_ctx* c) {
  if (c->side) return 0;
  int least = 0, greatest = 0;
  GP_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
  GP_HIP(hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, least));
  return 0;
}

template <typename T>
static int dev_alloc(gpfit_ctx* c, T** p, size_t count) {
  void* q = nullptr;
  GP_HIP(hipMalloc(&q, count * sizeof(T)));
  c->allocs.push_back(q);
  *p = (T*)q;
  return 0;
}

// ------------------------------------------------------------------ shared stages of the fused closures
// The fused entry points are short sequences of the stages below (file-local functions on the context, the
// stream and plain pointers: nothing here allocates or dispatches indirectly -- the host enqueue time of a unit is
// part of its measured time at N <= 2048).  Which entry point uses which:
//   stage                                   fit_eval  _batch  grad_pullback  _projected  _sparse (each single and _batch)
//   admit                                      x        x          x             x          x
//   build_kernel                               x        x          x             x      (its parts)
//   solve_mean, post_join_args,
//   demote_for_mixed, set_pending              x        x
//   adjoint_pass, xty                          x        x          x             x          x
//   pullback_to_metric                                             x             x          x
//   projected_factor, _kl_products, _adjoints, closure_prepare / _collect        x          x
//   assemble_out                          (fit_eval_finish)                      x          x
// A stage is a fixed launch sequence; where two entry points order their launches differently the cut is between
// stages, never inside one.
template <typename R>
static R* ws_as(double* b) { return reinterpret_cast<R*>(b); }  // the workspace is allocated for fp64

// utils.py:2020-2028: out-of-box theta -> infinite loss and infinite gradients
static void fill_out_of_box(double* out) {
  const double inf = std::numeric_limits<double>::infinity();
  out[OUT_LOSS] = inf;
  out[OUT_LOGLIK] = out[OUT_KL] = std::numeric_limits<double>::quiet_NaN();
  for (int i = 0; i < 6; ++i) out[OUT_GRAD + i] = inf;
}

// Admission of one evaluation to context c: the limits (lower / upper may be absent), the capacity for np padded
// stimuli, the masked pixel list (c->pix_host) with its count d and padded count dp, and the hyperparameters.
// Returns 0, -2 (theta outside the limits: `out` holds the infinite loss / gradients) or -3; the error strings carry
// the entry point's `name` and speak of `whose` capacity ("the context" / "a context's").
struct Admitted { int d, dp; Theta th; };
static int admit(gpfit_ctx* c, const char* name, const char* whose, const double* theta, const double* lower,
                 const double* upper, int n_rows, int n_cols, int np, double* out, Admitted* a) {
  if (lower && upper && check_limits(theta, lower, upper) != 0) {
    fill_out_of_box(out);
    return -2;
  }
  if (np > c->np_cap || n_rows * n_cols > c->dfull_cap) {
    set_error(std::string(name) + ": problem larger than " + whose + " capacity");
    return -3;
  }
  a->d = compute_mask(theta, n_rows, n_cols, nullptr, c->pix_host);
  a->dp = (int)round_up(a->d, 32);
  if (a->d <= 0 || a->dp > c->dp_cap) {
    set_error(std::string(name) + ": masked pixel count is zero or exceeds " + whose + " capacity");
    return -3;
  }
  a->th = make_theta(theta);
  return 0;
}

// ---- kernel build: the metric C, then per set of stimuli the masked copies and vectors, then the Gram matrix
template <typename R>
static int build_metric(gpfit_ctx* c, hipStream_t s, const Theta& th, int d, int dp, int n_rows, int n_cols) {
  return launch_localker<R>(th, c->pix, d, dp, n_rows, n_cols, ws_as<R>(c->Cmat), dp, nullptr, s);
}
// one set of n stimuli: masked and k-major in Xt [dp][np], row-major in Xm [np][dp], C Xt, and Kvec / q
template <typename R>
static int kernel_side(gpfit_ctx* c, Lane lane, const R* X, int64_t ldx, int n, int np, int d, int dp, double s0sq,
                       R* Xt, R* XCt, R* Xm, R* Kvec, R* q) {
  const int64_t ld = np;
  const hipStream_t s = lane.s;
  GP_TRY(launch_gather(X, ldx, n, c->pix, d, dp, np, Xt, ld, Xm, dp, s));
  // C X^T (C is symmetric: read k-major)
  GP_TRY(product(lane, {dp, np, dp}, 1.0, trans(mat(ws_as<R>(c->Cmat), dp)), plain(mat(Xt, ld)), into(mat(XCt, ld))));
  return launch_qvec(Xt, XCt, ld, dp, n, np, s0sq, Kvec, q, s);
}
// K~ = acosker(x, x) with its cosine matrix: lower tiles, identity on the padding.  mirror: the tiles also store
// their transposes (for callers that multiply with K~ from the left).  The launch sits in a profiling scope for every
// caller: only gpfit_fit_eval, _projected and _sparse ever open a profile (prof_begin), and those three had it.
template <typename R>
static int gram_square(hipStream_t s, const R* XCt, const R* Xt, const R* q, R* Kout, R* Cos, int n, int np, int dp,
                       double s0sq, int mirror) {
  GramArgsT<R> g{};
  g.XCt = XCt; g.Xt = Xt; g.q1 = q; g.q2 = q; g.Kout = Kout; g.Cos = Cos;
  g.ld1 = np; g.ld2 = np; g.ldk = np; g.np1 = np; g.np2 = np; g.nv1 = n; g.nv2 = n; g.Kd = dp;
  g.s0sq = s0sq; g.lower = 1; g.pad_identity = 1;
  g.mirror = mirror;
  ProfScope ps(s, (double)np * (np + TILE) * dp, 2);
  return launch_gram(g, s);
}
// the kernel objects of one set of stimuli in the context's own buffers: Cmat, Xt, XCt, Xm, Kvec, q, Kbuf, Cos
template <typename R>
static int build_kernel(gpfit_ctx* c, Lane lane, const Theta& th, int d, int dp, int n_rows, int n_cols, const R* X,
                        int64_t ldx, int n, int np, int mirror) {
  const double s0sq = th.sigma0 * th.sigma0;
  const hipStream_t s = lane.s;
  GP_TRY(build_metric<R>(c, s, th, d, dp, n_rows, n_cols));
  GP_TRY(kernel_side<R>(c, lane, X, ldx, n, np, d, dp, s0sq, ws_as<R>(c->Xt), ws_as<R>(c->XCt), ws_as<R>(c->Xm),
                        ws_as<R>(c->Kvec), ws_as<R>(c->q)));
  return gram_square<R>(s, ws_as<R>(c->XCt), ws_as<R>(c->Xt), ws_as<R>(c->q), ws_as<R>(c->Kbuf), ws_as<R>(c->Cos), n, np,
                        dp, s0sq, mirror);
}

// ---- the vectors behind K~'s factor: y = L^-1 m, m^T K~^-1 m = y . y, b = K~^-1 m = L^-T y.  Sizes in block form
// (top_in_blocks) substitute with A = L11^-1, C = L22^-1 (the diagonal halves of Libuf) and L21 (in Lbuf); Libuf's 21
// block is stale there and never read:
//   y1 = A m1 ,  y2 = C (m2 - L21 y1) ,  b2 = C^T y2 ,  b1 = A^T (y1 - L21^T b2)
// (the same bytes as the whole lower triangle of L^-1; bv doubles as the scratch of the two right-hand sides)
template <typename R>
static int solve_mean(gpfit_ctx* c, int np, bool blocks, hipStream_t s) {
  const int64_t ld = np;
  R *m = ws_as<R>(c->mpad), *y = ws_as<R>(c->yv), *b = ws_as<R>(c->bv);
  if (!blocks) {
    GP_TRY(launch_trmv_lower(ws_as<R>(c->Libuf), ld, np, m, y, s));
    GP_TRY(launch_dot(y, y, np, c->scal + S_MKM, s));
    return launch_trmv_lower_t(ws_as<R>(c->Libuf), ld, np, y, b, c->trmv_part, s);
  }
  const int kt = np / TILE, n1 = ((kt + 1) / 2) * TILE, n2 = np - n1;   // potrf_lockstep's split of the top node
  const R *A = ws_as<R>(c->Libuf), *C = A + (int64_t)n1 * ld + n1, *L21 = ws_as<R>(c->Lbuf) + (int64_t)n1 * ld;
  GP_TRY(launch_trmv_lower(A, ld, n1, m, y, s));
  GP_TRY(launch_gemv_sub(L21, ld, n2, n1, y, m + n1, b + n1, s));
  GP_TRY(launch_trmv_lower(C, ld, n2, b + n1, y + n1, s));
  GP_TRY(launch_dot(y, y, np, c->scal + S_MKM, s));
  GP_TRY(launch_trmv_lower_t(C, ld, n2, y + n1, b + n1, c->trmv_part, s));
  GP_TRY(launch_gemv_t_sub(L21, ld, n2, n1, b + n1, y, b, c->trmv_part, s));
  return launch_trmv_lower_t(A, ld, n1, b, b, c->trmv_part, s);
}

// ---- pull-back of an n x n adjoint to the d x d metric
// Adjoint pass over the lower tiles of W: Lambda = tril(A_w, -1) + 1/2 diag(A_w) into the lower 64-tiles of A (zeros
// above the diagonal inside the diagonal tiles; the tiles above it are neither written here nor read by
// lambda_t_x_list), t into tvec, the sums into scal[S_ADJ..].
template <typename R>
static int adjoint_pass(gpfit_ctx* c, hipStream_t s, const R* W, const R* Cos, const R* bv, const R* q, const R* wl, int n,
                        int np, R* A, R* tvec) {
  GP_TRY(launch_adjoint(W, Cos, (int64_t)np, bv, q, n, np, A, c->upart, c->vpart, c->sumA_part, s));
  const int t64 = np / 64;
  return launch_adjoint_reduce(c->upart, c->vpart, c->sumA_part, t64, t64 * (t64 + 1) / 2, q, wl, n, np, tvec, c->rpad,
                               c->scal + S_ADJ, s);
}
// out [dp][dp] = Xa^T Yb over np rows: split-k into the slabs of Mpart, added in slab order; sym: out = G + G^T with
// G that sum (the same pass: no extra launch).  prof: the product is
// counted by a profile (gpfit_set_profile(c, 1)) -- so far only for the full-rank unit (post_join_list); the
// truncated-rank closures' profiles never counted theirs, and their launch counts stay as they were.
template <typename R>
static int xty(gpfit_ctx* c, hipStream_t s, const R* Xa, const R* Yb, int np, int dp, R* out, bool prof, bool sym = false) {
  // (no workspace, as ever: gemm_route keeps a split_k > 1 launch off the stream-K schedule, so none is ever read)
  GemmArgsT<R> g = product_args(Lane{s, nullptr}, {dp, dp, np}, 1.0, trans(mat(Xa, dp)), plain(mat(Yb, dp)),
                                into(mat(ws_as<R>(c->Mpart), dp)));
  g.split_k = c->split_k_M; g.sC = (int64_t)dp * dp;
  const GemmRoute r = gemm_route(g);
  if (prof) {
    ProfScope ps(s, g_prof ? gemm_flops(g, r.tile) : 0.0, (g_prof && r.tile != TILE) ? 3 : 0);
    GP_TRY(launch_gemm(g, r, s));
  } else {
    GP_TRY(launch_gemm(g, r, s));
  }
  if (sym) return launch_reduce_slices_sym(ws_as<R>(c->Mpart), (int64_t)dp * dp, c->split_k_M, out, dp, s);
  return launch_reduce_slices(ws_as<R>(c->Mpart), (int64_t)dp * dp, c->split_k_M, out, (int64_t)dp * dp, s);
}
// The pull-back in its Lambda form.  A_w = Lambda + Lambda^T, so
//   M = Xm^T (A_w + diag t) Xm = G + G^T ,   G = Xm^T (Lambda^T Xm + 1/2 diag(t) Xm):
// half the flops of A_w Xm, and the adjoint pass stores every tile once.
// Slabs of the product Lambda^T Xm (GemmArgsT::k_slabs): a function of the shape alone -- a unit gets the same cut,
// hence the same bits, alone and inside a group.  Four slabs from 32 tiles per side, two from 8, and never more
// than fit the np x np scratch matrix (np x dp each).
static int pullback_slabs(int np, int dp) {
  const int nt = np / SLAB_TILE;
  return std::max(1, std::min(nt >= 32 ? 4 : (nt >= 8 ? 2 : 1), np / dp));
}
// Y[i] = Lambda[i]^T Xm[i] for cnt units of one shape (np a multiple of 64): Lambda is read k-major as A_w was, so
// op(A) is upper triangular (a_tri 2) and the launch walks each row panel's own k range only, cut into
// (panel, slab) items of roughly equal length.  One launch -- a pointer batch for cnt > 1 -- then per unit the sum
// of each row's live slabs, in slab order (no atomics).  a = Lambda^T, b = Xm; scratch: np x np elements each, idle (Z behind W).
template <typename R>
static int lambda_t_x_list(Lane lane, const Operand<R>& a, const Operand<R>& b, const Mat<R>& Y, const Mat<R>& scratch, int np, int dp) {
  const int cnt = Y.cnt;
  if (cnt <= 0 || cnt > GEMM_MAXB) return cnt == 0 ? 0 : -3;
  const int slabs = pullback_slabs(np, dp);
  const SlabPlan sp = slab_plan(np, slabs);
  const bool direct = sp.live == 1;   // one slab: straight into Y
  const Output<R> c = into(direct ? Y : scratch);
  GemmArgsT<R> g = cnt > 1 ? batch_args(lane, {np, dp, np}, 1.0, a, b, c) : product_args(lane, {np, dp, np}, 1.0, a, b, c);
  g.k_slabs = slabs;
  g.sC = (int64_t)np * dp;
  GP_TRY(run_gemm(lane.s, g));
  if (direct) return 0;
  for (int i = 0; i < cnt; ++i)
    GP_TRY(launch_reduce_slabs(scratch.p[i], (int64_t)np * dp, sp.live, sp.ks * SLAB_TILE, Y.p[i], np, dp, lane.s));
  return 0;
}
// Mmat = Xm^T (A_w + diag t) Xm for the adjoint W of acosker(x, x) on n stimuli (q, Cos, Xm theirs; A, scratch:
// np x np work matrices), with the b b^T and dKvec terms the caller left in bv / wl.  The contraction with dC_p
// (launch_metric_contract) is the caller's: the sparse closure adds two more d x d matrices first.
static int pullback_to_metric(gpfit_ctx* c, Lane lane, const double* W, const double* Cos, const double* q, int n,
                              int np, int dp, double* A, const double* Xm, double* scratch) {
  const hipStream_t s = lane.s;
  GP_TRY(adjoint_pass<double>(c, s, W, Cos, c->bv, q, c->wl, n, np, A, c->tvec));
  GP_TRY(lambda_t_x_list(lane, trans(tril(mat(A, np))), plain(mat(Xm, dp)), mat(c->Ybuf, dp), mat(scratch, dp), np, dp));
  GP_TRY(launch_rowscale_add(c->Ybuf, dp, Xm, dp, c->tvec, np, dp, s, 0.5));
  return xty<double>(c, s, Xm, c->Ybuf, np, dp, c->Mmat, false, true);
}

// ---- the n_kept x n_kept algebra of the truncated-rank closures (nb = n_kept padded; leading dimension nb), in the
// scratch matrices S1..S4 = Vbuf, LVbuf, LiVbuf, TmpV of each unit's context -- for a list of cnt units (the
// closures of a group; one unit: the single closures), every small kernel one launch for the list (kernels.h).
// What is kept per unit beside the contexts (V_b, ldvb, nk, vc, m_b, d) is indexed like the caller's tables (units.h).
// the work matrices of a unit's V_b chain (the caller's: which of the context's are idle differs between the closures).
// The recursion writes a chain's L, L^-1 and Tmp on and below the diagonal only and reads them as triangles (k ranges
// that end with the diagonal tile, which the leaf writes whole) or as blocks below the diagonal: what the tiles above
// hold is never summed, and the truncated closure hands over Wbuf, Zbuf and Tmp as the last evaluation left them.  The
// sparse closure clears its three first (launch_zero3_group): its chain began in slots of the split-K scratch, which
// were cleared, and the clear moved with the chain into Kbuf, Lbuf and Abuf.  Each keeps its own launch sequence.
struct ProjChain { double *Va, *Vl, *Vli, *Vt; };
// K~_b (packed into S1) = L L^T with L^-1 (utils.py:2067) and V_b (packed into Va) = L_V L_V^T (log|V_b|, :1326): the
// 2 cnt chains in lock step, the inverse for the K~_b chains only; then K~_b^-1 = L^-T L^-1 in S1 and V_b in S2, both
// stored in full with the identity on the padding.  nk[i]: the unit's own n_kept; nb is shared (the recursion's split).
static int projected_factor(Lane lane, const Units& U, const double* const* V_b, const int64_t* ldvb, const int* nk, int nb,
                            const ProjChain* vc) {
  if (U.cnt == 0) return 0;
  const int cnt = U.cnt;
  const int64_t lb = nb;
  const hipStream_t s = lane.s;
  CholBatchT<double> cb;
  uint32_t kchains = 0;
  for (int i = 0; i < cnt; ++i) {
    const ProjChain& v = vc[U.at[i]];
    kchains |= 1u << add_v_chain(cb, U.ctx[i], INFO_K);   // K~_b's chain, in S1..S4
    add_chain(cb, v.Va, v.Vl, v.Vli, v.Vt, U.ctx[i]->info + INFO_V);
  }
  cb.ld = lb; cb.ctx = nullptr; cb.side_min = 0;
  GP_TRY(potrf_lockstep<double>(cb, 0, nb, kchains, lane));
  const PerUnit<int> nks = U.from(nk);
  GP_TRY(launch_logdet_pair_group(cnt, U.table<const double*>([&](int u) { return vc[u].Vl; }), U.scal(S_LOGDET_V),
                                  U.cof(&gpfit_ctx::LVbuf), U.scal(S_LOGDET_K), lb, nks, s));
  GP_TRY(product(lane, {nb, nb, nb}, 1.0, trans(tril(U.mats(&gpfit_ctx::LiVbuf, lb))), plain(tril(U.mats(&gpfit_ctx::LiVbuf, lb))),
                 into_lower(U.mats(&gpfit_ctx::Vbuf, lb))));   // L^-T L^-1
  GP_TRY(launch_symmetrize_group(cnt, U.of(&gpfit_ctx::Vbuf), lb, nb, s));
  GP_TRY(launch_pack_lower_group(cnt, U.from(V_b), U.from(ldvb), nks, U.of(&gpfit_ctx::LVbuf), lb, nb, s));
  return launch_symmetrize_group(cnt, U.of(&gpfit_ctx::LVbuf), lb, nb, s);
}
// K~_b^-1 V_b in S3, its trace tr(K~_b^-1 V_b) in scal[S_TRACE], P1 = K~_b^-1 V_b K~_b^-1 in S4.  (The two closures form
// a V_b on different sides of this stage, and b = K~_b^-1 m_b behind it.)
static int projected_kl_products(Lane lane, const Units& U, const int* nk, int nb) {
  if (U.cnt == 0) return 0;
  const int64_t lb = nb;
  const Mat<double> Ki = U.mats(&gpfit_ctx::Vbuf, lb), S2 = U.mats(&gpfit_ctx::LVbuf, lb), S3 = U.mats(&gpfit_ctx::LiVbuf, lb),
                    S4 = U.mats(&gpfit_ctx::TmpV, lb);
  GP_TRY(product(lane, {nb, nb, nb}, 1.0, plain(Ki), plain(S2), into(S3)));
  GP_TRY(launch_proj_trace_group(U.cnt, U.of(&gpfit_ctx::LiVbuf), lb, U.from(nk), U.scal(S_TRACE), lane.s));
  return product(lane, {nb, nb, nb}, 1.0, plain(S3), plain(Ki), into(S4));
}
// What both closures run behind a V_b, for the units of pg (a = pg.am is B, or K_b K~_b^-1): b = K~_b^-1 m_b and m_b . b;
// moments, rate, likelihood pieces (utils.py:1090, 1101, 1138, 1243) and the per-point adjoints g_m, g_v; G_a, G_a K~_b^-1,
// P2 = a^T G_a K~_b^-1 in the k slabs of each unit's `part`, G_K~b, and G_Kb in place on G_a K~_b^-1 (utils._closure_adjoints).
static int projected_adjoints(Lane lane, const ProjGroupT& pg, double* const* part, const int64_t* part_elems) {
  auto all = [&](const PerUnit<double*>& X) { return mats(pg.n_units, pg.ld, [&](int i) { return X[i]; }); };
  GP_TRY(launch_symv_lower_group(pg.n_units, pg.Ki, pg.ld, pg.nb, pg.mb, pg.bvec, lane.s));
  GP_TRY(launch_dot_group(pg.n_units, pg.mb, pg.bvec, pg.nb, pg.mkm, lane.s));
  GP_TRY(launch_proj_moments_group(pg, lane.s));
  GP_TRY(launch_proj_ga_group(pg, lane.s));
  GP_TRY(product(lane, {pg.np, pg.nb, pg.nb}, 1.0, plain(all(pg.Ga)), plain(all(pg.Ki)), into(all(pg.GaKi))));
  GP_TRY(gemm_splitk_list(lane, {pg.nb, pg.nb, pg.np}, 1.0, trans(all(pg.am)), plain(all(pg.GaKi)), all(pg.P2), part, part_elems));
  GP_TRY(launch_proj_gktb_group(pg, lane.s));   // G_K~b
  return launch_proj_gkb_group(pg, lane.s);     // G_Kb
}
// The housekeeping of the closures of cnt units, one launch each (kernels.h).  Begin: pixel lists, info words, m_b padded
// to nb, bv / wl cleared.  End: the 64 scalars and the info words of every unit straight into its pinned host buffers.
static int closure_prepare(const Units& U, const int* d, const int* nk, const double* const* m_b, int nb, hipStream_t s) {
  ClosurePrepT gp{};
  gp.n_units = U.cnt; gp.nb = nb;
  for (int i = 0; i < U.cnt; ++i) {
    gp.pix_host.v[i] = U.ctx[i]->pix_host; gp.cap.v[i] = U.ctx[i]->np_cap; gp.cap_max = std::max(gp.cap_max, U.ctx[i]->np_cap);
  }
  gp.pix = U.of(&gpfit_ctx::pix); gp.info = U.of(&gpfit_ctx::info); gp.d = U.from(d); gp.nk = U.from(nk);
  gp.m_b = U.from(m_b); gp.mpad = U.of(&gpfit_ctx::mpad); gp.bv = U.of(&gpfit_ctx::bv); gp.wl = U.of(&gpfit_ctx::wl);
  return launch_closure_prepare(gp, s);
}
static int closure_collect(const Units& U, hipStream_t s) {
  GroupCollectT gc{};
  gc.n_units = U.cnt;
  for (int i = 0; i < U.cnt; ++i) {
    gpfit_ctx* c = U.ctx[i];
    gc.scal[i] = c->scal; gc.info[i] = c->info; gc.scal_host[i] = c->scal_host; gc.info_host[i] = c->info_host;
  }
  return launch_group_collect(gc, s);
}

// ---- host assembly of an evaluation's 16 output scalars from the device scalars (c->scal_host, c->info_host)
// the part of the sigma_0 row every closure has, derived from utils.py:996-1004 / 1036
static double sigma0_row_metric(const double* sc, double sigma0) { return sigma0 * (2.0 * sc[S_ADJ_SUMA] + 2.0 * sc[S_ADJ]); }
// d(loss)/d(theta) = dKL - dL (utils.py:2097-2099): the metric rows come from the contraction, the sigma_0 row in
// closed form from the caller
static void grad_rows(const double* sc, double sigma0_row, double* g6) {
  g6[0] = sigma0_row;
  g6[1] = sc[S_D_EPSX];
  g6[2] = sc[S_D_EPSY];
  g6[3] = sc[S_D_BETA];
  g6[4] = sc[S_D_RHO];
  g6[5] = sc[S_D_AMP];
}
// pad: what the identity padding of both factors contributes to scal[S_TRACE] = ||L^-1 L_V||_F^2 (np - n for the full-rank
// unit, whose trace is that norm; 0 for the truncated-rank closures, whose trace kernel stops at n_kept).
// err_K / err_V: the messages of the two Cholesky failures, whose LAPACK info is the return value.
static int assemble_out(gpfit_ctx* c, double A, double lambda0, double sigma0_row, int pad, int d, int want_grad,
                        const char* err_K, const char* err_V, double* out_host) {
  const double* sc = c->scal_host;
  const double loglik = A * sc[S_RLAM] + lambda0 * sc[S_SUMR] - sc[S_SUMF];      // utils.py:1243
  const double trKinvV = sc[S_TRACE] - (double)pad;
  const double logdetV = sc[S_LOGDET_V];
  const double KL = -0.5 * logdetV + 0.5 * sc[S_LOGDET_K] + 0.5 * sc[S_MKM] + 0.5 * trKinvV;  // utils.py:1326
  out_host[OUT_LOSS] = -(loglik - KL);                                           // utils.py:2087-2089
  out_host[OUT_LOGLIK] = loglik;
  out_host[OUT_KL] = KL;
  if (want_grad) grad_rows(sc, sigma0_row, out_host + OUT_GRAD);
  else
    for (int i = 0; i < 6; ++i) out_host[OUT_GRAD + i] = 0.0;
  out_host[OUT_LOGDET_K] = sc[S_LOGDET_K];
  out_host[OUT_LOGDET_V] = logdetV;
  out_host[OUT_TRACE] = trKinvV;
  out_host[OUT_MKM] = sc[S_MKM];
  out_host[OUT_D] = (double)d;
  out_host[OUT_INFO_K] = (double)c->info_host[INFO_K];
  out_host[OUT_INFO_V] = (double)c->info_host[INFO_V];
  if (c->info_host[INFO_K] != 0) {
    set_error(err_K);
    return c->info_host[INFO_K];
  }
  if (c->info_host[INFO_V] != 0) {
    set_error(err_V);
    return c->info_host[INFO_V];
  }
  return 0;
}

// Everything after the join of the two factorisation chains: T = L^-1 L_V and its norm, and (with
// gradients) Q = I - T T^T, the two-sided product W, the adjoint pass and the pull-back to the metric.
// Sizes in block form (top_in_blocks): K~'s inverse factor arrives as the inverses of its two diagonal halves (Li:
// A = L11^-1, C = L22^-1; Li's 21 block is stale) and the factor's own 21 block (L: the matrix whose 21 block holds
// L21) -- [L^-1]21 is never formed.  Smaller sizes: Li is the full inverse factor, L is not read.
// Templated separately from the first half of the unit so that the mixed-precision mode (fp64
// factorisations, fp32 gradient products) can run it on single-precision copies.
template <typename R>
struct PostJoin {
  const R *Li, *L, *LV, *Cos, *bv, *q, *wl, *Xm, *Cmat;       // inputs
  R *T, *W, *Z, *H, *A, *Y, *tvec, *Mpart, *Mmat;             // work matrices (np^2), Y [np][dp], Mpart / Mmat
};
template <typename R>
static PostJoin<R> post_join_args(gpfit_ctx* c) {
  auto RP = ws_as<R>;
  return PostJoin<R>{RP(c->Libuf), RP(c->Lbuf), RP(c->LVbuf), RP(c->Cos), RP(c->bv), RP(c->q), RP(c->wl), RP(c->Xm), RP(c->Cmat),
                     RP(c->Tbuf), RP(c->Wbuf), RP(c->Zbuf), RP(c->Tmp), RP(c->Abuf), RP(c->Ybuf), RP(c->tvec),
                     RP(c->Mpart), RP(c->Mmat)};
}
// Mixed precision: fp64 factorisations, log-determinants and likelihood; fp32 for the N^3-heavy products T, Q, W and
// the pull-back (T's norm, the trace term of the KL, is therefore fp32-derived: 2e-9 on the loss at N = 8192).  This
// is the hand-over: single-precision copies of the factors and of the O(N^2) / O(N) operands of the adjoint pass.
// Li -> Kbuf (its input was destroyed by the factorisation), in block form with L21 in the image's 21 block (where
// the full inverse has [L^-1]21), L_V -> Vbuf (likewise; kept while the V factor is
// reused), cos(delta) -> TmpV, vectors and the d x d metric into spare buffers.
static int demote_for_mixed(gpfit_ctx* c, bool reuse_V, int np, int dp, bool blocks, hipStream_t s, PostJoin<float>* pf) {
  auto F = ws_as<float>;
  const int64_t nn = (int64_t)np * np;
  GP_TRY((launch_reduce_slices<double, float>(c->Libuf, nn, 1, F(c->Kbuf), nn, s)));
  if (blocks) {
    const int kt = np / TILE, n1 = ((kt + 1) / 2) * TILE;
    GP_TRY(launch_demote_block(c->Lbuf + (int64_t)n1 * np, np, F(c->Kbuf) + (int64_t)n1 * np, np, np - n1, n1, s));
  }
  if (!(reuse_V && c->lv32_valid)) GP_TRY((launch_reduce_slices<double, float>(c->LVbuf, nn, 1, F(c->Vbuf), nn, s)));
  c->lv32_valid = true;
  GP_TRY((launch_reduce_slices<double, float>(c->Cos, nn, 1, F(c->TmpV), nn, s)));
  GP_TRY((launch_reduce_slices<double, float>(c->bv, np, 1, F(c->q2), np, s)));
  GP_TRY((launch_reduce_slices<double, float>(c->q, np, 1, F(c->dq1), np, s)));
  GP_TRY((launch_reduce_slices<double, float>(c->wl, np, 1, F(c->dq2), np, s)));
  GP_TRY((launch_reduce_slices<double, float>(c->Xm, (int64_t)np * dp, 1, F(c->Xt2), (int64_t)np * dp, s)));
  GP_TRY((launch_reduce_slices<double, float>(c->Cmat, (int64_t)dp * dp, 1, F(c->dCpad), (int64_t)dp * dp, s)));
  *pf = PostJoin<float>{F(c->Kbuf), F(c->Kbuf), F(c->Vbuf), F(c->TmpV), F(c->q2), F(c->dq1), F(c->dq2), F(c->Xt2), F(c->dCpad),
                        F(c->Tbuf), F(c->Wbuf), F(c->Zbuf), F(c->Tmp), F(c->Abuf), F(c->Ybuf), F(c->tvec),
                        F(c->Mpart), F(c->Mmat)};
  return 0;
}

// T = L^-1 L_V of cnt units in block form (top_in_blocks), with ||T||_F^2 into scal[5]:
//   T11 = A LV11 ,  T22 = C LV22                 lower x lower -> lower (one list when the halves are equal)
//   S = LV21 - L21 T11 ,  T21 = C S              dense x lower, lower x dense; S in Z's 21 block (idle until W):
//                                                L_V stays intact (its factor may be reused)
//   from the size where the launch takes the XCD-aware table: T11 alone, then [T21 | T22] = C [S | LV22] as one launch
// The tiles leave their sums of squares behind (no separate pass over T) where a launch can carry the epilogue;
// whether it is asked to depends on the single unit's launch only, so a group sums the norm in the unit's order.
template <typename R>
static int t_in_blocks(Lane lane, int cnt, gpfit_ctx* const* cs, const PostJoin<R>* a, int np) {
  using PJ = PostJoin<R>;
  const int64_t ld = np;
  const hipStream_t s = lane.s;
  const int kt = np / TILE, n1 = ((kt + 1) / 2) * TILE, n2 = np - n1;   // potrf_lockstep's split of the top node
  const int64_t o21 = (int64_t)n1 * ld;
  int ent = 0;   // entries of frob_part written so far (the same for every unit)
  // blocks whose launch cannot carry the norm get a pass of their own -- unless no launch of the unit carries it
  // (all on small tiles): then ONE pass over T's lower tiles, which are exactly the tiles of the three blocks
  const auto Li0 = tril(mat(a[0].Li, ld)), LV0 = mat(a[0].LV, ld);   // the first unit's, for the probe
  const Mat<R> T0 = mat(a[0].T, ld);
  auto asks = [&](Dims d, const Operand<R>& LV, const Output<R>& out, int wk) {   // op(A) is a lower block of L^-1 in all three
    GemmArgsT<R> g1 = product_args(lane, d, 1.0, plain(Li0), LV, out, wk);
    g1.epi = 2; g1.sumsq = cs[0]->frob_part;
    return (fused_epilogues() & 2) ? gemm_route(g1).sumsq_entries : 0;
  };
  auto asks_diag = [&](int nblk) { return asks({nblk, nblk, nblk}, plain(tril(LV0)), into_lower(T0), walk(W_T)); };
  auto asks_21 = [&]() { return asks({n2, n1, n2}, plain(LV0), into(T0), walk(W_MERGE)); };
  auto blk = [&](auto X, int64_t o) { return mats(cnt, ld, [&](int i) { return a[i].*X + o; }); };
  // [T21 | T22] = C [S | LV22] as ONE launch of n2 x np x n2 where the single unit's launch qualifies for the XCD-aware
  // table and carries the tile norms: T21 and T22 share their left operand, and together they are a launch the
  // table balances (1552 tiles with a k range at N = 8192) where T22 alone went to stream-K and T21 alone to a plain
  // walk.  op(B) is dense left of column n1 (S, in Z's 21 block) and LV22's lower triangle from it on, read in place
  // (dense_then_lower); T's strict upper tiles of the 22 block have no k range and stay unwritten, as before.
  const Dims joint{n2, np, n2};
  int e_joint = 0;
  if (fused_epilogues() & 2) {
    GemmArgsT<R> g1 = product_args(lane, joint, 1.0, plain(tril(mat(a[0].Li + o21 + n1, ld))),
                                   dense_then_lower(mat(a[0].Z + o21, ld), mat(a[0].LV + o21, ld), n1), into(mat(a[0].T + o21, ld)), walk(W_T));
    g1.epi = 2; g1.sumsq = cs[0]->frob_part;
    const GemmRoute r1 = gemm_route(g1);
    if (r1.rc == 0 && r1.epi) e_joint = r1.sumsq_entries;
  }
  const bool any_fused = e_joint > 0 || asks_diag(n1) > 0 || asks_diag(n2) > 0 || asks_21() > 0;
  // the product into T's blocks `out` with the tile norms asked for (e entries per problem, from sums[q] on) or passed
  // over afterwards
  auto normed_product = [&](Dims d, const Operand<R>& A, const Operand<R>& B, const Output<R>& out, int wk, bool ask, Epilogue<R>& e,
                            const char* what) -> int {
    e.which = ask ? 2 : 0;
    GP_TRY(product(lane, d, 1.0, A, B, out, wk, &e));
    if (e.carried != ask) {
      set_error(std::string("post_join: the tile-norm epilogue of ") + what + " was announced but not carried");
      return -100;
    }
    if (!e.carried && any_fused)
      for (int q = 0; q < out.m.cnt; ++q) GP_TRY(launch_frob_tiles<R>(out.m.p[q], ld, d.M, d.N, out.lower ? 1 : 0, e.sumsq[q], s));
    return 0;
  };
  // one list of lower x lower blocks: cb blocks (at rb[], all of size nblk) per unit
  auto diag_blocks = [&](int cb, const int* rb, int nblk) -> int {
    const int tb = nblk / TILE;
    int e = asks_diag(nblk);
    const bool ask = e > 0;
    if (!ask) e = tb * (tb + 1) / 2;
    auto blk = [&](auto X) { return mats(cnt * cb, ld, [&](int q) { return a[q / cb].*X + (int64_t)rb[q % cb] * (ld + 1); }); };
    Epilogue<R> ep{};
    for (int q = 0; q < cnt * cb && q < GEMM_MAXB; ++q) ep.sumsq[q] = cs[q / cb]->frob_part + ent + (q % cb) * e;
    GP_TRY(normed_product({nblk, nblk, nblk}, plain(tril(blk(&PJ::Li))), plain(tril(blk(&PJ::LV))), into_lower(blk(&PJ::T)),
                          walk(W_T), ask, ep, "a diagonal block of T"));
    ent += cb * e;
    return 0;
  };
  const int r_both[2] = {0, n1};
  if (e_joint > 0) GP_TRY(diag_blocks(1, r_both, n1));
  else if (n2 == n1 && 2 * cnt <= GEMM_MAXB) GP_TRY(diag_blocks(2, r_both, n1));
  else {
    GP_TRY(diag_blocks(1, r_both, n1));
    GP_TRY(diag_blocks(1, r_both + 1, n2));
  }
  {
    // S = LV21 - L21 T11 (in Z's 21 block): LV21 comes in through the added-matrix epilogue where the launch carries it
    // (L_V stays intact), else from a copy with beta = 1 -- the same arithmetic
    const Dims dS{n2, n1, n1};
    const Operand<R> L21 = plain(blk(&PJ::L, o21)), T11 = plain(tril(blk(&PJ::T, 0)));
    const Mat<R> S = blk(&PJ::Z, o21);
    Epilogue<R> add{8};
    for (int i = 0; i < cnt; ++i) add.aux[i] = const_cast<R*>(a[i].LV) + o21;   // (read only: epilogue 8)
    bool fused_s = false;
    if (fused_epilogues() & 8) {
      GemmArgsT<R> g = product_args(lane, dS, -1.0, L21, T11, into(S), walk(W_TMP));
      g.epi = 8; g.aux = add.aux[0];
      fused_s = gemm_route(g).epi != 0;   // (128-tiles only, which are issued unit by unit: the single unit's route decides)
    }
    if (fused_s) {
      GP_TRY(product(lane, dS, -1.0, L21, T11, into(S), walk(W_TMP), &add));
      if (!add.carried) {
        set_error("post_join: the added-matrix epilogue of S was announced but not carried");
        return -100;
      }
    } else {
      if (gemm_logging()) fprintf(stderr, "[gpfit copy] rows %d cols %d problems %d (LV21 into Z21)\n", n2, n1, cnt);
      for (int i = 0; i < cnt; ++i)
        GP_HIP(hipMemcpy2DAsync(a[i].Z + o21, (size_t)ld * sizeof(R), a[i].LV + o21, (size_t)ld * sizeof(R), (size_t)n1 * sizeof(R),
                                (size_t)n2, hipMemcpyDeviceToDevice, s));
      GP_TRY(product(lane, dS, -1.0, L21, T11, into(S, 1.0), walk(W_TMP)));
    }
  }
  if (e_joint > 0) {
    // unit by unit (a 128-tile launch each).  The table's tiles leave their norms at ti * tiles_n + tj; the entries of
    // the tiles that are not in it are zeroed here
    Epilogue<R> ep{};
    for (int i = 0; i < cnt; ++i) {
      ep.sumsq[i] = cs[i]->frob_part + ent;
      GP_HIP(hipMemsetAsync(ep.sumsq[i], 0, (size_t)e_joint * sizeof(double), s));
    }
    GP_TRY(normed_product(joint, plain(tril(blk(&PJ::Li, o21 + n1))), dense_then_lower(blk(&PJ::Z, o21), blk(&PJ::LV, o21), n1),
                          into(blk(&PJ::T, o21)), walk(W_T), true, ep, "[T21 | T22]"));
    ent += e_joint;
  } else {
    // T21 = C S
    int e = asks_21();
    const bool ask = e > 0;
    if (!ask) e = (n2 / TILE) * (n1 / TILE);
    Epilogue<R> ep{};
    for (int i = 0; i < cnt; ++i) ep.sumsq[i] = cs[i]->frob_part + ent;
    GP_TRY(normed_product({n2, n1, n2}, plain(tril(blk(&PJ::Li, o21 + n1))), plain(blk(&PJ::Z, o21)), into(blk(&PJ::T, o21)),
                          walk(W_MERGE), ask, ep, "T21"));
    ent += e;
  }
  for (int i = 0; i < cnt; ++i) {
    if (any_fused) GP_TRY(launch_frob_finish(cs[i]->frob_part, ent, cs[i]->scal + S_TRACE, s));
    else GP_TRY(launch_frob_lower(a[i].T, ld, np, cs[i]->scal + S_TRACE, cs[i]->frob_part, s));
  }
  return 0;
}

// cnt units at once (the units of a group, gpfit_fit_eval_batch; cnt = 1: the single unit): every product goes
// through product / two_sided_list -- one pointer-batched launch where a single unit's product cannot fill the
// chip, unit by unit through the ordinary launcher (balanced schedules, fused epilogues) where it can -- and the
// element-wise passes run unit by unit, all on ONE stream: a stream that waits on an event is not free on this
// runtime (every queue with a pending barrier packet slows the dispatch of the others), so a group gets its
// concurrency from batched launches, not from streams.  lane: the caller's stream with the leader's workspace.
template <typename R, typename PhaseFn>
static int post_join_list(Lane lane, int cnt, gpfit_ctx* const* cs, const PostJoin<R>* a, const Theta* th, int n, int np, const int* d,
                          const int* dp, int n_rows, int n_cols, int want_grad, bool blocks, PhaseFn&& phase) {
  using PJ = PostJoin<R>;
  const int64_t ld = np;
  const hipStream_t s = lane.s;
  if (cnt <= 0 || cnt > GEMM_MAXB) return cnt == 0 ? 0 : -3;
  auto all = [&](auto X, int64_t ldx) { return mats(cnt, ldx, [&](int i) { return a[i].*X; }); };   // matrix X of every unit
  // T = L^-1 L_V (lower x lower -> lower);  tr(K~^-1 V) = ||T||_F^2
  if (!blocks) {
    // the tiles leave their sums of squares behind (no separate pass over T) where the launch can carry the epilogue
    Epilogue<R> e{(fused_epilogues() & 2) ? 2 : 0};
    for (int i = 0; i < cnt; ++i) e.sumsq[i] = cs[i]->frob_part;
    GP_TRY(product(lane, {np, np, np}, 1.0, plain(tril(all(&PJ::Li, ld))), plain(tril(all(&PJ::LV, ld))), into_lower(all(&PJ::T, ld)),
                   walk(W_T), &e));
    for (int i = 0; i < cnt; ++i) {
      if (e.carried) GP_TRY(launch_frob_finish(cs[i]->frob_part, e.sumsq_entries, cs[i]->scal + S_TRACE, s));
      else GP_TRY(launch_frob_lower(a[i].T, ld, np, cs[i]->scal + S_TRACE, cs[i]->frob_part, s));
    }
  } else {
    GP_TRY(t_in_blocks<R>(lane, cnt, cs, a, np));
  }
  phase(4, s);
  if (!want_grad) return 0;
  // W = 1/2 (K~^-1 - K~^-1 V K~^-1) = 1/2 Li^T (I - T T^T) Li        (T = L^-1 L_V)
  //   Q = I - T T^T   lower x upper, lower tiles only          N^3/3
  //   W = 1/2 Li^T Q Li  two-sided product (two_sided_top /    13/12 N^3 with one split
  //                      two_sided_list)
  //                      (direct: R = Q Li, W = 1/2 Li^T R     4/3 N^3)
  {
    // T T^T: every tile of a tile column has the same k range [0, col + 128).  XCD-aware macro-tile schedule for
    // a single large unit (2.97 ms at N = 8192 in the fit; the column-major heavy-first data-parallel walk 3.02,
    // stream-K 3.2)
    Epilogue<R> mirror{(fused_epilogues() & 1) ? 1 : 0};
    GP_TRY(product(lane, {np, np, np}, -1.0, plain(tril(all(&PJ::T, ld))), trans(tril(all(&PJ::T, ld))), into_lower(all(&PJ::W, ld)),
                   walk(W_Q), &mirror));
    for (int i = 0; i < cnt; ++i) {
      GP_TRY(launch_add_diag(a[i].W, ld, np, 1.0, s));
      if (!mirror.carried) GP_TRY(launch_symmetrize(a[i].W, ld, np, s));   // otherwise the tiles stored their transposes
    }
  }
  phase(5, s);
  {
    static const int ts_min = getenv("GPFIT_TS_MIN") ? atoi(getenv("GPFIT_TS_MIN")) : 4096;
    TwoSidedBufs<R> tb[GEMM_MAXB];
    for (int i = 0; i < cnt; ++i)   // Q in W, W over T
      tb[i] = TwoSidedBufs<R>{a[i].W, a[i].Li, a[i].T, a[i].Z, a[i].H, a[i].L, ld, ts_min > 0 ? ts_min : (1 << 30)};
    if (blocks) GP_TRY(two_sided_top<R>(lane, cnt, tb, np));
    else {
      int r0[GEMM_MAXB];
      for (int i = 0; i < cnt; ++i) r0[i] = 0;
      GP_TRY(two_sided_list<R>(lane, cnt, tb, r0, np));
    }
  }
  phase(6, s);
  for (int i = 0; i < cnt; ++i)
    GP_TRY(adjoint_pass<R>(cs[i], s, a[i].T, a[i].Cos, a[i].bv, a[i].q, a[i].wl, n, np, a[i].A, a[i].tvec));
  // pull the contraction with dK~ back to the d x d metric: M = X^T (Aw + diag t) X = G + G^T (pullback_to_metric;
  // units with the same masked pixel count share the launch, the others go one by one through the same route)
  {
    bool same_dp = true;
    for (int i = 1; i < cnt; ++i) same_dp = same_dp && dp[i] == dp[0];
    if (same_dp)
      GP_TRY(lambda_t_x_list(lane, trans(tril(all(&PJ::A, ld))), plain(all(&PJ::Xm, dp[0])), all(&PJ::Y, dp[0]), all(&PJ::Z, dp[0]), np,
                             dp[0]));
    else
      for (int i = 0; i < cnt; ++i)
        GP_TRY(lambda_t_x_list(lane, trans(tril(mat(a[i].A, ld))), plain(mat(a[i].Xm, dp[i])), mat(a[i].Y, dp[i]), mat(a[i].Z, dp[i]), np,
                               dp[i]));
  }
  for (int i = 0; i < cnt; ++i) {
    gpfit_ctx* c = cs[i];
    GP_TRY(launch_rowscale_add(a[i].Y, dp[i], a[i].Xm, dp[i], a[i].tvec, np, dp[i], s, 0.5));
    GP_TRY(xty<R>(c, s, a[i].Xm, a[i].Y, np, dp[i], a[i].Mmat, true, true));
    GP_TRY(launch_metric_contract(th[i], c->pix, d[i], n_rows, n_cols, a[i].Cmat, dp[i], a[i].Mmat, dp[i], c->scal + S_METRIC, c->upart,
                                  c->info + INFO_METRIC, s));
  }
  return 0;
}

// what gpfit_fit_eval_finish needs to collect the evaluation just enqueued on c.  use_done: it waits for the
// group's completion event (c->pend.done) instead of the stream.
static void set_pending(gpfit_ctx* c, hipStream_t s, double A, double lambda0, double sigma0, int n, int np, int d,
                        int want_grad, int elem_bytes, bool use_done) {
  c->pend.active = true; c->pend.stream = s; c->pend.A = A; c->pend.lambda0 = lambda0; c->pend.sigma0 = sigma0;
  c->pend.n = n; c->pend.np = np; c->pend.d = d; c->pend.want_grad = want_grad; c->pend.elem_bytes = elem_bytes;
  c->pend.use_done = use_done;
}

// The fused unit of work, templated on the scalar type of the device data: fp64 is the
// reference's precision (headline); fp32 serves the hyperparameter-grid configuration
// (BASELINE configs[4]) -- every matrix, factorisation and GEMM in fp32 on v_mfma_f32_16x16x4_f32,
// scalars and reductions accumulated in fp64.
int fit_eval_finish(gpfit_ctx* c, double* out_host);

template <typename R>
static int fit_eval_impl(gpfit_ctx* c, void* stream, const double* theta, const double* lower, const double* upper,
                         int n_rows, int n_cols, const R* X, int64_t ldx, int64_t N, const R* r, const R* m,
                         const R* V, int64_t ldv, double logA, double lambda0, int want_grad, double* out_host,
                         R* lam_m_out, R* lam_var_out, R* f_out) {
  auto RP = ws_as<R>;
  if (!c || !theta || !X || !r || !m || !V || !out_host || N <= 0) {
    set_error("gpfit_fit_eval: bad argument");
    return -3;
  }
  GP_CTX_ENTER(c, "gpfit_fit_eval");
  hipStream_t s = (hipStream_t)stream;
  const int n = (int)N, np = (int)round_up(N, TILE);
  Admitted ad;
  GP_TRY(admit(c, "gpfit_fit_eval", "the context", theta, lower, upper, n_rows, n_cols, np, out_host, &ad));
  const int d = ad.d, dp = ad.dp;
  const Theta th = ad.th;
  const double A = std::exp(logA);
  const int64_t ld = np;
  const bool blocks = top_in_blocks(np, sizeof(R));   // the closure works on the top node's blocks, no [L^-1]21
  c->cur_n = n; c->cur_np = np; c->cur_d = d; c->cur_dp = dp;

  ++g_eval_count;
  const auto t_host0 = std::chrono::steady_clock::now();
  auto phase = [&](int i, hipStream_t st) {
    if (c->profile != 2) return;
    if (!c->phase_ev[i]) (void)hipEventCreate(&c->phase_ev[i]);
    (void)hipEventRecord(c->phase_ev[i], st);
  };
  c->phase_valid = false;
  phase(0, s);
  const Lane lane = main_lane(c, s);
  prof_begin(c);
  struct ProfGuard { gpfit_ctx* c; ~ProfGuard() { prof_end(c); } } prof_guard{c};
  GP_HIP(hipMemsetAsync(c->info, 0, 4 * sizeof(int), s));
  GP_HIP(hipMemcpyAsync(c->pix, c->pix_host, (size_t)d * sizeof(int), hipMemcpyHostToDevice, s));
  GP_HIP(hipMemsetAsync(RP(c->mpad), 0, (size_t)np * sizeof(R), s));
  GP_HIP(hipMemcpyAsync(RP(c->mpad), m, (size_t)n * sizeof(R), hipMemcpyDeviceToDevice, s));

  // ---- V: only log|V| and L_V are needed (no full inverse).
  // Opt-in reuse (flag bit 1 of want_grad): the caller promises V is the matrix of the previous
  // call on this context (V is constant during an M-step, utils.py:2016-2114), so L_V and
  // log|V| are kept.  bench.py never sets it: the unit of work includes this factorisation.
  const bool reuse_V = (want_grad & 2) && c->lv_valid && c->lv_n == n && c->lv_bytes == (int)sizeof(R);
  const bool async_call = (want_grad & 4) != 0;
  const bool mixed_grad = (want_grad & 8) != 0 && sizeof(R) == 8 && (want_grad & 1);
  want_grad &= 1;
  // tuning knob: smallest block whose inverse-merge product goes to the side stream (0 = never)
  // (only for synchronous calls: with several units in flight on several contexts the chip is busy
  // anyway and more streams per context oversubscribe the hardware queues -- 64 cells x N = 4096,
  // four in flight: 161 -> 118 cells/s with side streams)
  static const int side_min_env = getenv("GPFIT_SIDE_MIN") ? atoi(getenv("GPFIT_SIDE_MIN")) : 1024;
  const int side_min = async_call ? 0 : side_min_env;
  if (!async_call) GP_TRY(ensure_side_stream(c));
  c->side_ev_next = 0;
  // V is packed on the aux stream, beside the kernel build; both matrices then go through ONE recursion
  // (potrf_lockstep) whose latency-bound levels are shared launches.
  if (!reuse_V) {
    c->lv_valid = false; c->lv32_valid = false;
    GP_HIP(hipEventRecord(c->ev_fork, s));
    GP_HIP(hipStreamWaitEvent(c->aux, c->ev_fork, 0));
    GP_TRY(launch_pack_lower(V, ldv, n, RP(c->Vbuf), ld, np, c->aux));
    GP_HIP(hipEventRecord(c->ev_join, c->aux));
  }

  // ---- main stream: metric, kernel matrix, moments, Cholesky of K~ with its inverse
  GP_TRY(build_kernel<R>(c, lane, th, d, dp, n_rows, n_cols, X, ldx, n, np, 0));
  GP_TRY(launch_moments(RP(c->Kvec), RP(c->q), RP(c->Cos), ld, V, ldv, m, r, n, A, lambda0, RP(c->lam_m), RP(c->lam_var), RP(c->fvec),
                        RP(c->wl), c->scal + S_RLAM, c->sumA_part, c->info + INFO_MOMENTS, s));
  phase(1, s);
  {
    // K~ (with its inverse) and V in lock step; K~ alone when V's factor is reused
    CholBatchT<R> cb;
    add_k_chain(cb, c);
    if (!reuse_V) add_v_chain(cb, c);
    cb.ld = ld; cb.ctx = c; cb.side_min = side_min;
    if (!reuse_V) GP_HIP(hipStreamWaitEvent(s, c->ev_join, 0));   // V is packed
    // (K~'s chain in block form: the inverses of the two diagonal halves only -- everything behind substitutes with
    // L21, and the top-level look-ahead on the side stream disappears with the merge)
    if (blocks) GP_TRY(potrf_lockstep<R>(cb, 0, np, 0u, lane, 1u));
    else GP_TRY(potrf_lockstep<R>(cb, 0, np, 1u, lane));
    if (!reuse_V) GP_TRY(launch_logdet(RP(c->LVbuf), ld, n, c->scal + S_LOGDET_V, s));
    phase(3, s);
  }
  GP_TRY(launch_logdet(RP(c->Lbuf), ld, n, c->scal + S_LOGDET_K, s));
  GP_TRY(solve_mean<R>(c, np, blocks, s));

  phase(2, s);
  // ---- everything that needs both factors
  if (mixed_grad) {
    PostJoin<float> pf;
    GP_TRY(demote_for_mixed(c, reuse_V, np, dp, blocks, s, &pf));
    GP_TRY(post_join_list<float>(lane, 1, &c, &pf, &th, n, np, &d, &dp, n_rows, n_cols, want_grad, blocks, phase));
  } else {
    const PostJoin<R> pj = post_join_args<R>(c);
    GP_TRY(post_join_list<R>(lane, 1, &c, &pj, &th, n, np, &d, &dp, n_rows, n_cols, want_grad, blocks, phase));
  }

  if (lam_m_out) GP_HIP(hipMemcpyAsync(lam_m_out, RP(c->lam_m), (size_t)n * sizeof(R), hipMemcpyDeviceToDevice, s));
  if (lam_var_out) GP_HIP(hipMemcpyAsync(lam_var_out, RP(c->lam_var), (size_t)n * sizeof(R), hipMemcpyDeviceToDevice, s));
  if (f_out) GP_HIP(hipMemcpyAsync(f_out, RP(c->fvec), (size_t)n * sizeof(R), hipMemcpyDeviceToDevice, s));
  GP_HIP(hipMemcpyAsync(c->scal_host, c->scal, 64 * sizeof(double), hipMemcpyDeviceToHost, s));
  GP_HIP(hipMemcpyAsync(c->info_host, c->info, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
  phase(7, s);
  c->phase_valid = (c->profile == 2 && want_grad && !reuse_V);
  c->last_enqueue_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
  set_pending(c, s, A, lambda0, th.sigma0, n, np, d, want_grad, (int)sizeof(R), false);
  if (async_call) return 0;
  return fit_eval_finish(c, out_host);
}

// Several independent units (cells, hyperparameter-grid points: SURVEY 8(e)) of the same N in one call, each on
// its own context (its own workspace), all on the caller's stream.  The factorisations of ALL units -- 2 chains
// per unit -- are one lock-step recursion (potrf_lockstep): its latency-bound leaves and small products are
// shared launches, so their cost is paid once per group instead of once per unit; the products behind the
// factorisations share their launches the same way wherever one unit's product cannot fill the chip
// (post_join_list).  Every unit's numbers are bit-identical to gpfit_fit_eval on its own.
// want_grad bits as gpfit_fit_eval (1 gradients, 2 reuse this context's V factor, 8 mixed precision); bit 2
// (asynchronous) is implied: the call returns after enqueuing and the units are collected one by one with
// gpfit_fit_eval_finish.  rc_out[u]: 0 enqueued (collect it), -2 theta outside the limits (out_host[OUT_COUNT u ..]
// already holds the infinite loss / gradients, nothing to collect).
template <typename R>
static int fit_eval_batch_impl(gpfit_ctx* const* cs, int nu, void* stream, const double* theta6, const double* lower,
                               const double* upper, int n_rows, int n_cols, const R* const* X, int64_t ldx, int64_t N,
                               const R* const* r, const R* const* m, const R* const* V, int64_t ldv, const double* logA,
                               const double* lambda0, int want_grad, double* out_host, int* rc_out) {
  auto RP = ws_as<R>;
  const Refuse refuse{"gpfit_fit_eval_batch"};
  if (!cs || nu <= 0 || 2 * nu > GEMM_MAXB || !theta6 || !X || !r || !m || !V || !logA || !lambda0 || !out_host || !rc_out ||
      N <= 0)
    return refuse("bad argument (1 .. 16 units per call)");
  for (int u = 0; u < nu; ++u) {
    if (!cs[u] || !X[u] || !r[u] || !m[u] || !V[u]) return refuse("null context or operand");
    if (const char* why = unit_context_refusal(cs, u, "an asynchronous evaluation is pending on one of the contexts"))
      return refuse(why);
  }
  DeviceGuard device_guard(cs[0]->device);
  hipStream_t s = (hipStream_t)stream;
  const int n = (int)N, np = (int)round_up(N, TILE);
  const int64_t ld = np;
  const bool mixed_grad = (want_grad & 8) != 0 && sizeof(R) == 8 && (want_grad & 1);
  const bool want_reuse = (want_grad & 2) != 0;
  const bool blocks = top_in_blocks(np, sizeof(R));   // as in fit_eval_impl
  want_grad &= 1;
  const auto t_host0 = std::chrono::steady_clock::now();

  struct Unit { gpfit_ctx* c; int u, d, dp; Theta th; double A; bool reuse_V; };
  Unit un[GEMM_MAXB];
  int na = 0;
  for (int u = 0; u < nu; ++u) {
    gpfit_ctx* c = cs[u];
    Admitted ad;
    const int rc = admit(c, "gpfit_fit_eval_batch", "a context's", theta6 + 6 * u, lower, upper, n_rows, n_cols, np,
                         out_host + OUT_COUNT * u, &ad);
    rc_out[u] = rc == -2 ? -2 : 0;
    if (rc == -2) continue;
    if (rc != 0) return rc;
    Unit& q = un[na++];
    q.c = c; q.u = u; q.d = ad.d; q.dp = ad.dp; q.th = ad.th; q.A = std::exp(logA[u]);
    q.reuse_V = want_reuse && c->lv_valid && c->lv_n == n && c->lv_bytes == (int)sizeof(R);
    c->cur_n = n; c->cur_np = np; c->cur_d = q.d; c->cur_dp = q.dp;
    c->phase_valid = false;
    c->side_ev_next = 0;
  }
  if (na == 0) return 0;
  gpfit_ctx* c0 = un[0].c;
  const Lane lane = main_lane(c0, s);   // every launch of the group on the caller's stream with the leader's workspace
  // tuning aid: GPFIT_BATCH_TIMES=1 prints the three phases of every group (synchronises: not for timed runs)
  static const bool batch_times = getenv("GPFIT_BATCH_TIMES") != nullptr;
  hipEvent_t tev[4] = {nullptr, nullptr, nullptr, nullptr};
  if (batch_times) {
    for (auto& e : tev) (void)hipEventCreate(&e);
    (void)hipEventRecord(tev[0], s);
  }
  // Everything on the caller's stream (post_join_list: a group gets its concurrency from batched launches).
  // ---- phase 1, unit by unit: kernel build, moments, V packed (pixel lists, info words and padded means of all
  // units by one launch)
  {
    GroupPrepT<R> gp{};
    gp.n_units = na; gp.n = n; gp.np = np;
    for (int i = 0; i < na; ++i) {
      gpfit_ctx* c = un[i].c;
      gp.pix_host[i] = c->pix_host; gp.pix[i] = c->pix; gp.d[i] = un[i].d; gp.info[i] = c->info;
      gp.m[i] = m[un[i].u]; gp.mpad[i] = RP(c->mpad);
    }
    GP_TRY(launch_group_prepare(gp, s));
  }
  for (int i = 0; i < na; ++i) {
    Unit& q = un[i];
    gpfit_ctx* c = q.c;
    GP_TRY(build_kernel<R>(c, lane, q.th, q.d, q.dp, n_rows, n_cols, X[q.u], ldx, n, np, 0));
    GP_TRY(launch_moments(RP(c->Kvec), RP(c->q), RP(c->Cos), ld, V[q.u], ldv, m[q.u], r[q.u], n, q.A, lambda0[q.u], RP(c->lam_m),
                          RP(c->lam_var), RP(c->fvec), RP(c->wl), c->scal + S_RLAM, c->sumA_part, c->info + INFO_MOMENTS, s));
    if (!q.reuse_V) {
      c->lv_valid = false; c->lv32_valid = false;
      GP_TRY(launch_pack_lower(V[q.u], ldv, n, RP(c->Vbuf), ld, np, s));
    }
  }
  if (batch_times) (void)hipEventRecord(tev[1], s);
  // ---- phase 2: all factorisations in lock step
  {
    CholBatchT<R> cb;
    uint32_t kchains = 0;   // the K~ chains: their inverse factors -- in block form the two diagonal halves only
    for (int i = 0; i < na; ++i) {
      kchains |= 1u << add_k_chain(cb, un[i].c);
      if (!un[i].reuse_V) add_v_chain(cb, un[i].c);
    }
    cb.ld = ld; cb.ctx = nullptr; cb.side_min = 0;
    if (blocks) GP_TRY(potrf_lockstep<R>(cb, 0, np, 0u, lane, kchains));
    else GP_TRY(potrf_lockstep<R>(cb, 0, np, kchains, lane));
  }
  if (batch_times) (void)hipEventRecord(tev[2], s);
  // ---- phase 3: everything that needs the factors
  auto no_phase = [](int, hipStream_t) {};
  gpfit_ctx* cl[GEMM_MAXB];
  Theta thl[GEMM_MAXB];
  int dl[GEMM_MAXB], dpl[GEMM_MAXB];
  PostJoin<R> pjl[GEMM_MAXB];
  PostJoin<float> pfl[GEMM_MAXB];
  for (int i = 0; i < na; ++i) {
    Unit& q = un[i];
    gpfit_ctx* c = q.c;
    cl[i] = c; thl[i] = q.th; dl[i] = q.d; dpl[i] = q.dp;
    if (!q.reuse_V) GP_TRY(launch_logdet_pair(RP(c->Lbuf), c->scal + S_LOGDET_K, RP(c->LVbuf), c->scal + S_LOGDET_V, ld, n, s));
    else GP_TRY(launch_logdet(RP(c->Lbuf), ld, n, c->scal + S_LOGDET_K, s));
    GP_TRY(solve_mean<R>(c, np, blocks, s));
    if (mixed_grad) GP_TRY(demote_for_mixed(c, q.reuse_V, np, q.dp, blocks, s, &pfl[i]));
    else pjl[i] = post_join_args<R>(c);
  }
  if (mixed_grad) GP_TRY(post_join_list<float>(lane, na, cl, pfl, thl, n, np, dl, dpl, n_rows, n_cols, want_grad, blocks, no_phase));
  else GP_TRY(post_join_list<R>(lane, na, cl, pjl, thl, n, np, dl, dpl, n_rows, n_cols, want_grad, blocks, no_phase));
  GP_TRY(closure_collect(Units::all(cl, na), s));
  // one completion event for the group, recorded on the leader's context and waited on by every unit's finish
  if (!c0->pend.done) GP_HIP(hipEventCreateWithFlags(&c0->pend.done, hipEventDisableTiming));
  GP_HIP(hipEventRecord(c0->pend.done, s));
  for (int i = 0; i < na; ++i) {
    Unit& q = un[i];
    gpfit_ctx* c = q.c;
    if (c != c0) {
      // (a context's own event so that it can outlive the leader: recording is a barrier packet, no kernel)
      if (!c->pend.done) GP_HIP(hipEventCreateWithFlags(&c->pend.done, hipEventDisableTiming));
      GP_HIP(hipEventRecord(c->pend.done, s));
    }
    set_pending(c, s, q.A, lambda0[q.u], q.th.sigma0, n, np, q.d, want_grad, (int)sizeof(R), true);
  }
  c0->last_enqueue_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
  if (batch_times) {
    (void)hipEventRecord(tev[3], s);
    (void)hipEventSynchronize(tev[3]);
    float a = 0, b = 0, d3 = 0;
    (void)hipEventElapsedTime(&a, tev[0], tev[1]);
    (void)hipEventElapsedTime(&b, tev[1], tev[2]);
    (void)hipEventElapsedTime(&d3, tev[2], tev[3]);
    fprintf(stderr, "[gpfit batch] %d units: build %.3f ms, lock-step factorisations %.3f ms, post %.3f ms (enqueue %.2f ms)\n", na, a,
            b, d3, c0->last_enqueue_ms);
    for (auto& e : tev) (void)hipEventDestroy(e);
  }
  return 0;
}

// Gradient pull-back for an externally supplied adjoint: out6[p] = sum_ij W_ij dK~_p,ij +
// sum_i gvec_i dKvec_p,i with the reference's analytic dK~_p / dKvec_p (utils.py:996-1021,
// 1036-1044) at theta, WITHOUT materialising any dK: the same contraction to the d x d metric the
// fused full-rank unit uses.  This is what the truncated-rank (B-projected) closure needs once its
// n x n adjoints have been lifted to W = (B G_Kb~ + G_Kb) B^T (utils._closure_projected).
static int grad_pullback_impl(gpfit_ctx* c, void* stream, const double* theta, int n_rows, int n_cols, const double* X,
                              int64_t ldx, int64_t N, const double* W, int64_t ldw, const double* gvec,
                              double* out6) {
  using R = double;
  if (!c || !theta || !X || !W || !gvec || !out6 || N <= 0) {
    set_error("gpfit_grad_pullback: bad argument");
    return -3;
  }
  GP_CTX_ENTER(c, "gpfit_grad_pullback");
  hipStream_t s = (hipStream_t)stream;
  const int n = (int)N, np = (int)round_up(N, TILE);
  Admitted ad;   // (no limits here: theta is wherever the caller's closure was evaluated)
  GP_TRY(admit(c, "gpfit_grad_pullback", "the context", theta, nullptr, nullptr, n_rows, n_cols, np, nullptr, &ad));
  const int d = ad.d, dp = ad.dp;
  const Theta th = ad.th;
  c->lv_valid = false; c->lv32_valid = false;  // the workspace matrices are reused
  const Lane lane = main_lane(c, s);
  GP_HIP(hipMemcpyAsync(c->pix, c->pix_host, (size_t)d * sizeof(int), hipMemcpyHostToDevice, s));
  GP_TRY(build_kernel<R>(c, lane, th, d, dp, n_rows, n_cols, X, ldx, n, np, 0));
  GP_TRY(launch_pack_lower(W, ldw, n, c->Wbuf, (int64_t)np, np, s));
  GP_HIP(hipMemsetAsync(c->bv, 0, (size_t)np * sizeof(R), s));             // no -1/2 b b^T term here
  GP_HIP(hipMemsetAsync(c->wl, 0, (size_t)np * sizeof(R), s));
  GP_TRY(launch_scale_copy<R>(c->wl, gvec, n, -1.0, s));                    // t_i = u_i / q_i + gvec_i
  GP_TRY(pullback_to_metric(c, lane, c->Wbuf, c->Cos, c->q, n, np, dp, c->Abuf, c->Xm, c->Zbuf));
  GP_TRY(launch_metric_contract(th, c->pix, d, n_rows, n_cols, c->Cmat, dp, c->Mmat, dp, c->scal + S_METRIC, c->upart,
                                c->info + INFO_METRIC, s));
  GP_HIP(hipMemcpyAsync(c->scal_host, c->scal, 64 * sizeof(double), hipMemcpyDeviceToHost, s));
  GP_HIP(hipStreamSynchronize(s));
  const double* sc = c->scal_host;
  grad_rows(sc, sigma0_row_metric(sc, th.sigma0) - 2.0 * th.sigma0 * sc[S_ADJ_WL], out6);
  return 0;
}

// The admission of the units of a truncated closure call (gpfit_fit_eval_projected / _sparse and their _batch forms),
// all of it before anything is enqueued or written: every unit's arguments and context, then every unit's admit();
// then rc_out[u] = 0 or -2 with the infinite loss / gradients in the unit's outputs.  U: the units to run (none: the
// call is done); what was found out about them, indexed like the caller's tables.
struct ClosureUnits {
  Units U;
  int nb;   // n_kept padded, shared: the recursion's split depends on it
  int d[CHAIN_MAXU], dp[CHAIN_MAXU], nk[CHAIN_MAXU];
  Theta th[CHAIN_MAXU];
  double A[CHAIN_MAXU];
};
// nk_max / nk_max_name: the bound on n_kept and what the refusal calls it; np: the padded stimuli a context must hold;
// operands(u): the body's own operands of unit u are there; fits(u): what the body asks of the unit's context beyond
// the shared checks -- the sentence of a refusal, or empty.
template <typename Operands, typename Fits>
static int admit_closure_units(const char* name, gpfit_ctx* const* cs, int nu, const double* theta6, const double* lower6,
                               const double* upper6, int n_rows, int n_cols, int np, const int64_t* n_kept, int64_t nk_max,
                               const char* nk_max_name, const int64_t* ldb, const int64_t* ldvb, const double* logA,
                               Operands&& operands, Fits&& fits, double* out_host, int* rc_out, ClosureUnits* a) {
  const Refuse refuse{name};
  a->nb = (int)round_up(n_kept[0], TILE);
  for (int u = 0; u < nu; ++u) {
    const std::string unit = unit_prefix(nu, u);
    if (!cs[u] || !operands(u)) return refuse(unit + "null context or operand");
    if (n_kept[u] <= 0 || n_kept[u] > nk_max)
      return refuse(unit + "bad argument: n_kept " + std::to_string(n_kept[u]) + " is not within 1 .. " + nk_max_name + " = " +
                    std::to_string(nk_max));
    if (ldb[u] < n_kept[u] || ldvb[u] < n_kept[u]) return refuse(unit + "bad leading dimension");
    if (const char* why = unit_context_refusal(cs, u)) return refuse(why);
    // the recursion's split depends on the padded size: only equal padded sizes give the bits of the single call
    if (round_up(n_kept[u], TILE) != a->nb)
      return refuse(unit + "round_up(n_kept, 128) = " + std::to_string(round_up(n_kept[u], TILE)) + " differs from unit 0's " +
                    std::to_string(a->nb) + " (group the units by padded size)");
    const std::string why = fits(u);
    if (!why.empty()) return refuse(unit + why);
  }
  bool outside[CHAIN_MAXU];
  for (int u = 0; u < nu; ++u) {
    double scratch_out[OUT_COUNT];
    Admitted ad;
    const int rc = admit(cs[u], name, nu > 1 ? "a context's" : "the context", theta6 + 6 * u, lower6 ? lower6 + 6 * u : nullptr,
                         upper6 ? upper6 + 6 * u : nullptr, n_rows, n_cols, np, scratch_out, &ad);
    outside[u] = rc == -2;
    if (rc == -2) continue;
    if (rc != 0) return rc;
    a->U.add(cs[u], u);
    a->d[u] = ad.d; a->dp[u] = ad.dp; a->nk[u] = (int)n_kept[u]; a->th[u] = ad.th; a->A[u] = std::exp(logA[u]);
  }
  for (int u = 0; u < nu; ++u) {
    rc_out[u] = outside[u] ? -2 : 0;
    if (outside[u]) fill_out_of_box(out_host + OUT_COUNT * u);
  }
  for (int i = 0; i < a->U.cnt; ++i) {
    gpfit_ctx* c = a->U.ctx[i];
    c->lv_valid = false; c->lv32_valid = false;
    c->side_ev_next = 0;
  }
  return 0;
}

// The operands of the element-wise passes (ProjGroupT) that both closures keep in the same members of a context: n
// training points padded to np; each closure adds the matrices it places differently (am, Kb, aV, Ga, GaKi, P2).
static ProjGroupT closure_group(const ClosureUnits& a, int n, int np, const double* const* r, const double* lambda0) {
  const Units& U = a.U;
  ProjGroupT pg{};
  pg.n_units = U.cnt; pg.n = n; pg.np = np; pg.nb = a.nb; pg.ld = a.nb;
  pg.r = U.from(r); pg.A = U.from(a.A); pg.lambda0 = U.from(lambda0);
  pg.mb = U.of(&gpfit_ctx::mpad); pg.Kvec = U.of(&gpfit_ctx::Kvec); pg.lam_m = U.of(&gpfit_ctx::lam_m);
  pg.lam_var = U.of(&gpfit_ctx::lam_var); pg.f = U.of(&gpfit_ctx::fvec); pg.gm = U.of(&gpfit_ctx::dq1); pg.gv = U.of(&gpfit_ctx::dq2);
  pg.part = U.of(&gpfit_ctx::upart); pg.out3 = U.scal(S_RLAM);
  pg.Ki = U.of(&gpfit_ctx::Vbuf); pg.P1 = U.of(&gpfit_ctx::TmpV); pg.bvec = U.of(&gpfit_ctx::yv);
  pg.mkm = U.scal(S_MKM); pg.G = U.of(&gpfit_ctx::LiVbuf);
  return pg;
}
// Behind a closure's last launch: every unit's scalars and info words to the host, the call's one synchronisation, and
// each unit's 16 outputs and return code.  sigma0_row(scal_host, A, sigma0): the closure's own row of sigma_0.
template <typename Row>
static int closure_finish(const char* name, const ClosureUnits& a, hipStream_t s, const double* lambda0, double* out_host,
                          int* rc_out, Row&& sigma0_row) {
  GP_TRY(closure_collect(a.U, s));
  GP_HIP(hipStreamSynchronize(s));
  const std::string err_K = std::string(name) + ": Cholesky of the projected K_tilde failed (non-positive pivot)";
  const std::string err_V = std::string(name) + ": Cholesky of V_b failed (non-positive pivot)";
  for (int i = 0; i < a.U.cnt; ++i) {
    gpfit_ctx* c = a.U.ctx[i];
    const int u = a.U.at[i];
    rc_out[u] = assemble_out(c, a.A[u], lambda0[u], sigma0_row(c->scal_host, a.A[u], a.th[u].sigma0), 0, a.d[u], 1, err_K.c_str(),
                             err_V.c_str(), out_host + OUT_COUNT * u);
  }
  return 0;
}

// Truncated-rank (B-projected) M-step closure with the inducing set = the training set
// (utils.py:2030-2099 with n < n_tilde = n_t), fused: kernel build, projection on the kept
// eigen-directions B, Cholesky of the n x n matrices, moments / likelihood / KL, the n x n and N x n
// adjoints of the loss, their lift W = (B G_K~b + G_Kb) B^T and the pull-back to the metric, all on
// the device in one call (the algebra of utils._closure_projected).  Every
// N x n matrix lives zero-padded to nb = ceil(n / 128) 128 columns in one of the context's N x N
// work matrices; the n x n ones carry the identity on their padding (log-determinants and solves
// are unaffected, the padding of G_K~b cancels to zero).
// ONE body for gpfit_fit_eval_projected (the group of one) and gpfit_fit_eval_projected_batch: nu independent units, each
// on its own context and this closure's own choice of work matrices, all on the caller's stream with one synchronisation
// at the end -- the structure of fit_eval_sparse_group_impl below.  Unit by unit: the kernel build (the masked pixel count
// differs from unit to unit, and the Gram launch fills the chip alone) and the pull-back (the same, and its slabs go to the
// unit's own Mpart).  For the list: everything between them -- the 2 nu factorisations as one lock-step recursion, the
// products through product / gemm_splitk_list on the list of units, every small kernel as its unit-batched form.  A unit
// runs the same products in the same order with the same slab counts and the same reduction order in every small kernel
// whatever else is in the group, so its 16 outputs have the same bits alone and in any group.  Two things depend on a
// context's capacity -- how many k slabs its scratch holds (gemm_splitk_list) and the route of the lift -- so the
// contexts of one call have one capacity (refused otherwise): the route is decided once per call from shared values
// and is the one each unit takes alone on its context.
// Returns 0, or < 0 before anything is enqueued or any output written; rc_out[u]: 0, -2 (theta outside the unit's limits:
// the infinite loss / gradients in its outputs, nothing enqueued for it) or the LAPACK info of a failed pivot.
static int fit_eval_projected_group_impl(const char* name, gpfit_ctx* const* cs, int nu, void* stream, const double* theta6,
                                         const double* lower6, const double* upper6, int n_rows, int n_cols,
                                         const double* const* X, int64_t ldx, int64_t N, const double* const* r,
                                         const double* const* B, const int64_t* ldb, const int64_t* n_kept,
                                         const double* const* m_b, const double* const* V_b, const int64_t* ldvb,
                                         const double* logA, const double* lambda0, double* out_host, int* rc_out) {
  using R = double;
  const Refuse refuse{name};
  if (nu < 1 || nu > CHAIN_MAXU) return refuse("1 .. " + std::to_string(CHAIN_MAXU) + " units per call");
  if (!cs || !theta6 || !X || !r || !B || !ldb || !n_kept || !m_b || !V_b || !ldvb || !logA || !lambda0 || !out_host || !rc_out ||
      N <= 0 || (lower6 == nullptr) != (upper6 == nullptr))
    return refuse("bad argument");
  const int n = (int)N, np = (int)round_up(N, TILE);
  ClosureUnits ad;
  GP_TRY(admit_closure_units(
      name, cs, nu, theta6, lower6, upper6, n_rows, n_cols, np, n_kept, N, "N", ldb, ldvb, logA,
      [&](int u) { return X[u] && r[u] && B[u] && m_b[u] && V_b[u]; },
      [&](int u) -> std::string {
        // the slabs of the projections and the route of the lift depend on the capacity: one capacity, one route per call
        if (cs[u]->np_cap != cs[0]->np_cap)
          return "the context's capacity of " + std::to_string(cs[u]->np_cap) + " stimuli differs from unit 0's " +
                 std::to_string(cs[0]->np_cap) + " (group the units by the capacity of their contexts)";
        return std::string();
      },
      out_host, rc_out, &ad));
  const Units& U = ad.U;
  const int na = U.cnt, nb = ad.nb;
  if (na == 0) return 0;
  DeviceGuard device_guard(cs[0]->device);
  hipStream_t s = (hipStream_t)stream;
  const int64_t ld = np, lb = nb;
  gpfit_ctx* c0 = U.ctx[0];
  const Lane lane = main_lane(c0, s);   // every launch on the caller's stream with the leader's workspace
  ++g_eval_count;
  prof_begin(c0);
  struct ProfGuard { gpfit_ctx* c; ~ProfGuard() { prof_end(c); } } prof_guard{c0};
  // The work matrices, per context (as ever): Kt = Kbuf, Bp = Lbuf, Kb = Libuf, aV = Tbuf, Ga = Zbuf, GaKi = Tmp, W = Wbuf;
  // the V_b chain in Abuf, Wbuf, Zbuf, Tmp; P2 = Abuf; S1..S4 = Vbuf, LVbuf, LiVbuf, TmpV (n x n, leading dimension nb);
  // mbp = mpad, bvec = yv, gm = dq1, gv = dq2.
  const PerUnit<int> nks = U.from(ad.nk);
  GP_TRY(closure_prepare(U, ad.d, ad.nk, m_b, nb, s));   // pixel lists, info words, the padded m_b, bv / wl cleared
  // ---- unit by unit, the kernel build (as the full-rank unit): C, X masked, cos, Kvec, q, and K~ stored in full by the
  // tiles themselves (mirror): it is multiplied from the left below.  (The masked pixel count differs per unit.)
  for (int i = 0; i < na; ++i) {
    const int u = U.at[i];
    GP_TRY(build_kernel<R>(U.ctx[i], lane, ad.th[u], ad.d[u], ad.dp[u], n_rows, n_cols, X[u], ldx, n, np, 1));
  }
  // ---- projection (utils.py:2047-2049): K_b = K~ B, K~_b = sym(B^T K_b)
  const Mat<R> Kt = U.mats(&gpfit_ctx::Kbuf, ld), Bp = U.mats(&gpfit_ctx::Lbuf, lb), Kb = U.mats(&gpfit_ctx::Libuf, lb),
               aV = U.mats(&gpfit_ctx::Tbuf, lb), GaKi = U.mats(&gpfit_ctx::Tmp, lb);
  const Mat<R> S2 = U.mats(&gpfit_ctx::LVbuf, lb), S3 = U.mats(&gpfit_ctx::LiVbuf, lb), S4 = U.mats(&gpfit_ctx::TmpV, lb);
  GP_TRY(launch_pad_copy_group(na, U.from(B), U.from(ldb), n, nks, U.of(&gpfit_ctx::Lbuf), lb, np, nb, s));
  // (skinny products with a long k are cut into k slabs, gemm_splitk_list, each unit's in its own scratch; Wbuf is free
  // until the adjoints)
  R* part[CHAIN_MAXU];
  int64_t part_elems[CHAIN_MAXU];
  for (int i = 0; i < na; ++i) { part[i] = U.ctx[i]->Wbuf; part_elems[i] = (int64_t)U.ctx[i]->np_cap * U.ctx[i]->np_cap; }
  GP_TRY(gemm_splitk_list(lane, {np, nb, np}, 1.0, plain(Kt), plain(Bp), Kb, part, part_elems));
  GP_TRY(gemm_splitk_list(lane, {nb, nb, np}, 1.0, trans(Bp), plain(Kb), S4, part, part_elems));
  GP_TRY(launch_symmetrize_avg_group(na, U.of(&gpfit_ctx::TmpV), lb, nks, s));                                 // :2048
  GP_TRY(launch_pack_lower_group(na, U.cof(&gpfit_ctx::TmpV), U.same(lb), nks, U.of(&gpfit_ctx::Vbuf), lb, nb, s));
  {
    // (log|V_b| of :1326: V_b is factored together with K~_b -- the 2 na chains as one lock-step recursion on this stream,
    // each unit's V_b chain in four work matrices of its context nothing else needs before the adjoints: Abuf, Wbuf, Zbuf,
    // Tmp, handed over as the last evaluation left them -- the note at ProjChain)
    ProjChain vc[CHAIN_MAXU];
    for (int i = 0; i < na; ++i) {
      gpfit_ctx* c = U.ctx[i];
      vc[U.at[i]] = ProjChain{c->Abuf, c->Wbuf, c->Zbuf, c->Tmp};
    }
    GP_TRY(launch_pack_lower_group(na, U.from(V_b), U.from(ldvb), nks, U.of(&gpfit_ctx::Abuf), lb, nb, s));
    GP_TRY(projected_factor(lane, U, V_b, ldvb, ad.nk, nb, vc));
  }
  // K~_b^-1 is in S1 now.  a V = B V_b, then K~_b^-1 V_b with its trace and K~_b^-1 V_b K~_b^-1 (P1, in S4)
  GP_TRY(product(lane, {np, nb, nb}, 1.0, plain(Bp), plain(S2), into(aV)));
  GP_TRY(projected_kl_products(lane, U, ad.nk, nb));
  // ---- moments / likelihood pieces with a = B and the adjoints G_a, G_Kb, G_K~b (P2 = B^T G_a K~_b^-1 in Abuf)
  ProjGroupT pg = closure_group(ad, n, np, r, lambda0);
  pg.am = U.of(&gpfit_ctx::Lbuf); pg.Kb = U.of(&gpfit_ctx::Libuf); pg.aV = U.of(&gpfit_ctx::Tbuf);
  pg.Ga = U.of(&gpfit_ctx::Zbuf); pg.GaKi = U.of(&gpfit_ctx::Tmp); pg.P2 = U.of(&gpfit_ctx::Abuf);
  GP_TRY(projected_adjoints(lane, pg, part, part_elems));
  GP_TRY(product(lane, {np, nb, nb}, 1.0, plain(Bp), plain(S3), into(GaKi, 1.0)));          // + B G_K~b
  // W = sym((.) B^T).  With P = B G_K~b + G_Kb:  1/2 (P B^T + B P^T) = 1/2 [P | B] [B | P]^T -- ONE product with
  // k = 2 nb that writes the lower tiles only (what the adjoint pass reads): the same flops as the full P B^T, and
  // neither its upper half nor the averaging pass over N x N exist.  (Falls back to the two steps when 2 nb
  // columns do not fit the N x N scratch matrices, i.e. when hardly anything was truncated.)  One route for the call:
  // nb, np and the capacity are shared.
  const Mat<R> W = U.mats(&gpfit_ctx::Wbuf, ld);
  if (2 * (int64_t)nb * np <= (int64_t)c0->np_cap * c0->np_cap) {
    const int64_t l2b = 2 * lb;   // Cat1 = Zbuf, Cat2 = Tbuf: G_a and a V_b are dead
    const PerUnit<const double*> P = U.cof(&gpfit_ctx::Tmp), Bc = U.cof(&gpfit_ctx::Lbuf);
    const PerUnit<double*> Cat1 = U.of(&gpfit_ctx::Zbuf), Cat2 = U.of(&gpfit_ctx::Tbuf);
    const PerUnit<double*> Cat1b = U.of(&gpfit_ctx::Zbuf, nb), Cat2b = U.of(&gpfit_ctx::Tbuf, nb);
    const PerUnit<int64_t> lbs = U.same(lb);
    const PerUnit<int> nbs = U.same(nb);
    GP_TRY(launch_pad_copy_group(na, P, lbs, np, nbs, Cat1, l2b, np, nb, s));
    GP_TRY(launch_pad_copy_group(na, Bc, lbs, np, nbs, Cat1b, l2b, np, nb, s));
    GP_TRY(launch_pad_copy_group(na, Bc, lbs, np, nbs, Cat2, l2b, np, nb, s));
    GP_TRY(launch_pad_copy_group(na, P, lbs, np, nbs, Cat2b, l2b, np, nb, s));
    GP_TRY(product(lane, {np, np, 2 * nb}, 0.5, plain(U.mats(&gpfit_ctx::Zbuf, l2b)), trans(U.mats(&gpfit_ctx::Tbuf, l2b)),
                   into_lower(W)));
  } else {
    GP_TRY(product(lane, {np, np, nb}, 1.0, plain(GaKi), trans(Bp), into(W)));
    GP_TRY(launch_symmetrize_avg_group(na, U.of(&gpfit_ctx::Wbuf), ld, U.same(np), s));
  }
  // ---- unit by unit (the masked pixel count again), the pull-back of <W, dK~_p> + <gvec, dKvec_p> to the metric (as
  // gpfit_grad_pullback; gvec = -g_v; bv and wl were cleared at the start)
  for (int i = 0; i < na; ++i) {
    gpfit_ctx* c = U.ctx[i];
    const int u = U.at[i], d = ad.d[u], dp = ad.dp[u];
    GP_TRY(launch_scale_copy<R>(c->wl, c->dq2, n, 1.0, s));
    GP_TRY(pullback_to_metric(c, lane, c->Wbuf, c->Cos, c->q, n, np, dp, c->Abuf, c->Xm, c->Zbuf));   // G_a's Zbuf is dead
    GP_TRY(launch_metric_contract(ad.th[u], c->pix, d, n_rows, n_cols, c->Cmat, dp, c->Mmat, dp, c->scal + S_METRIC, c->upart,
                                  c->info + INFO_METRIC, s));
  }
  return closure_finish(name, ad, s, lambda0, out_host, rc_out,
                        [](const double* sc, double, double sigma0) { return sigma0_row_metric(sc, sigma0) - 2.0 * sigma0 * sc[S_ADJ_WL]; });
}

// Sparse M-step closure (n_tilde < n_t: K[n_t][n_tilde] != K~, a = K_b K~_b^-1 with non-zero da_p;
// utils.py:2030-2099, 1114-1120), fused like the truncated-rank one above.  Two kernel objects (the
// square K~ on the inducing stimuli and the rectangular K between training and inducing stimuli), the
// same n x n algebra with a = K_b K~_b^-1 in place of B, and two adjoints to pull back:
//   W~  = sym(B G_K~b B^T)   against dK~_p   (square pull-back on the inducing stimuli)
//   W_K = G_Kb B^T           against dK_p    (rectangular pull-back, with the dKvec term riding on it)
// (algebra of utils._closure_sparse).  The two d x d matrices are added before the one contraction
// with dC_p, which is linear in them.
// ONE body for gpfit_fit_eval_sparse (the group of one) and gpfit_fit_eval_sparse_batch: nu independent units, each on
// its own context, all on the caller's stream with one synchronisation at the end.  Unit by unit, as in
// fit_eval_batch_impl: the kernel builds and the pull-backs (the masked pixel count differs from unit to unit and these
// launches fill the chip alone).  Everything between them goes out for the list: the factorisations of all units as one
// lock-step recursion, every product through product on the list of units, every small kernel as its unit-batched
// form.  A unit runs the same products in the same order with the same reduction order in every small kernel whatever
// else is in the group, so its 16 outputs have the same bits alone and in any group.
// Returns 0, or < 0 before anything is enqueued or any output written; rc_out[u]: 0, -2 (theta outside the unit's limits:
// the infinite loss / gradients in its outputs, nothing enqueued for it) or the LAPACK info of a failed pivot.
static int fit_eval_sparse_group_impl(const char* name, gpfit_ctx* const* cs, int nu, void* stream, const double* theta6,
                                      const double* lower6, const double* upper6, int n_rows, int n_cols,
                                      const double* const* X, int64_t ldx, int64_t N, const double* const* Xtilde, int64_t ldxt,
                                      int64_t Ntilde, const double* const* r, const double* const* B, const int64_t* ldb,
                                      const int64_t* n_kept, const double* const* m_b, const double* const* V_b,
                                      const int64_t* ldvb, const double* logA, const double* lambda0, double* out_host,
                                      int* rc_out) {
  using R = double;
  const Refuse refuse{name};
  if (nu < 1 || nu > CHAIN_MAXU) return refuse("1 .. " + std::to_string(CHAIN_MAXU) + " units per call");
  if (!cs || !theta6 || !X || !Xtilde || !r || !B || !ldb || !n_kept || !m_b || !V_b || !ldvb || !logA || !lambda0 || !out_host ||
      !rc_out || N <= 0 || Ntilde <= 0 || (lower6 == nullptr) != (upper6 == nullptr))
    return refuse("bad argument");
  const int n1 = (int)N, n2 = (int)Ntilde;
  const int np1 = (int)round_up(N, TILE), np2 = (int)round_up(Ntilde, TILE);
  ClosureUnits ad;
  GP_TRY(admit_closure_units(
      name, cs, nu, theta6, lower6, upper6, n_rows, n_cols, std::max(np1, np2), n_kept, Ntilde, "Ntilde", ldb, ldvb, logA,
      [&](int u) { return X[u] && Xtilde[u] && r[u] && B[u] && m_b[u] && V_b[u]; }, [](int) { return std::string(); }, out_host,
      rc_out, &ad));
  const Units& U = ad.U;
  const int na = U.cnt, nb = ad.nb;
  if (na == 0) return 0;
  DeviceGuard device_guard(cs[0]->device);
  hipStream_t s = (hipStream_t)stream;
  const int64_t l2 = np2, lb = nb;
  gpfit_ctx* c0 = U.ctx[0];
  const Lane lane = main_lane(c0, s);   // every launch on the caller's stream with the leader's workspace
  ++g_eval_count;
  prof_begin(c0);
  struct ProfGuard { gpfit_ctx* c; ~ProfGuard() { prof_end(c); } } prof_guard{c0};
  // The work matrices, per context (as ever): X1m = Xm, X2m = XDt, Zm = XDt2; Kt = Kbuf, CosT = Cos, Kr = Lbuf,
  // CosR = Libuf, Bp = Tbuf, Kb = Zbuf, am = Tmp, aV = Abuf; S1..S4 = Vbuf, LVbuf, LiVbuf, TmpV; mbp = mpad, bvec = yv,
  // gm = dq1, gv = dq2, gvec = hvec.
  const PerUnit<int> nks = U.from(ad.nk);
  GP_TRY(closure_prepare(U, ad.d, ad.nk, m_b, nb, s));   // pixel lists, info words, the padded m_b, bv / wl cleared
  // ---- unit by unit, the kernel objects: C; training side (x: Xt, XCt, q, Kvec), inducing side (xtilde: Xt2, XCt2, q2);
  // K~ = acosker(xtilde, xtilde), lower tiles mirrored by the tiles themselves; K = acosker(x, xtilde)
  for (int i = 0; i < na; ++i) {
    gpfit_ctx* c = U.ctx[i];
    const int u = U.at[i], d = ad.d[u], dp = ad.dp[u];
    const Theta& th = ad.th[u];
    const double s0sq = th.sigma0 * th.sigma0;
    GP_TRY(build_metric<R>(c, s, th, d, dp, n_rows, n_cols));
    GP_TRY(kernel_side<R>(c, lane, X[u], ldx, n1, np1, d, dp, s0sq, c->Xt, c->XCt, c->Xm, c->Kvec, c->q));
    GP_TRY(kernel_side<R>(c, lane, Xtilde[u], ldxt, n2, np2, d, dp, s0sq, c->Xt2, c->XCt2, c->XDt, c->hvec, c->q2));
    GP_TRY(gram_square<R>(s, c->XCt2, c->Xt2, c->q2, c->Kbuf, c->Cos, n2, np2, dp, s0sq, 1));
    GramArgsT<R> g{};  // K = acosker(x, xtilde): rectangular, with its cosine matrix
    g.XCt = c->XCt; g.Xt = c->Xt2; g.q1 = c->q; g.q2 = c->q2; g.Kout = c->Lbuf; g.Cos = c->Libuf;
    g.ld1 = np1; g.ld2 = l2; g.ldk = l2; g.np1 = np1; g.np2 = np2; g.nv1 = n1; g.nv2 = n2; g.Kd = dp;
    g.s0sq = s0sq; g.lower = 0; g.pad_identity = 0;
    g.ldcos = l2;
    // The Gram kernel leaves K's padding alone, and the projection K B below runs over all np2 columns (against the zero
    // rows of the padded B) and all np1 rows: what an earlier call left there must not reach it -- a stale NaN times
    // zero is NaN.  (On a fresh context the padding already reads zero: the same bits.)
    if (np2 > n2) GP_HIP(hipMemset2DAsync(c->Lbuf + n2, (size_t)l2 * sizeof(R), 0, (size_t)(np2 - n2) * sizeof(R), (size_t)n1, s));
    if (np1 > n1) GP_HIP(hipMemsetAsync(c->Lbuf + (int64_t)n1 * l2, 0, (size_t)(np1 - n1) * l2 * sizeof(R), s));
    ProfScope ps(s, 2.0 * np1 * np2 * dp, 2);
    GP_TRY(launch_gram(g, s));
  }
  // ---- projection (:2047-2049, 2067-2068): K_b = K B, K~_b = sym(B^T K~ B), a = K_b K~_b^-1
  const Mat<R> Kt = U.mats(&gpfit_ctx::Kbuf, l2), Kr = U.mats(&gpfit_ctx::Lbuf, l2), Bp = U.mats(&gpfit_ctx::Tbuf, lb),
               Kb = U.mats(&gpfit_ctx::Zbuf, lb), am = U.mats(&gpfit_ctx::Tmp, lb), aV = U.mats(&gpfit_ctx::Abuf, lb);
  const Mat<R> Ki = U.mats(&gpfit_ctx::Vbuf, lb), S2 = U.mats(&gpfit_ctx::LVbuf, lb), S3 = U.mats(&gpfit_ctx::LiVbuf, lb),
               S4 = U.mats(&gpfit_ctx::TmpV, lb);
  GP_TRY(launch_pad_copy_group(na, U.from(B), U.from(ldb), n2, nks, U.of(&gpfit_ctx::Tbuf), lb, np2, nb, s));
  // (skinny products with a long k are cut into k slabs, gemm_splitk_list; Wbuf is free until the adjoints)
  R* part[CHAIN_MAXU];
  int64_t part_elems[CHAIN_MAXU];
  for (int i = 0; i < na; ++i) { part[i] = U.ctx[i]->Wbuf; part_elems[i] = (int64_t)U.ctx[i]->np_cap * U.ctx[i]->np_cap; }
  GP_TRY(gemm_splitk_list(lane, {np1, nb, np2}, 1.0, plain(Kr), plain(Bp), Kb, part, part_elems));
  GP_TRY(gemm_splitk_list(lane, {np2, nb, np2}, 1.0, plain(Kt), plain(Bp), am, part, part_elems));   // K~ B (temporary)
  GP_TRY(gemm_splitk_list(lane, {nb, nb, np2}, 1.0, trans(Bp), plain(am), S4, part, part_elems));
  GP_TRY(launch_symmetrize_avg_group(na, U.of(&gpfit_ctx::TmpV), lb, nks, s));
  GP_TRY(launch_pack_lower_group(na, U.cof(&gpfit_ctx::TmpV), U.same(lb), nks, U.of(&gpfit_ctx::Vbuf), lb, nb, s));
  {
    // The V_b chain of the lock-step factorisation takes four work matrices that are dead between the projections
    // above and the adjoints below, each of the context's full np_cap^2 size (nb <= np2 <= np_cap: an nb x nb chain
    // fits whatever n_kept is): Wbuf (free until P2), Kbuf and Lbuf (K~ and K are consumed by the projections;
    // rewritten as G_a and G_a K~_b^-1 further down) and Abuf (a V_b is formed behind the chain).  The cosine
    // matrices in Cos / Libuf stay untouched.
    ProjChain vc[CHAIN_MAXU];
    for (int i = 0; i < na; ++i) {
      gpfit_ctx* c = U.ctx[i];
      vc[U.at[i]] = ProjChain{c->Wbuf, c->Kbuf, c->Lbuf, c->Abuf};
    }
    GP_TRY(launch_pack_lower_group(na, U.from(V_b), U.from(ldvb), nks, U.of(&gpfit_ctx::Wbuf), lb, nb, s));
    // tiles above the diagonal read as zero
    GP_TRY(launch_zero3_group(na, U.of(&gpfit_ctx::Kbuf), U.of(&gpfit_ctx::Lbuf), U.of(&gpfit_ctx::Abuf), (int64_t)nb * nb, s));
    GP_TRY(projected_factor(lane, U, V_b, ldvb, ad.nk, nb, vc));
  }
  GP_TRY(projected_kl_products(lane, U, ad.nk, nb));
  GP_TRY(product(lane, {np1, nb, nb}, 1.0, plain(Kb), plain(Ki), into(am)));           // a
  GP_TRY(product(lane, {np1, nb, nb}, 1.0, plain(am), plain(S2), into(aV)));           // a V_b
  // ---- moments / likelihood pieces with a = K_b K~_b^-1, per-point adjoints; G_a = Kbuf, G_a K~_b^-1 = Lbuf [np1][nb]
  ProjGroupT pg = closure_group(ad, n1, np1, r, lambda0);
  pg.am = U.of(&gpfit_ctx::Tmp); pg.Kb = U.of(&gpfit_ctx::Zbuf); pg.aV = U.of(&gpfit_ctx::Abuf);
  pg.Ga = U.of(&gpfit_ctx::Kbuf); pg.GaKi = U.of(&gpfit_ctx::Lbuf); pg.P2 = U.of(&gpfit_ctx::Wbuf);
  for (int i = 0; i < na; ++i) {   // P2's slabs behind P1 in TmpV
    part[i] = U.ctx[i]->TmpV + (int64_t)nb * nb;
    part_elems[i] = (int64_t)U.ctx[i]->np_cap * U.ctx[i]->np_cap - (int64_t)nb * nb;
  }
  GP_TRY(projected_adjoints(lane, pg, part, part_elems));
  // ---- the two adjoints:  W~ = sym(B G_K~b B^T) [np2 x np2],  W_K = G_Kb B^T [np1 x np2]
  GP_TRY(product(lane, {np2, nb, nb}, 1.0, plain(Bp), plain(S3), into(U.mats(&gpfit_ctx::Kbuf, lb))));   // B G_K~b  (G_a is dead)
  GP_TRY(product(lane, {np2, np2, nb}, 1.0, plain(U.mats(&gpfit_ctx::Kbuf, lb)), trans(Bp), into(U.mats(&gpfit_ctx::Wbuf, l2))));
  GP_TRY(launch_symmetrize_avg_group(na, U.of(&gpfit_ctx::Wbuf), l2, U.same(np2), s));
  GP_TRY(product(lane, {np1, np2, nb}, 1.0, plain(U.mats(&gpfit_ctx::Lbuf, lb)), trans(Bp), into(U.mats(&gpfit_ctx::Abuf, l2))));   // W_K  (a V_b is dead)
  // ---- unit by unit, the two pull-backs
  for (int i = 0; i < na; ++i) {
    gpfit_ctx* c = U.ctx[i];
    const int u = U.at[i], d = ad.d[u], dp = ad.dp[u];
    double *X1m = c->Xm, *X2m = c->XDt, *Zm = c->XDt2, *KtU = c->Kbuf, *WK = c->Abuf, *gv = c->dq2, *gvec = c->hvec;
    // square pull-back on the inducing stimuli (no b b^T term, no dKvec term: bv / wl were cleared at the start; A_w
    // into K_b, which is dead; a (Tmp) is dead)
    GP_TRY(pullback_to_metric(c, lane, c->Wbuf, c->Cos, c->q2, n2, np2, dp, c->Zbuf, X2m, c->Tmp));
    // rectangular pull-back (x, xtilde) with gvec = -g_v on the training side (dKvec term)
    GP_TRY(launch_scale_copy<R>(gvec, gv, n1, -1.0, s));
    double* t1 = c->tvec;
    double* t2 = c->tvec + c->np_cap;
    GP_TRY(launch_adjoint_rect(WK, l2, c->Libuf, l2, c->q, c->q2, n1, n2, np1, np2, KtU, l2, c->upart, c->vpart, c->rect_part,
                               gvec, t1, t2, c->rpad, c->mpad, c->scal + S_RECT, s));
    GP_TRY(product(lane, {np1, dp, np2}, 1.0, plain(mat(KtU, l2)), plain(mat(X2m, dp)), into(mat(c->Ybuf, dp))));
    GP_TRY(launch_rowscale_add(c->Ybuf, dp, X1m, dp, t1, np1, dp, s));
    GP_HIP(hipMemsetAsync(Zm, 0, (size_t)np2 * dp * sizeof(double), s));
    GP_TRY(launch_rowscale_add(Zm, dp, X2m, dp, t2, np2, dp, s));
    GP_TRY(xty<R>(c, s, X1m, c->Ybuf, np1, dp, c->dCpad, false));
    GP_TRY(launch_axpby_block<double>(c->Mmat, dp, c->dCpad, dp, dp, dp, 1.0, 1.0, s));
    GP_TRY(xty<R>(c, s, X2m, Zm, np2, dp, c->dCpad, false));
    GP_TRY(launch_axpby_block<double>(c->Mmat, dp, c->dCpad, dp, dp, dp, 1.0, 1.0, s));
    GP_TRY(launch_symmetrize_avg(c->Mmat, dp, dp, s));
    GP_TRY(launch_metric_contract(ad.th[u], c->pix, d, n_rows, n_cols, c->Cmat, dp, c->Mmat, dp, c->scal + S_METRIC, c->upart,
                                  c->info + INFO_METRIC, s));
  }
  return closure_finish(name, ad, s, lambda0, out_host, rc_out, [](const double* sc, double A, double sigma0) {
    const double sum_gvec = 0.5 * A * A * sc[S_SUMF];                                               // -sum g_v
    return sigma0_row_metric(sc, sigma0) + sigma0 * (2.0 * sc[S_RECT] + sc[S_RECT_U1] + sc[S_RECT_U2]) + 2.0 * sigma0 * sum_gvec;
  });
}

// Wait for the evaluation enqueued on this context and assemble its 16 host scalars.
int fit_eval_finish(gpfit_ctx* c, double* out_host) {
  if (!c || !out_host || !c->pend.active) {
    set_error("gpfit_fit_eval_finish: nothing pending on this context");
    return -3;
  }
  c->pend.active = false;
  DeviceGuard device_guard(c->device);
  if (c->pend.use_done && c->pend.done) GP_HIP(hipEventSynchronize(c->pend.done));
  else GP_HIP(hipStreamSynchronize(c->pend.stream));
  const double* sc = c->scal_host;
  const double sigma0 = c->pend.sigma0;
  GP_TRY(assemble_out(c, c->pend.A, c->pend.lambda0, sigma0_row_metric(sc, sigma0) - 2.0 * sigma0 * sc[S_ADJ_WL],
                      c->pend.np - c->pend.n, c->pend.d, c->pend.want_grad, "Cholesky of K_tilde failed: non-positive pivot",
                      "Cholesky of V failed: non-positive pivot", out_host));
  c->lv_valid = true;
  c->lv_n = c->pend.n;
  c->lv_bytes = c->pend.elem_bytes;
  return 0;
}

}  // namespace gpfit

using namespace gpfit;

extern "C" {

int gpfit_fit_eval(gpfit_ctx* c, void* stream, const double* theta, const double* lower, const double* upper,
                   int n_rows, int n_cols, const double* X, int64_t ldx, int64_t N, const double* r,
                   const double* m, const double* V, int64_t ldv, double logA, double lambda0, int want_grad,
                   double* out_host, double* lam_m_out, double* lam_var_out, double* f_out) {
  return fit_eval_impl<double>(c, stream, theta, lower, upper, n_rows, n_cols, X, ldx, N, r, m, V, ldv, logA, lambda0,
                               want_grad, out_host, lam_m_out, lam_var_out, f_out);
}

int gpfit_fit_eval_f32(gpfit_ctx* c, void* stream, const double* theta, const double* lower, const double* upper,
                       int n_rows, int n_cols, const float* X, int64_t ldx, int64_t N, const float* r,
                       const float* m, const float* V, int64_t ldv, double logA, double lambda0, int want_grad,
                       double* out_host, float* lam_m_out, float* lam_var_out, float* f_out) {
  return fit_eval_impl<float>(c, stream, theta, lower, upper, n_rows, n_cols, X, ldx, N, r, m, V, ldv, logA, lambda0,
                              want_grad, out_host, lam_m_out, lam_var_out, f_out);
}

int gpfit_fit_eval_finish(gpfit_ctx* c, double* out_host) { return fit_eval_finish(c, out_host); }

int gpfit_fit_eval_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* theta, const double* lower,
                         const double* upper, int n_rows, int n_cols, const double* const* X, int64_t ldx, int64_t N,
                         const double* const* r, const double* const* m, const double* const* V, int64_t ldv,
                         const double* logA, const double* lambda0, int want_grad, double* out_host, int* rc_out) {
  return fit_eval_batch_impl<double>(ctxs, n_units, stream, theta, lower, upper, n_rows, n_cols, X, ldx, N, r, m, V, ldv,
                                     logA, lambda0, want_grad, out_host, rc_out);
}

int gpfit_fit_eval_batch_f32(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* theta, const double* lower,
                             const double* upper, int n_rows, int n_cols, const float* const* X, int64_t ldx, int64_t N,
                             const float* const* r, const float* const* m, const float* const* V, int64_t ldv,
                             const double* logA, const double* lambda0, int want_grad, double* out_host, int* rc_out) {
  return fit_eval_batch_impl<float>(ctxs, n_units, stream, theta, lower, upper, n_rows, n_cols, X, ldx, N, r, m, V, ldv,
                                    logA, lambda0, want_grad, out_host, rc_out);
}

int gpfit_fit_eval_projected(gpfit_ctx* c, void* stream, const double* theta, const double* lower, const double* upper,
                             int n_rows, int n_cols, const double* X, int64_t ldx, int64_t N, const double* r,
                             const double* B, int64_t ldb, int64_t n_kept, const double* m_b, const double* V_b,
                             int64_t ldvb, double logA, double lambda0, double* out_host) {
  // the group of one (fit_eval_projected_group_impl): a unit's numbers are the same alone and in any group
  int rc = 0;
  const int ret = fit_eval_projected_group_impl("gpfit_fit_eval_projected", &c, 1, stream, theta, lower, upper, n_rows, n_cols, &X,
                                                ldx, N, &r, &B, &ldb, &n_kept, &m_b, &V_b, &ldvb, &logA, &lambda0, out_host, &rc);
  return ret != 0 ? ret : rc;
}

static_assert(GPFIT_FIT_EVAL_PROJECTED_MAX_UNITS == CHAIN_MAXU, "the header states the units of a group call");

int gpfit_fit_eval_projected_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* theta, const double* lower,
                                   const double* upper, int n_rows, int n_cols, const double* const* X, int64_t ldx, int64_t N,
                                   const double* const* r, const double* const* B, const int64_t* ldb, const int64_t* n_kept,
                                   const double* const* m_b, const double* const* V_b, const int64_t* ldvb, const double* logA,
                                   const double* lambda0, double* out_host, int* rc_out) {
  return fit_eval_projected_group_impl("gpfit_fit_eval_projected_batch", ctxs, n_units, stream, theta, lower, upper, n_rows,
                                       n_cols, X, ldx, N, r, B, ldb, n_kept, m_b, V_b, ldvb, logA, lambda0, out_host, rc_out);
}

int gpfit_fit_eval_sparse(gpfit_ctx* c, void* stream, const double* theta, const double* lower, const double* upper,
                          int n_rows, int n_cols, const double* X, int64_t ldx, int64_t N, const double* Xtilde,
                          int64_t ldxt, int64_t Ntilde, const double* r, const double* B, int64_t ldb, int64_t n_kept,
                          const double* m_b, const double* V_b, int64_t ldvb, double logA, double lambda0,
                          double* out_host) {
  // the group of one (fit_eval_sparse_group_impl): a unit's numbers are the same alone and in any group
  int rc = 0;
  const int ret = fit_eval_sparse_group_impl("gpfit_fit_eval_sparse", &c, 1, stream, theta, lower, upper, n_rows, n_cols, &X, ldx, N,
                                             &Xtilde, ldxt, Ntilde, &r, &B, &ldb, &n_kept, &m_b, &V_b, &ldvb, &logA, &lambda0,
                                             out_host, &rc);
  return ret != 0 ? ret : rc;
}

static_assert(GPFIT_FIT_EVAL_SPARSE_MAX_UNITS == CHAIN_MAXU, "the header states the units of a group call");

int gpfit_fit_eval_sparse_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* theta, const double* lower,
                                const double* upper, int n_rows, int n_cols, const double* const* X, int64_t ldx, int64_t N,
                                const double* const* Xtilde, int64_t ldxt, int64_t Ntilde, const double* const* r,
                                const double* const* B, const int64_t* ldb, const int64_t* n_kept, const double* const* m_b,
                                const double* const* V_b, const int64_t* ldvb, const double* logA, const double* lambda0,
                                double* out_host, int* rc_out) {
  return fit_eval_sparse_group_impl("gpfit_fit_eval_sparse_batch", ctxs, n_units, stream, theta, lower, upper, n_rows, n_cols, X,
                                    ldx, N, Xtilde, ldxt, Ntilde, r, B, ldb, n_kept, m_b, V_b, ldvb, logA, lambda0, out_host,
                                    rc_out);
}

int gpfit_grad_pullback(gpfit_ctx* c, void* stream, const double* theta, int n_rows, int n_cols, const double* X,
                        int64_t ldx, int64_t N, const double* W, int64_t ldw, const double* gvec, double* out6) {
  return grad_pullback_impl(c, stream, theta, n_rows, n_cols, X, ldx, N, W, ldw, gvec, out6);
}

int gpfit_ctx_create(int device, int64_t n_max, int64_t d_max, int64_t d_full_max, gpfit_ctx** out) {
  if (!out || n_max <= 0 || d_max <= 0) {
    set_error("gpfit_ctx_create: bad argument");
    return -3;
  }
  DeviceGuard device_guard(device);  // the caller's current device is restored on return
  {
    int cur = -1;
    GP_HIP(hipGetDevice(&cur));
    if (cur != device) {
      set_error("gpfit_ctx_create: cannot select the requested device");
      return -3;
    }
  }
  gpfit_ctx* c = new gpfit_ctx();
  c->device = device;
  c->np_cap = (int)round_up(n_max, TILE);
  c->dp_cap = (int)round_up(d_max, 32);
  c->dfull_cap = (int)std::max<int64_t>(d_full_max, d_max);
  const size_t np = c->np_cap, dp = c->dp_cap, nn = np * np;
  int rc = 0;
  auto A = [&](double** p, size_t cnt) { if (!rc) rc = dev_alloc(c, p, cnt); };
  A(&c->Kbuf, nn); A(&c->Cos, nn); A(&c->Lbuf, nn); A(&c->Libuf, nn); A(&c->Vbuf, nn); A(&c->LVbuf, nn);
  A(&c->LiVbuf, nn); A(&c->Tbuf, nn); A(&c->Zbuf, nn); A(&c->Wbuf, nn); A(&c->Abuf, nn); A(&c->Tmp, nn);
  A(&c->TmpV, nn);
  A(&c->Xt, dp * np); A(&c->Xm, np * dp); A(&c->XCt, dp * np); A(&c->Cmat, dp * dp); A(&c->Ybuf, np * dp);
  A(&c->Mpart, (size_t)c->split_k_M * dp * dp); A(&c->Mmat, dp * dp);
  A(&c->Xt2, dp * np); A(&c->XCt2, dp * np); A(&c->XDt, dp * np); A(&c->XDt2, dp * np); A(&c->dCpad, dp * dp);
  A(&c->q2, np); A(&c->dq1, np); A(&c->dq2, np); A(&c->hvec, np);
  A(&c->Kvec, np); A(&c->q, np); A(&c->lam_m, np); A(&c->lam_var, np); A(&c->fvec, np); A(&c->wl, np);
  A(&c->yv, np); A(&c->bv, np); A(&c->tvec, 2 * np); A(&c->mpad, np); A(&c->rpad, np);
  const size_t t64 = np / 64;
  A(&c->upart, t64 * np); A(&c->vpart, t64 * np); A(&c->sumA_part, t64 * (t64 + 1) / 2);
  A(&c->rect_part, t64 * t64);
  A(&c->frob_part, 33 * (np / TILE) * (np / TILE + 1) / 2); A(&c->trmv_part, (np / TRMV_ROWS + 1) * np);
  A(&c->scal, 64);
  for (int i = 0; i < 2 && !rc; ++i) {
    double* w = nullptr;
    rc = dev_alloc(c, &w, SK_WS_BYTES / sizeof(double));
    c->sk_ws[i] = w;
  }
  if (!rc) rc = dev_alloc(c, &c->pix, (size_t)c->dfull_cap);
  if (!rc) rc = dev_alloc(c, &c->info, 4);
  if (!rc) rc = dev_alloc(c, &c->chain, 1);
  if (rc) {
    gpfit_ctx_destroy(c);
    return rc;
  }
  // pinned AND mapped into the device's address space: the group kernels read pix_host and write scal_host / info_host
  // directly (elementwise.hip: group_prepare_kernel, group_collect_kernel)
  constexpr unsigned HOST_FLAGS = hipHostMallocMapped | hipHostMallocPortable;
  GP_HIP(hipHostMalloc((void**)&c->scal_host, SCAL_HOST_COUNT * sizeof(double), HOST_FLAGS));
  GP_HIP(hipHostMalloc((void**)&c->pix_host, (size_t)c->dfull_cap * sizeof(int), HOST_FLAGS));
  GP_HIP(hipHostMalloc((void**)&c->info_host, 4 * sizeof(int), HOST_FLAGS));
  GP_HIP(hipHostMalloc((void**)&c->chain_host, (size_t)CHAIN_MAX_STEPS * CHAIN_REC * sizeof(double), HOST_FLAGS));
  {
    // the aux stream only packs V while the kernel matrix is being built, off the critical path: lowest priority,
    // so that whenever both streams have work ready the main stream's kernel build is dispatched first
    int least = 0, greatest = 0;
    GP_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    GP_HIP(hipStreamCreateWithPriority(&c->aux, hipStreamNonBlocking, least));
  }
  // (the side stream of the look-ahead is created on first use: ensure_side_stream)
  GP_HIP(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
  GP_HIP(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
  // the strict-upper tiles of every triangular work matrix are never written and must read as 0
  // wherever a dense GEMM touches them (Zbuf is written in full; the others are only read
  // through triangular k ranges) -- zero everything once so no kernel ever sees garbage.
  for (double* p : {c->Kbuf, c->Cos, c->Lbuf, c->Libuf, c->Vbuf, c->LVbuf, c->LiVbuf, c->Tbuf, c->Zbuf, c->Wbuf,
                    c->Abuf, c->Tmp, c->TmpV})
    GP_HIP(hipMemset(p, 0, nn * sizeof(double)));
  GP_HIP(hipDeviceSynchronize());
  *out = c;
  return 0;
}

void gpfit_ctx_destroy(gpfit_ctx* c) {
  if (!c) return;
  DeviceGuard device_guard(c->device);
  (void)hipDeviceSynchronize();
  for (void* p : c->allocs) (void)hipFree(p);
  if (c->pend.done) (void)hipEventDestroy(c->pend.done);
  if (c->scal_host) (void)hipHostFree(c->scal_host);
  if (c->pix_host) (void)hipHostFree(c->pix_host);
  if (c->info_host) (void)hipHostFree(c->info_host);
  if (c->chain_host) (void)hipHostFree(c->chain_host);
  if (c->aux) (void)hipStreamDestroy(c->aux);
  if (c->side) (void)hipStreamDestroy(c->side);
  for (hipEvent_t e : c->side_ev) (void)hipEventDestroy(e);
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  for (hipEvent_t e : c->phase_ev)
    if (e) (void)hipEventDestroy(e);
  delete c;
}

int gpfit_set_profile(gpfit_ctx* c, int on) {
  if (!c) return -3;
  c->profile = (on == 2) ? 2 : (on ? 1 : 0);
  return 0;
}

int gpfit_get_phases(gpfit_ctx* c, double* out8) {
  if (!c || !out8) return -3;
  if (!c->phase_valid) {
    set_error("gpfit_get_phases: no phase-timed evaluation (gpfit_set_profile(ctx, 2), then a synchronous gpfit_fit_eval with gradients)");
    return -3;
  }
  DeviceGuard device_guard(c->device);
  GP_HIP(hipDeviceSynchronize());
  for (int i = 0; i < 8; ++i) {
    float t = 0.f;
    GP_HIP(hipEventElapsedTime(&t, c->phase_ev[0], c->phase_ev[i]));
    out8[i] = t;
  }
  return 0;
}

double gpfit_last_enqueue_ms(gpfit_ctx* c) { return c ? c->last_enqueue_ms : -1.0; }

int gpfit_get_profile(gpfit_ctx* c, double* out16) {
  if (!c || !out16) return -3;
  for (int i = 0; i < 16; ++i) out16[i] = c->prof_out[i];
  return 0;
}

int gpfit_check_limits(const double* theta, const double* lower, const double* upper) {
  return check_limits(theta, lower, upper);
}

int gpfit_localker_mask(const double* theta, int n_rows, int n_cols, uint8_t* mask_host, int64_t* d_out) {
  if (!theta || n_rows <= 0 || n_cols <= 0) {
    set_error("gpfit_localker_mask: bad argument");
    return -3;
  }
  const int d = compute_mask(theta, n_rows, n_cols, mask_host, nullptr);
  if (d_out) *d_out = d;
  return 0;
}


}  // extern "C"
