// C-ABI test hooks of the GEMM launcher: which route a launch takes, the plans of the balanced schedules, and an
// entry point that reaches every field of GemmArgsT (both element types, pointer batches, strided batches,
// split-K, fused epilogues, the pair launch) -- and of the Cholesky recursion: potrf_lockstep on the caller's own
// buffers with every argument exposed -- and of the element-wise and reduction launchers of elementwise.hip, one table
// from an op number to the launcher -- and of the launchers of skinny.hip and the ungated ones of projected.hip.  No
// arithmetic happens here: the hooks fill the launcher's own argument struct and read the launcher's own decision
// (gemm_route, common.h) and its planners.
#include "gemm_core.h"
#include "context.h"
#include "gpfit_mi355x.h"

#include <cstring>

namespace gpfit {
namespace {

template <typename R>
int fill(const gpfit_dev_gemm_args& d, GemmArgsT<R>& g) {
  g = GemmArgsT<R>{};
  g.A = (const R*)d.A; g.B = (const R*)d.B; g.C = (R*)d.C;
  g.lda = d.lda; g.ldb = d.ldb; g.ldc = d.ldc;
  g.M = d.M; g.N = d.N; g.K = d.K;
  g.alpha = d.alpha; g.beta = d.beta;
  g.a_kmajor = d.a_kmajor; g.b_kmajor = d.b_kmajor;
  g.out_lower = d.out_lower; g.a_tri = d.a_tri; g.b_tri = d.b_tri;
  g.batch = d.batch > 0 ? d.batch : 1;
  g.sA = d.sA; g.sB = d.sB; g.sC = d.sC;
  g.split_k = d.split_k > 0 ? d.split_k : 1;
  g.k_slabs = d.k_slabs > 0 ? d.k_slabs : 0;
  g.tile = d.tile;
  g.reverse = d.walk & 15;
  g.half_occ = (d.walk >> 4) & 1;
  g.sk_ws = d.sk_ws;
  g.epi = d.epi;
  g.aux = (R*)d.aux;
  g.sumsq = d.sumsq;
  g.b_split = d.b_split;
  g.nptr = d.nptr;
  if (d.nptr < 0 || d.nptr > GEMM_MAXB) return d.nptr < 0 ? -3 : 0;  // too many: the launcher's own error, no copy
  for (int b = 0; b < d.nptr; ++b) {
    if (!d.Ap || !d.Bp || !d.Cp) return -3;
    g.Ap[b] = (const R*)d.Ap[b];
    g.Bp[b] = (const R*)d.Bp[b];
    g.Cp[b] = (R*)d.Cp[b];
    g.auxp[b] = d.auxp ? (R*)d.auxp[b] : nullptr;
    g.sumsqp[b] = d.sumsqp ? d.sumsqp[b] : nullptr;
  }
  return 0;
}

// The route as the launcher computes it, field by field, and the verdict of the schedule's planner: the table's
// length for an XCD route, the stream-K kernel's grid -- or the planner's decline, with which the launch stays
// data-parallel exactly as launch_gemm then runs it.
template <typename R>
int route(const gpfit_dev_gemm_args& d, const gpfit_dev_gemm_args* d2, gpfit_dev_gemm_route_t& o) {
  std::memset(&o, 0, sizeof(o));
  o.sk_first = -1;
  GemmArgsT<R> a, b;
  if (fill(d, a) != 0 || (d2 && fill(*d2, b) != 0)) return -3;
  GemmRoute r = d2 ? gemm_pair_shape(a, b) : gemm_route(a);
  long blocks = d2 ? r.tiles : -1;   // pair: tiles of both members; stream-K: its kernel's grid; else the route's grid
  if (r.rc == 0 && r.sched == GEMM_STREAMK) {
    SkHostPlan plan;
    if (streamk_plan_host(a, r.sk_first, plan) != 0) r.stay_data_parallel();
    else blocks = plan.blocks;
  }
  if (r.rc == 0 && r.sched == GEMM_XCD) {
    std::vector<int> table;
    if (xcd_plan_host(a, table) != 0) return -3;
    r.gx = (int)table.size();   // as launch_gemm_xcd
  }
  o.rc = r.rc; o.tile = r.tile; o.sk_first = r.sk_first; o.xcd = r.sched == GEMM_XCD; o.stages = r.stages;
  o.half_occ = r.half; o.edge = r.edge; o.epi = r.epi; o.sumsq_entries = r.sumsq_entries; o.slabs = r.slabs;
  o.pair = d2 && r.rc == 0;
  o.blocks = (int)std::min<long>(blocks >= 0 ? blocks : (long)r.gx * r.gy * r.gz, 0x7fffffffL);
  return 0;
}

template <typename R>
int64_t plan(const gpfit_dev_gemm_args& d, int kind, int32_t* out, int64_t cap) {
  GemmArgsT<R> a;
  if (fill(d, a) != 0 || a.M <= 0 || a.N <= 0) return -3;
  const GemmRoute r = gemm_route(a);
  if (r.rc != 0) return -3;
  if (kind == 1) {
    if (r.sched != GEMM_XCD) return -1;
    std::vector<int> table;
    if (xcd_plan_host(a, table) != 0) return -1;
    const int64_t need = 1 + (int64_t)table.size();
    if (need > cap || !out) return need;
    out[0] = (int32_t)table.size();
    std::memcpy(out + 1, table.data(), table.size() * sizeof(int));
    return need;
  }
  if (kind == 4) {
    // the same table, every entry with the k range the kernel gives its tile
    if (r.sched != GEMM_XCD) return -1;
    std::vector<int> table;
    if (xcd_plan_host(a, table) != 0) return -1;
    const int64_t need = 1 + 3 * (int64_t)table.size();
    if (need > cap || !out) return need;
    out[0] = (int32_t)table.size();
    for (size_t e = 0; e < table.size(); ++e) {
      const int t = table[e];
      KRange kr{0, 0};
      if (t >= 0) kr = gemm_tile_k_range(a.a_tri, a.b_tri, a.K, (t >> 16) * TILE, (t & 0xffff) * TILE, TILE, a.b_split);
      out[1 + 3 * e] = t; out[2 + 3 * e] = kr.beg; out[3 + 3 * e] = kr.end;
    }
    return need;
  }
  if (kind == 3) {
    // the slab plan of the triangular-operand route: the items in launch order with their k ranges
    if (a.k_slabs <= 0) return -1;
    const SlabPlan sp = slab_plan(a.M, a.k_slabs);
    const int64_t need = 4 + 4 * (int64_t)sp.items;
    if (need > cap || !out) return need;
    out[0] = sp.items; out[1] = sp.live; out[2] = sp.ks * SLAB_TILE; out[3] = SLAB_TILE;
    for (int e = 0; e < sp.items; ++e) {
      int ti, z;
      slab_item(sp, e, ti, z);
      int32_t* w = out + 4 + 4 * e;
      w[0] = ti; w[1] = z;
      // as the kernel: the tile's k range (the same for every tile column), clipped to the slab
      const KRange kr = gemm_tile_k_range(a.a_tri, a.b_tri, a.K, ti * SLAB_TILE, 0, SLAB_TILE);
      w[2] = std::max(kr.beg, z * sp.ks * SLAB_TILE);
      w[3] = std::min(kr.end, (z + 1) * sp.ks * SLAB_TILE);
    }
    return need;
  }
  if (kind != 2) return -3;
  if (r.sched != GEMM_STREAMK) return -1;
  const int first = r.sk_first;
  SkHostPlan p;
  if (streamk_plan_host(a, first, p) != 0) return -1;
  const int64_t nt = (int64_t)p.tiles.size(), nfix = (int64_t)p.fix_tile.size(), nslot = (int64_t)p.fix_slot.size();
  const int64_t need = 8 + 5 * nt + nfix + (nfix + 1) + nslot;
  if (need > cap || !out) return need;
  out[0] = first; out[1] = (int32_t)nt; out[2] = p.total; out[3] = p.blocks; out[4] = p.per_block;
  out[5] = (int32_t)nfix; out[6] = (int32_t)nslot;
  out[7] = (int32_t)(SK_WS_BYTES / ((size_t)TILE * TILE * sizeof(double)));
  int32_t* w = out + 8;
  for (const SkTile& t : p.tiles) { *w++ = t.row0; *w++ = t.col0; *w++ = t.kbeg; *w++ = t.ksteps; *w++ = t.prefix; }
  std::memcpy(w, p.fix_tile.data(), nfix * sizeof(int)); w += nfix;
  std::memcpy(w, p.fix_ptr.data(), (nfix + 1) * sizeof(int)); w += nfix + 1;
  std::memcpy(w, p.fix_slot.data(), nslot * sizeof(int));
  return need;
}

template <typename R>
int run(hipStream_t s, const gpfit_dev_gemm_args& d, const gpfit_dev_gemm_args* d2) {
  GemmArgsT<R> a, b;
  if (fill(d, a) != 0 || (d2 && fill(*d2, b) != 0)) {
    set_error("gpfit_dev_gemm: a pointer batch needs its pointer arrays");
    return -3;
  }
  return d2 ? launch_gemm_pair(a, b, gemm_pair_shape(a, b), s) : launch_gemm(a, s);
}

// The one table of the floating-point device work buffers of a context: every one gpfit_ctx_create allocates, by the
// member's name (the stream-K workspaces as sk_ws[0] and sk_ws[1]), with the byte size of that allocation.  A test fills
// them (gpfit_dev_ctx_fill) to show that no entry point reads what an earlier call left behind.  Deliberately absent:
//   pix          -- pixel indices: a stale one is an address, and a test that filled it could cause a wild read; the
//                   tests built on this table must not be able to provoke a fault
//   info         -- words 2 and 3 are tickets whose contract is "0 between calls" (INFO_MOMENTS, INFO_METRIC)
//   chain        -- the ChainBlock holds step counters and flags beside its numbers
//   scal_host, pix_host, info_host, chain_host -- pinned host memory, written by the host as well
// (tests/test_context_cases_cpu.py holds this table against the members of gpfit_ctx.)
struct CtxBuf { const char* name; void* p; int64_t bytes; };
std::vector<CtxBuf> ctx_buffers(gpfit_ctx* c) {
  const int64_t np = c->np_cap, dp = c->dp_cap, nn = np * np * 8, nd = np * dp * 8, dd = dp * dp * 8, v = np * 8;
  const int64_t t64 = np / 64, t128 = np / TILE;
  return {
      // N x N work matrices
      {"Kbuf", c->Kbuf, nn}, {"Cos", c->Cos, nn}, {"Lbuf", c->Lbuf, nn}, {"Libuf", c->Libuf, nn}, {"Vbuf", c->Vbuf, nn},
      {"LVbuf", c->LVbuf, nn}, {"LiVbuf", c->LiVbuf, nn}, {"Tbuf", c->Tbuf, nn}, {"Zbuf", c->Zbuf, nn}, {"Wbuf", c->Wbuf, nn},
      {"Abuf", c->Abuf, nn}, {"Tmp", c->Tmp, nn}, {"TmpV", c->TmpV, nn},
      // N x d / d x d
      {"Xt", c->Xt, nd}, {"Xm", c->Xm, nd}, {"XCt", c->XCt, nd}, {"Cmat", c->Cmat, dd}, {"Ybuf", c->Ybuf, nd},
      {"Mpart", c->Mpart, (int64_t)c->split_k_M * dd}, {"Mmat", c->Mmat, dd}, {"Xt2", c->Xt2, nd}, {"XCt2", c->XCt2, nd},
      {"XDt", c->XDt, nd}, {"XDt2", c->XDt2, nd}, {"dCpad", c->dCpad, dd},
      // vectors
      {"Kvec", c->Kvec, v}, {"q", c->q, v}, {"lam_m", c->lam_m, v}, {"lam_var", c->lam_var, v}, {"fvec", c->fvec, v},
      {"wl", c->wl, v}, {"yv", c->yv, v}, {"bv", c->bv, v}, {"tvec", c->tvec, 2 * v}, {"mpad", c->mpad, v}, {"rpad", c->rpad, v},
      {"q2", c->q2, v}, {"dq1", c->dq1, v}, {"dq2", c->dq2, v}, {"hvec", c->hvec, v},
      // partial sums
      {"upart", c->upart, t64 * v}, {"vpart", c->vpart, t64 * v}, {"sumA_part", c->sumA_part, t64 * (t64 + 1) / 2 * 8},
      {"frob_part", c->frob_part, 33 * t128 * (t128 + 1) / 2 * 8}, {"trmv_part", c->trmv_part, (np / TRMV_ROWS + 1) * v},
      {"rect_part", c->rect_part, t64 * t64 * 8},
      // device scalars and the stream-K workspaces
      {"scal", c->scal, 64 * 8}, {"sk_ws[0]", c->sk_ws[0], (int64_t)SK_WS_BYTES}, {"sk_ws[1]", c->sk_ws[1], (int64_t)SK_WS_BYTES}};
}
CtxBuf ctx_buffer(gpfit_ctx* c, const char* name) {
  for (const CtxBuf& t : ctx_buffers(c))
    if (std::strcmp(t.name, name) == 0) return t;
  return {nullptr, nullptr, 0};
}

// potrf_lockstep on the caller's buffers: nothing but the batch struct is filled here
template <typename R>
int potrf(gpfit_ctx* c, hipStream_t s, int nb, void* const* A, void* const* L, void* const* Li, void* const* Tmp,
          int* const* info, int64_t ld, int n, uint32_t need, uint32_t halves, int side_min) {
  CholBatchT<R> B;
  B.nb = nb;
  for (int b = 0; b < nb; ++b) {
    B.A[b] = (R*)A[b]; B.L[b] = (R*)L[b]; B.Li[b] = (R*)Li[b]; B.Tmp[b] = (R*)Tmp[b];
    B.info[b] = info[b];
  }
  B.ld = ld;
  if (side_min > 0) {
    GP_TRY(ensure_side_stream(c));
    B.ctx = c; B.side_min = side_min;
    c->side_ev_next = 0;   // as the closures do at the head of a call: the events of the look-ahead are reused
  }
  return potrf_lockstep<R>(B, 0, n, need, main_lane(c, s), halves);
}

// ---- the element-wise launchers by number (gpfit_dev_elementwise): a table from the op to its launch_* function
// what an op requires: the pointers p[0 .. nptr), the extents n[0 .. nsize) >= 1; f32: the launcher has a float instance
struct EwSpec { int nptr, nsize; bool f32; };
constexpr EwSpec EW_SPEC[GPFIT_EW_NOPS] = {
    /* TRMV_LOWER */ {3, 1, true},   /* TRMV_LOWER_T */ {4, 1, true},    /* SYMV_LOWER */ {3, 1, false},
    /* GEMV_SUB */ {4, 2, true},     /* GEMV_T_SUB */ {5, 2, true},      /* DOT */ {3, 1, true},
    /* LOGDET */ {2, 1, true},       /* LOGDET_PAIR */ {4, 1, true},     /* FROB_LOWER */ {3, 1, true},
    /* FROB_TILES */ {2, 2, true},   /* REDUCE_SLICES */ {2, 1, true},   /* REDUCE_SLABS */ {2, 4, true},
    /* REDUCE_SLICES_SYM */ {2, 2, true}, /* PACK_LOWER */ {2, 2, true}, /* PACK_TRI */ {2, 2, false},
    /* UNPACK_SYM */ {2, 1, false},  /* UNPACK_TRI */ {2, 1, false},     /* SYMMETRIZE */ {1, 1, true},
    /* SYMMETRIZE_AVG */ {1, 1, false}, /* PAD_COPY */ {2, 4, false},    /* GATHER */ {2, 4, true},
    /* ESTEP_BUILD */ {5, 2, false}, /* ADD_DIAG */ {1, 1, true},        /* AXPBY_BLOCK */ {2, 2, true},
    /* DEMOTE_BLOCK */ {2, 2, false}, /* QVEC */ {4, 3, true},           /* MOMENTS */ {13, 1, true},
    /* ADJOINT */ {8, 2, true},      /* ADJOINT_REDUCE */ {8, 4, true},  /* ADJOINT_RECT */ {13, 4, false},
    /* METRIC_CONTRACT */ {6, 3, true}, /* DK_SIGMA0 */ {4, 2, false},   /* DQ */ {3, 2, false},
    /* DK_METRIC */ {6, 2, false},   /* ESTEP_PREP */ {5, 2, false},     /* ROWSCALE_ADD */ {3, 2, true},
};

// the multiples the launchers state for their extents (kernels.h); launch_gather and launch_gemv_t_sub refuse their own
bool ew_multiples(int op, const int32_t* n) {
  switch (op) {
    case GPFIT_EW_TRMV_LOWER_T: return n[0] % 64 == 0;
    case GPFIT_EW_FROB_LOWER: return n[0] % TILE == 0;
    case GPFIT_EW_FROB_TILES: return n[0] % TILE == 0 && n[1] % TILE == 0;
    case GPFIT_EW_PACK_LOWER: case GPFIT_EW_ESTEP_BUILD: return n[1] % TILE == 0;
    case GPFIT_EW_ADJOINT: return n[1] % 64 == 0;
    case GPFIT_EW_ADJOINT_RECT: return n[2] % 64 == 0 && n[3] % 64 == 0;
    case GPFIT_EW_AXPBY_BLOCK: return n[1] % 2 == 0;
    default: return true;
  }
}

template <typename R>
int ew_single(hipStream_t s, int op, const gpfit_dev_ew_args& a) {
  void* const* p = a.p;
  const int64_t* ld = a.ld;
  const int32_t* n = a.n;
  auto in = [&](int k) { return (const R*)p[k]; };
  auto out = [&](int k) { return (R*)p[k]; };
  auto din = [&](int k) { return (const double*)p[k]; };
  auto dout = [&](int k) { return (double*)p[k]; };
  switch (op) {
    case GPFIT_EW_TRMV_LOWER: return launch_trmv_lower<R>(in(0), ld[0], n[0], in(1), out(2), s);
    case GPFIT_EW_TRMV_LOWER_T: return launch_trmv_lower_t<R>(in(0), ld[0], n[0], in(1), out(2), dout(3), s);
    case GPFIT_EW_GEMV_SUB: return launch_gemv_sub<R>(in(0), ld[0], n[0], n[1], in(1), in(2), out(3), s);
    case GPFIT_EW_GEMV_T_SUB: return launch_gemv_t_sub<R>(in(0), ld[0], n[0], n[1], in(1), in(2), out(3), dout(4), s);
    case GPFIT_EW_DOT: return launch_dot<R>(in(0), in(1), n[0], dout(2), s);
    case GPFIT_EW_LOGDET: return launch_logdet<R>(in(0), ld[0], n[0], dout(1), s);
    case GPFIT_EW_LOGDET_PAIR: return launch_logdet_pair<R>(in(0), dout(1), in(2), dout(3), ld[0], n[0], s);
    case GPFIT_EW_FROB_LOWER: return launch_frob_lower<R>(in(0), ld[0], n[0], dout(1), dout(2), s);
    case GPFIT_EW_FROB_TILES: return launch_frob_tiles<R>(in(0), ld[0], n[0], n[1], n[2], dout(1), s);
    case GPFIT_EW_REDUCE_SLICES: return launch_reduce_slices<R, R>(in(0), ld[0], n[0], out(1), ld[1], s);
    case GPFIT_EW_REDUCE_SLABS: return launch_reduce_slabs<R>(in(0), ld[0], n[0], n[1], out(1), n[2], n[3], s);
    case GPFIT_EW_REDUCE_SLICES_SYM: return launch_reduce_slices_sym<R>(in(0), ld[0], n[0], out(1), n[1], s);
    case GPFIT_EW_PACK_LOWER: return launch_pack_lower<R>(in(0), ld[0], n[0], out(1), ld[1], n[1], s);
    case GPFIT_EW_SYMMETRIZE: return launch_symmetrize<R>(out(0), ld[0], n[0], s);
    case GPFIT_EW_GATHER:
      return launch_gather<R>(in(0), ld[0], n[0], (const int*)p[2], n[1], n[2], n[3], out(1), ld[1], out(3), ld[2], s);
    case GPFIT_EW_ADD_DIAG: return launch_add_diag<R>(out(0), ld[0], n[0], a.s[0], s);
    case GPFIT_EW_AXPBY_BLOCK: return launch_axpby_block<R>(out(0), ld[0], in(1), ld[1], n[0], n[1], a.s[0], a.s[1], s);
    case GPFIT_EW_QVEC: return launch_qvec<R>(in(0), in(1), ld[0], n[2], n[0], n[1], a.s[0], out(2), out(3), s);
    case GPFIT_EW_MOMENTS:
      return launch_moments<R>(in(0), in(1), in(2), ld[0], in(3), ld[1], in(4), in(5), n[0], a.s[0], a.s[1], out(6), out(7),
                               out(8), out(9), dout(10), dout(11), (int*)p[12], s);
    case GPFIT_EW_ADJOINT:
      return launch_adjoint<R>(in(0), in(1), ld[0], in(2), in(3), n[0], n[1], out(4), dout(5), dout(6), dout(7), s);
    case GPFIT_EW_ADJOINT_REDUCE:
      return launch_adjoint_reduce<R>(din(0), din(1), din(2), n[2], n[3], in(3), in(4), n[0], n[1], out(5), dout(6), dout(7),
                                      s);
    case GPFIT_EW_METRIC_CONTRACT: {
      Theta th;
      static_assert(sizeof(Theta) == sizeof(a.theta), "gpfit_dev_ew_args::theta is Theta as its doubles");
      std::memcpy(&th, a.theta, sizeof(th));
      return launch_metric_contract<R>(th, (const int*)p[0], n[0], n[1], n[2], in(1), ld[0], in(2), ld[1], dout(3), dout(4),
                                       (int*)p[5], s);
    }
    case GPFIT_EW_ROWSCALE_ADD: return launch_rowscale_add<R>(out(0), ld[0], in(1), ld[1], in(2), n[0], n[1], s, a.s[0]);
    default: break;
  }
  return -3;
}

// the launchers that exist for double only
int ew_single_f64(hipStream_t s, int op, const gpfit_dev_ew_args& a) {
  void* const* p = a.p;
  const int64_t* ld = a.ld;
  const int32_t* n = a.n;
  auto in = [&](int k) { return (const double*)p[k]; };
  auto out = [&](int k) { return (double*)p[k]; };
  switch (op) {
    case GPFIT_EW_SYMV_LOWER: return launch_symv_lower(in(0), ld[0], n[0], in(1), out(2), s);
    case GPFIT_EW_PACK_TRI: return launch_pack_tri(in(0), ld[0], n[0], out(1), ld[1], n[1], s);
    case GPFIT_EW_UNPACK_SYM: return launch_unpack_sym(in(0), ld[0], n[0], out(1), ld[1], s);
    case GPFIT_EW_UNPACK_TRI: return launch_unpack_tri(in(0), ld[0], n[0], out(1), ld[1], s);
    case GPFIT_EW_SYMMETRIZE_AVG: return launch_symmetrize_avg(out(0), ld[0], n[0], s);
    case GPFIT_EW_PAD_COPY: return launch_pad_copy(in(0), ld[0], n[0], n[1], out(1), ld[1], n[2], n[3], s);
    case GPFIT_EW_ESTEP_BUILD: return launch_estep_build(in(0), ld[0], n[0], n[1], in(1), out(2), out(3), out(4), ld[1], s);
    case GPFIT_EW_DEMOTE_BLOCK: return launch_demote_block(in(0), ld[0], (float*)p[1], ld[1], n[0], n[1], s);
    case GPFIT_EW_ADJOINT_RECT:
      return launch_adjoint_rect(in(0), ld[0], in(1), ld[1], in(2), in(3), n[0], n[1], n[2], n[3], out(4), ld[2], out(5), out(6),
                                 out(7), in(13), out(8), out(9), out(10), out(11), out(12), s);
    case GPFIT_EW_DK_SIGMA0: return launch_dk_sigma0(in(0), ld[0], in(1), in(2), n[0], n[1], a.s[0], out(3), ld[1], s);
    case GPFIT_EW_DQ: return launch_dq(in(0), in(1), ld[0], n[1], n[0], in(2), out(3), out(4), s);
    case GPFIT_EW_DK_METRIC: return launch_dk_metric(out(0), ld[0], in(1), ld[1], in(2), in(3), in(4), in(5), n[0], n[1], s);
    case GPFIT_EW_ESTEP_PREP: return launch_estep_prep(in(0), in(1), in(2), n[0], n[1], a.s[0], out(3), out(4), s);
    default: break;
  }
  return ew_single<double>(s, op, a);
}

// the unit-batched launchers: the host tables copied into PerUnit<>, a common value where no table is given
template <typename T>
PerUnit<T> ew_ptrs(const gpfit_dev_ew_args& a, int k) {
  PerUnit<T> r{};
  for (int u = 0; u < a.n_units; ++u) r.v[u] = a.up[k] ? (T)a.up[k][u] : nullptr;
  return r;
}
PerUnit<int> ew_sizes(const gpfit_dev_ew_args& a, int k) {
  PerUnit<int> r{};
  for (int u = 0; u < a.n_units; ++u) r.v[u] = a.un[k] ? a.un[k][u] : a.n[k];
  return r;
}
PerUnit<int64_t> ew_lds(const gpfit_dev_ew_args& a, int k) {
  PerUnit<int64_t> r{};
  for (int u = 0; u < a.n_units; ++u) r.v[u] = a.uld[k] ? a.uld[k][u] : a.ld[k];
  return r;
}
PerUnit<double> ew_scalars(const gpfit_dev_ew_args& a, int k) {
  PerUnit<double> r{};
  for (int u = 0; u < a.n_units; ++u) r.v[u] = a.us[k] ? a.us[k][u] : a.s[k];
  return r;
}

int ew_group(hipStream_t s, int op, const gpfit_dev_ew_args& a) {
  const int nu = a.n_units;
  const int64_t* ld = a.ld;
  const int32_t* n = a.n;
  auto in = [&](int k) { return ew_ptrs<const double*>(a, k); };
  auto out = [&](int k) { return ew_ptrs<double*>(a, k); };
  switch (op) {
    case GPFIT_EW_TRMV_LOWER: return launch_trmv_lower_group(nu, out(0), ld[0], n[0], out(1), out(2), s);
    case GPFIT_EW_TRMV_LOWER_T: return launch_trmv_lower_t_group(nu, out(0), ld[0], n[0], out(1), out(2), out(3), s);
    case GPFIT_EW_SYMV_LOWER: return launch_symv_lower_group(nu, out(0), ld[0], n[0], out(1), out(2), s);
    case GPFIT_EW_DOT: return launch_dot_group(nu, out(0), out(1), n[0], out(2), s);
    case GPFIT_EW_LOGDET_PAIR: return launch_logdet_pair_group(nu, in(0), out(1), in(2), out(3), ld[0], ew_sizes(a, 0), s);
    case GPFIT_EW_REDUCE_SLICES: return launch_reduce_slices_group(nu, out(0), ld[0], n[0], out(1), ld[1], s);
    case GPFIT_EW_PACK_LOWER:
      return launch_pack_lower_group(nu, in(0), ew_lds(a, 0), ew_sizes(a, 0), out(1), ld[1], n[1], s);
    case GPFIT_EW_PACK_TRI: return launch_pack_tri_group(nu, in(0), ew_lds(a, 0), ew_sizes(a, 0), out(1), ld[1], n[1], s);
    case GPFIT_EW_SYMMETRIZE: return launch_symmetrize_group(nu, out(0), ld[0], n[0], s);
    case GPFIT_EW_SYMMETRIZE_AVG: return launch_symmetrize_avg_group(nu, out(0), ld[0], ew_sizes(a, 0), s);
    case GPFIT_EW_PAD_COPY:
      return launch_pad_copy_group(nu, in(0), ew_lds(a, 0), ew_sizes(a, 0), ew_sizes(a, 1), out(1), ld[1], n[2], n[3], s);
    case GPFIT_EW_GATHER:
      return launch_gather_group(nu, in(0), ew_lds(a, 0), ew_sizes(a, 0), ew_ptrs<const int*>(a, 2), ew_sizes(a, 1), n[2], n[3],
                                 out(1), ld[1], s);
    case GPFIT_EW_ADD_DIAG: return launch_add_diag_group(nu, out(0), ld[0], n[0], a.s[0], s);
    case GPFIT_EW_QVEC:
      return launch_qvec_group(nu, in(0), in(1), ld[0], n[2], ew_sizes(a, 0), n[1], ew_scalars(a, 0), out(2), out(3), s);
    default: break;
  }
  return -3;
}

// what a wrong test could turn into a wild access, refused before any launch
bool ew_valid(int op, int is_f32, const gpfit_dev_ew_args& a) {
  const bool group = (op & GPFIT_EW_GROUP) != 0;
  const int base = op & ~GPFIT_EW_GROUP;
  if (base < 0 || base >= GPFIT_EW_NOPS) return false;
  const EwSpec sp = EW_SPEC[base];
  if (is_f32 && (group || !sp.f32)) return false;
  if (!group) {
    for (int k = 0; k < sp.nptr; ++k) if (!a.p[k]) return false;
    for (int k = 0; k < sp.nsize; ++k) if (a.n[k] < 1) return false;
    if (base == GPFIT_EW_REDUCE_SLICES && a.ld[1] < 1) return false;
    return ew_multiples(base, a.n);
  }
  if (a.n_units < 1 || a.n_units > CHAIN_MAXU) return false;
  for (int k = 0; k < sp.nptr; ++k) {
    if (!a.up[k]) return false;
    for (int u = 0; u < a.n_units; ++u) if (!a.up[k][u]) return false;
  }
  for (int k = 0; k < sp.nsize; ++k)
    for (int u = 0; u < a.n_units; ++u) if ((a.un[k] ? a.un[k][u] : a.n[k]) < 1) return false;
  if (base == GPFIT_EW_REDUCE_SLICES && a.ld[1] < 1) return false;
  return ew_multiples(base, a.n);   // the extents with a stated multiple are common to the units
}

// ---- the launchers of skinny.hip (gpfit_dev_skinny): the hook's struct into SkinnyArgs / SkinnySumArgs, field by field
bool skinny_valid(int op, const gpfit_dev_skinny_args& d) {
  if (d.kc < 1 || d.kc > SKINNY_LD) return false;
  switch (op) {
    case GPFIT_SKINNY_SLABS: return d.A && d.B && d.O && d.M >= 1 && d.K >= 1 && d.tri >= 0 && d.tri <= 2;
    case GPFIT_SKINNY_SUM:
      if (!d.P || !d.dst || d.M < 1 || d.nslab < 1 || d.tri < 0 || d.tri > 2) return false;
      if (d.mode == SKINNY_SUM_PLAIN) return true;
      if (d.mode == SKINNY_SUM_ROWS) return d.L && d.Li && d.n >= 1;
      if (d.mode == SKINNY_SUM_SCHUR) return d.Kc && d.n >= 1;
      return false;
    case GPFIT_SKINNY_FINISH: return d.Lt && d.Lit && d.L && d.Li && d.logdet && d.n >= 1;
    default: return false;
  }
}

int skinny_run(hipStream_t s, int op, const gpfit_dev_skinny_args& d) {
  if (op == GPFIT_SKINNY_SLABS) {
    SkinnyArgs g{};
    g.A = d.A; g.sam = d.sam; g.sar = d.sar;
    g.B = d.B; g.sbr = d.sbr; g.sbc = d.sbc;
    g.O = d.O; g.soz = d.soz; g.som = d.som; g.soc = d.soc;
    g.alpha = d.alpha;
    g.M = d.M; g.K = d.K; g.kc = d.kc; g.tri = d.tri;
    return launch_skinny_slabs(g, s);
  }
  if (op == GPFIT_SKINNY_SUM) {
    SkinnySumArgs r{};
    r.P = d.P; r.pz = d.pz;
    r.M = d.M; r.kc = d.kc; r.nslab = d.nslab; r.tri = d.tri; r.mode = d.mode;
    r.dst = d.dst;
    r.L = d.L; r.ldl = d.ldl; r.Li = d.Li; r.ldi = d.ldi; r.n = d.n;
    r.Kc = d.Kc; r.ldk = d.ldk;
    return launch_skinny_sum(r, s);
  }
  return launch_append_block_finish(d.Lt, d.Lit, d.L, d.ldl, d.Li, d.ldi, d.n, d.kc, d.logdet, s);
}

// ---- the ungated launchers of projected.hip (gpfit_dev_projected): the host tables copied into ProjGroupT / PerUnit<>
// how many of up[] (group ops) or p[] (single launchers) an op requires; p[4] of ESTEP_SCALE (aLp) may be NULL
constexpr int PROJ_NPTR[GPFIT_PROJ_NOPS] = {13, 6, 3, 5, 2, 6, 6, 5};

bool proj_valid(int op, const gpfit_dev_proj_args& d) {
  if (op < 0 || op >= GPFIT_PROJ_NOPS) return false;
  if (op >= GPFIT_PROJ_ESTEP_ROWS) {
    for (int k = 0; k < PROJ_NPTR[op]; ++k)
      if (!d.p[k] && !(op == GPFIT_PROJ_ESTEP_SCALE && k == 4)) return false;
    if (d.n < 1 || d.nb < 1) return false;
    if (op == GPFIT_PROJ_ESTEP_MOMENTS) return d.ld >= d.nb;
    if (d.nrows < d.n || d.nrows % 32 != 0 || d.lda < d.nb) return false;
    return op == GPFIT_PROJ_ESTEP_ROWS || (d.npc >= 1 && d.ld >= d.npc);
  }
  if (d.n_units < 1 || d.n_units > CHAIN_MAXU) return false;
  for (int k = 0; k < PROJ_NPTR[op]; ++k) {
    if (!d.up[k]) return false;
    for (int u = 0; u < d.n_units; ++u) if (!d.up[k][u]) return false;
  }
  if (op == GPFIT_PROJ_TRACE) {
    if (!d.un || d.ld < 1) return false;
    for (int u = 0; u < d.n_units; ++u) if (d.un[u] < 1) return false;
    return true;
  }
  if (d.nb < 1 || d.ld < d.nb) return false;
  if (op == GPFIT_PROJ_GKTB) return true;
  if (d.n < 1) return false;
  if (op == GPFIT_PROJ_MOMENTS) return d.uA && d.ulambda0;
  return d.np >= d.n;
}

template <typename T>
PerUnit<T> proj_ptrs(const gpfit_dev_proj_args& d, int k) {
  PerUnit<T> r{};
  for (int u = 0; u < d.n_units; ++u) r.v[u] = (T)d.up[k][u];
  return r;
}

int proj_run(hipStream_t s, int op, const gpfit_dev_proj_args& d) {
  auto in = [&](int k) { return (const double*)d.p[k]; };
  auto out = [&](int k) { return (double*)d.p[k]; };
  auto up = [&](int k) { return proj_ptrs<double*>(d, k); };
  switch (op) {
    case GPFIT_PROJ_ESTEP_ROWS:
      return launch_estep_proj_rows(in(0), d.lda, d.nb, in(1), in(2), in(3), d.n, d.nrows, d.A, out(4), out(5), s);
    case GPFIT_PROJ_ESTEP_SCALE:
      return launch_estep_proj_scale(in(0), d.lda, d.nb, d.n, d.nrows, in(1), in(2), out(3), out(4), d.ld, d.npc, out(5), s);
    case GPFIT_PROJ_ESTEP_MOMENTS: return launch_estep_proj_moments(in(0), d.ld, d.nb, in(1), in(2), d.n, out(3), out(4), s);
    case GPFIT_PROJ_TRACE: {
      PerUnit<int> n{};
      for (int u = 0; u < d.n_units; ++u) n.v[u] = d.un[u];
      return launch_proj_trace_group(d.n_units, up(0), d.ld, n, up(1), s);
    }
    default: break;
  }
  ProjGroupT g{};
  g.n_units = d.n_units; g.n = d.n; g.np = d.np; g.nb = d.nb; g.ld = d.ld;
  switch (op) {
    case GPFIT_PROJ_MOMENTS:
      g.am = up(0); g.Kb = up(1); g.aV = up(2); g.mb = up(3); g.Kvec = up(4); g.r = proj_ptrs<const double*>(d, 5);
      g.lam_m = up(6); g.lam_var = up(7); g.f = up(8); g.gm = up(9); g.gv = up(10); g.part = up(11); g.out3 = up(12);
      for (int u = 0; u < d.n_units; ++u) { g.A.v[u] = d.uA[u]; g.lambda0.v[u] = d.ulambda0[u]; }
      return launch_proj_moments_group(g, s);
    case GPFIT_PROJ_GA:
      g.Kb = up(0); g.aV = up(1); g.gm = up(2); g.gv = up(3); g.mb = up(4); g.Ga = up(5);
      return launch_proj_ga_group(g, s);
    case GPFIT_PROJ_GKB:
      g.am = up(0); g.gv = up(1); g.GaKi = up(2);
      return launch_proj_gkb_group(g, s);
    default:
      g.Ki = up(0); g.P1 = up(1); g.P2 = up(2); g.bvec = up(3); g.G = up(4);
      return launch_proj_gktb_group(g, s);
  }
}

}  // namespace
}  // namespace gpfit

extern "C" {

int gpfit_dev_skinny(gpfit_ctx* ctx, void* stream, int op, const gpfit_dev_skinny_args* args) {
  if (!ctx || !args || !gpfit::skinny_valid(op, *args)) {
    gpfit::set_error("gpfit_dev_skinny: bad argument");
    return -3;
  }
  GP_CTX_ENTER(ctx, "gpfit_dev_skinny");
  return gpfit::skinny_run((hipStream_t)stream, op, *args);
}

int gpfit_dev_projected(gpfit_ctx* ctx, void* stream, int op, const gpfit_dev_proj_args* args) {
  if (!ctx || !args || !gpfit::proj_valid(op, *args)) {
    gpfit::set_error("gpfit_dev_projected: bad argument");
    return -3;
  }
  GP_CTX_ENTER(ctx, "gpfit_dev_projected");
  return gpfit::proj_run((hipStream_t)stream, op, *args);
}

int gpfit_dev_elementwise(gpfit_ctx* ctx, void* stream, int op, int is_f32, const gpfit_dev_ew_args* args) {
  if (!ctx || !args || !gpfit::ew_valid(op, is_f32, *args)) {
    gpfit::set_error("gpfit_dev_elementwise: bad argument");
    return -3;
  }
  GP_CTX_ENTER(ctx, "gpfit_dev_elementwise");
  hipStream_t s = (hipStream_t)stream;
  if (op & GPFIT_EW_GROUP) return gpfit::ew_group(s, op & ~GPFIT_EW_GROUP, *args);
  if (op == GPFIT_EW_REDUCE_SLICES && !is_f32 && args->n[1] == 1)   // double slices into a float destination
    return gpfit::launch_reduce_slices<double, float>((const double*)args->p[0], args->ld[0], args->n[0], (float*)args->p[1],
                                                      args->ld[1], s);
  return is_f32 ? gpfit::ew_single<float>(s, op, *args) : gpfit::ew_single_f64(s, op, *args);
}

int gpfit_dev_gemm_route(int is_f32, const gpfit_dev_gemm_args* args, const gpfit_dev_gemm_args* pair_args,
                         gpfit_dev_gemm_route_t* out) {
  if (!args || !out) return -3;
  return is_f32 ? gpfit::route<float>(*args, pair_args, *out) : gpfit::route<double>(*args, pair_args, *out);
}

int64_t gpfit_dev_gemm_plan(int is_f32, const gpfit_dev_gemm_args* args, int kind, int32_t* out, int64_t cap) {
  if (!args) return -3;
  return is_f32 ? gpfit::plan<float>(*args, kind, out, cap) : gpfit::plan<double>(*args, kind, out, cap);
}

int gpfit_dev_gemm(void* stream, int is_f32, const gpfit_dev_gemm_args* args, const gpfit_dev_gemm_args* pair_args) {
  if (!args) return -3;
  return is_f32 ? gpfit::run<float>((hipStream_t)stream, *args, pair_args)
                : gpfit::run<double>((hipStream_t)stream, *args, pair_args);
}

int gpfit_dev_potrf(gpfit_ctx* ctx, void* stream, int is_f32, int nb, void* const* A, void* const* L, void* const* Li,
                    void* const* Tmp, int* const* info, int64_t ld, int n, uint32_t need, uint32_t halves, int side_min) {
  const int64_t elem = is_f32 ? 4 : 8;
  bool ok = ctx && A && L && Li && Tmp && info && nb >= 1 && nb <= gpfit::GEMM_MAXB && n > 0 && n % gpfit::TILE == 0 &&
            ld >= n && (ld * elem) % 16 == 0 && side_min >= 0;
  if (ok) {
    const uint32_t all = nb >= 32 ? 0xffffffffu : ((1u << nb) - 1u);
    ok = ((need | halves) & ~all) == 0;
    for (int b = 0; b < nb && ok; ++b) ok = A[b] && L[b] && Li[b] && Tmp[b] && info[b];
  }
  if (!ok) {
    gpfit::set_error("gpfit_dev_potrf: bad argument");
    return -3;
  }
  GP_CTX_ENTER(ctx, "gpfit_dev_potrf");
  return is_f32 ? gpfit::potrf<float>(ctx, (hipStream_t)stream, nb, A, L, Li, Tmp, info, ld, n, need, halves, side_min)
                : gpfit::potrf<double>(ctx, (hipStream_t)stream, nb, A, L, Li, Tmp, info, ld, n, need, halves, side_min);
}

int gpfit_dev_ctx_copy(gpfit_ctx* ctx, const char* name, int64_t offset, void* dev, int64_t bytes, int to_ctx) {
  if (!ctx || !name || !dev || offset < 0 || bytes < 0 || ctx->pend.active) return -3;
  gpfit::DeviceGuard guard(ctx->device);
  const gpfit::CtxBuf b = gpfit::ctx_buffer(ctx, name);
  if (!b.p || offset + bytes > b.bytes) return -3;
  GP_HIP(hipDeviceSynchronize());
  char* w = (char*)b.p + offset;
  GP_HIP(hipMemcpy(to_ctx ? (void*)w : dev, to_ctx ? dev : (void*)w, (size_t)bytes, hipMemcpyDeviceToDevice));
  GP_HIP(hipDeviceSynchronize());
  return 0;
}

int gpfit_dev_ctx_buffer_name(int index, char* out, int cap) {
  // the names do not depend on the context: the table of an empty one has them all
  gpfit_ctx none;
  const std::vector<gpfit::CtxBuf> tab = gpfit::ctx_buffers(&none);
  if (index < 0 || index >= (int)tab.size() || !out || cap <= (int)std::strlen(tab[index].name)) return -3;
  std::strcpy(out, tab[index].name);
  return 0;
}

int gpfit_dev_ctx_fill(gpfit_ctx* ctx, const char* name, int byte) {
  if (!ctx || !name || ctx->pend.active) return -3;
  gpfit::DeviceGuard guard(ctx->device);
  const gpfit::CtxBuf b = gpfit::ctx_buffer(ctx, name);
  if (!b.p) return -3;
  GP_HIP(hipDeviceSynchronize());
  GP_HIP(hipMemset(b.p, byte, (size_t)b.bytes));
  GP_HIP(hipDeviceSynchronize());
  return 0;
}

}  // extern "C"
