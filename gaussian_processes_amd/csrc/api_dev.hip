// C-ABI test hooks of the GEMM launcher: which route a launch takes, the plans of the balanced schedules, and an
// entry point that reaches every field of GemmArgsT (both element types, pointer batches, strided batches,
// split-K, fused epilogues, the pair launch) -- and of the Cholesky recursion: potrf_lockstep on the caller's own
// buffers with every argument exposed.  No arithmetic happens here: the hooks fill the launcher's own argument
// struct and read the launcher's own decision (gemm_route, common.h) and its planners.
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

// a work buffer of the context by name, with its size in bytes
struct CtxBuf { void* p; int64_t bytes; };
CtxBuf ctx_buffer(gpfit_ctx* c, const char* name) {
  const int64_t np = c->np_cap, dp = c->dp_cap, nn = np * np * 8;
  const struct { const char* n; double* p; int64_t bytes; } tab[] = {
      {"Abuf", c->Abuf, nn}, {"Tbuf", c->Tbuf, nn}, {"Wbuf", c->Wbuf, nn}, {"Zbuf", c->Zbuf, nn}, {"Cos", c->Cos, nn},
      {"TmpV", c->TmpV, nn}, {"Tmp", c->Tmp, nn}, {"Kbuf", c->Kbuf, nn}, {"Xm", c->Xm, np * dp * 8}, {"Xt2", c->Xt2, np * dp * 8}, {"Ybuf", c->Ybuf, np * dp * 8},
      {"Mmat", c->Mmat, dp * dp * 8}, {"Cmat", c->Cmat, dp * dp * 8}, {"tvec", c->tvec, 2 * np * 8}, {"bv", c->bv, np * 8},
      {"q", c->q, np * 8}, {"wl", c->wl, np * 8}, {"q2", c->q2, np * 8}, {"dq1", c->dq1, np * 8}, {"dq2", c->dq2, np * 8}};
  for (const auto& t : tab)
    if (std::strcmp(t.n, name) == 0) return {t.p, t.bytes};
  return {nullptr, 0};
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

}  // namespace
}  // namespace gpfit

extern "C" {

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
