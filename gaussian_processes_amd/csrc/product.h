// How the host code writes one GEMM launch down: C = alpha op(A) op(B) + beta C as the algebra states it, for one
// problem or for a list of problems of one shape.  Internal header.
//   product(lane, {M, N, K}, alpha, plain(a) | trans(a), plain(b) | trans(b), into(c, beta) | into_lower(c, beta), walk, &epilogue)
// (on_tiles(into(c), 64): the same product on the block tile named)
// a, b, c are Mats: mat(p, ld) names one matrix block, mats(cnt, ld, i -> pointer) the same block of every problem of
// a list; tril(m) / triu(m) state the triangle of the block AS STORED (what op() makes of it is derived).  A block
// named through a pointer to const is a Mat<const R>: an operand, never an output (into() of it does not compile).
// That check costs templates beyond R, a deliberate exception: mats deduces its element type from the callable, plain /
// trans are overloaded on constness, fit.hip's block helpers take the matrix as a pointer to member (ts_blk, lambdas).
#pragma once
#include "context.h"
#include <type_traits>

namespace gpfit {

enum Tri { Dense = 0, Lower = 1, Upper = 2 };   // the values of GemmArgsT::a_tri / b_tri
struct Dims { int M, N, K; };                   // op(A) is M x K, op(B) is K x N

// one row-major block (leading dimension ld) in each of cnt problems; R is const-qualified for a read-only block
template <typename R> struct Mat { int cnt; int64_t ld; Tri tri; R* p[GEMM_MAXB]; };
template <typename R>
Mat<R> mat(R* p, int64_t ld) {
  Mat<R> m{};
  m.cnt = 1; m.ld = ld; m.p[0] = p;
  return m;
}
// at(i): problem i's block; the element type is that of the pointer it returns (more than a launch holds: product refuses)
template <typename F>
auto mats(int cnt, int64_t ld, F&& at) {
  Mat<std::remove_pointer_t<decltype(at(0))>> m{};
  m.cnt = cnt; m.ld = ld;
  for (int i = 0; i < cnt && i < GEMM_MAXB; ++i) m.p[i] = at(i);
  return m;
}
template <typename R> Mat<R> tril(Mat<R> m) { m.tri = Lower; return m; }
template <typename R> Mat<R> triu(Mat<R> m) { m.tri = Upper; return m; }

// op(X): X as stored, or transposed; an operand is read only, whatever it was named through
// split > 0: op(B) only -- dense left of column `split`, lower triangular from it on (m.tri says Lower), those columns
// read from p2 (GemmArgsT::b_split, B2)
template <typename R> struct Operand { Mat<const R> m; bool t; int split = 0; const R* p2[GEMM_MAXB] = {}; };
template <typename R> Operand<R> plain(const Mat<const R>& m) { return {m, false}; }
template <typename R> Operand<R> trans(const Mat<const R>& m) { return {m, true}; }
template <typename R> Operand<R> plain(const Mat<R>& m) {
  Operand<R> o{{m.cnt, m.ld, m.tri, {}}, false};
  for (int i = 0; i < m.cnt && i < GEMM_MAXB; ++i) o.m.p[i] = m.p[i];
  return o;
}
template <typename R> Operand<R> trans(const Mat<R>& m) { Operand<R> o = plain(m); o.t = true; return o; }
// [dense | lower]: the columns left of `col` from `dense`, the lower triangle from column `col` on from `lower`, both
// named by the block's origin (column 0) and of one leading dimension
template <typename R> Operand<R> dense_then_lower(const Mat<R>& dense, const Mat<const R>& lower, int col) {
  Operand<R> o = plain(tril(dense));
  o.split = col;
  for (int i = 0; i < lower.cnt && i < GEMM_MAXB; ++i) o.p2[i] = lower.p[i];
  return o;
}

// lower: the tiles on / below the diagonal only; tile: 0 the launcher's choice, else the block tile asked for
template <typename R> struct Output { Mat<R> m; bool lower; double beta; int tile = 0; };
template <typename R> Output<R> into(const Mat<R>& m, double beta = 0.0) { return {m, false, beta}; }
template <typename R> Output<R> into_lower(const Mat<R>& m, double beta = 0.0) { return {m, true, beta}; }
template <typename R> Output<R> on_tiles(Output<R> o, int tile) { o.tile = tile; return o; }

// A fused epilogue (GemmArgsT::epi): the request -- which one (0: none) and its per-problem operands -- and the
// launcher's answer: carried by all launches of the product or by none, and the sumsq entries each left per problem.
template <typename R> struct Epilogue { int which; R* aux[GEMM_MAXB]; double* sumsq[GEMM_MAXB]; bool carried; int sumsq_entries; };

// THE translation into GemmArgsT (problem 0 of a list), and the only place that knows the layout flags: op(A) is
// [M][K], so A as stored is a_kmajor 0 and A transposed 1; op(B) is [K][N], so B as stored is b_kmajor 1 and B
// transposed 0 (common.h); the triangle of op(X) is X's own, swapped when X is transposed.
template <typename R>
GemmArgsT<R> product_args(Lane lane, Dims d, double alpha, const Operand<R>& a, const Operand<R>& b, const Output<R>& c,
                          int walk = 0) {
  auto tri = [](const Operand<R>& o) { return (o.t && o.m.tri != Dense) ? (int)Lower + (int)Upper - (int)o.m.tri : (int)o.m.tri; };
  GemmArgsT<R> g{};
  g.A = a.m.p[0]; g.B = b.m.p[0]; g.C = c.m.p[0];
  g.lda = a.m.ld; g.ldb = b.m.ld; g.ldc = c.m.ld;
  g.M = d.M; g.N = d.N; g.K = d.K;
  g.alpha = alpha; g.beta = c.beta;
  g.a_kmajor = a.t ? 1 : 0; g.b_kmajor = b.t ? 0 : 1;
  g.out_lower = c.lower ? 1 : 0; g.a_tri = tri(a); g.b_tri = tri(b);
  g.batch = 1; g.split_k = 1; g.reverse = walk; g.sk_ws = lane.sk_ws;
  g.b_split = b.split; g.B2 = b.split > 0 ? b.p2[0] : nullptr;
  g.tile = c.tile;
  return g;
}
// the same as ONE pointer-batched launch over all problems of the list, with the epilogue's request (if any)
template <typename R>
GemmArgsT<R> batch_args(Lane lane, Dims d, double alpha, const Operand<R>& a, const Operand<R>& b, const Output<R>& c,
                        int walk = 0, const Epilogue<R>* e = nullptr) {
  GemmArgsT<R> g = product_args(lane, d, alpha, a, b, c, walk);
  g.nptr = g.batch = c.m.cnt;
  for (int i = 0; i < c.m.cnt; ++i) {
    g.Ap[i] = a.m.p[i]; g.Bp[i] = b.m.p[i]; g.Cp[i] = c.m.p[i];
    g.auxp[i] = e ? e->aux[i] : nullptr; g.sumsqp[i] = e ? e->sumsq[i] : nullptr;
  }
  g.epi = e ? e->which : 0;
  return g;
}

// fit.hip.  run_gemm: the single place that logs (GPFIT_GEMM_LOG) and profiles a launch, on its route r.
// product: the problems of a list as one pointer-batched launch, unless the product is a 128-tile launch already for a
// single problem -- then problem by problem through the ordinary launcher (one problem: always).
template <typename R> int run_gemm(hipStream_t s, const GemmArgsT<R>& g, const GemmRoute& r);
template <typename R> int run_gemm(hipStream_t s, const GemmArgsT<R>& g) { return run_gemm(s, g, gemm_route(g)); }
template <typename R>
int product(Lane lane, Dims d, double alpha, const Operand<R>& a, const Operand<R>& b, const Output<R>& c, int walk = 0,
            Epilogue<R>* e = nullptr);

}  // namespace gpfit
