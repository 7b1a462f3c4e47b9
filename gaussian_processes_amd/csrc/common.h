// Shared declarations for the MI355X (gfx950) GP-fit library.  Internal header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

namespace gpfit {

// float32-rounded pi: the reference overwrites torch.pi before switching the default
// dtype to float64 (reference utils.py:25 vs :33), so every pi in its kernel is this value.
constexpr double PI32 = 3.1415927410125732;

constexpr int TILE = 128;  // GEMM block tile (M and N) and Cholesky leaf size
constexpr int TRMV_ROWS = 128;  // rows per block of the transposed triangular matrix-vector product (partials: np / TRMV_ROWS slices)
constexpr int KTILE = 16;  // fp64 GEMM K step staged through LDS (fp32: 32, see ktile_of)

void set_error(const std::string& msg);

#define GP_HIP(expr)                                                                     \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      gpfit::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));               \
      return -100;                                                                       \
    }                                                                                    \
  } while (0)

// the same for the library's own int-returning functions: hand a non-zero code up
#define GP_TRY(expr)            \
  do {                          \
    int _rc = (expr);           \
    if (_rc != 0) return _rc;   \
  } while (0)

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// ---- MFMA GEMM (fp64, and fp32 for the theta-grid configuration) ----------------------
// C[M,N] = alpha * op(A)[M,K] * op(B)[K,N] + beta * C        (row-major storage)
//   a_kmajor = 0 : A stored [M][K] (k contiguous)   element (m,k) at A[m*lda + k]
//   a_kmajor = 1 : A stored [K][M] (m contiguous)   element (m,k) at A[k*lda + m]
//   b_kmajor = 1 : B stored [K][N] (n contiguous)   element (k,n) at B[k*ldb + n]
//   b_kmajor = 0 : B stored [N][K] (k contiguous)   element (k,n) at B[n*ldb + k]
// Triangular structure is exploited per block tile:
//   out_lower   : only the 128-blocks on/below the block diagonal are computed / written (M == N)
//   a_tri/b_tri : 0 dense, 1 op() is lower triangular, 2 op() is upper triangular
//                 (restricts each tile's k range; the skipped part must hold zeros or is
//                  simply never read)
// K must be a multiple of the K step (16 for fp64, 32 for fp32); M, N arbitrary (edges are
// predicated); lda/ldb multiples of 16 bytes.
constexpr int GEMM_MAXB = 32;  // problems of one pointer-batched launch (GemmArgsT::nptr)

template <typename R>
struct GemmArgsT {
  const R* A;
  const R* B;
  R* C;
  int64_t lda, ldb, ldc;
  int M, N, K;
  double alpha, beta;
  int a_kmajor, b_kmajor;
  int out_lower;
  int a_tri, b_tri;
  int batch;                 // number of independent problems (grid.y)
  int64_t sA, sB, sC;        // batch strides (elements)
  int split_k;               // >1: partial products written to C + z*sC (beta ignored)
  int k_slabs;               // >0: the triangular-operand route (a_tri == 2, square op(A), M == K a multiple of 64):
                             // 64-tiles, k cut into at most k_slabs fixed slabs of whole tiles (slab_plan below),
                             // one workgroup per (tile, slab) whose k range is not empty, heavy items first; slab z of
                             // a row panel goes to C + z*sC (beta ignored) and the panel's live slabs are
                             // z >= panel / tiles-per-slab.  A function of (M, k_slabs) alone: the same cut for one
                             // problem and for a pointer batch.
  int tile;                  // 0 = choose (128 / 64 / 32), else forced block tile
  int reverse;               // tile walk (gemm_walk_tile, gemm_core.h): bit 0 backwards, bit 1 column-major, bit 2 k
                             // downwards, bit 3 ask for the XCD-aware table
  int half_occ;              // 1: pad the launch with unused dynamic LDS so that only ONE workgroup of it fits on
                             // a CU: a long GEMM off the critical path then leaves half of every CU (79 KiB
                             // of LDS, 320 VGPRs) to the latency-bound kernels of the critical chain instead
                             // of holding every workgroup slot of the chip for its whole duration
  void* sk_ws;               // caller-owned stream-K workspace (>= SK_WS_BYTES); nullptr: process-wide one
  int b_split;               // > 0 (a multiple of 128, b_tri == 1): op(B) is dense left of column b_split and lower
                             // triangular from it on, the triangle's origin at that column: [T21 | T22] = C [S | LV22]
                             // as one launch.  The columns from b_split on are read from B2 (indexed like B: element
                             // (k, n) of op(B) at the same offset) where B2 is set.  One problem on the XCD-aware table
                             // only, which leaves out the tiles whose k range is empty: they stay unwritten
                             // (gemm_route refuses every other launch of this kind)
  const int* sched;          // device tile table of an XCD-aware schedule (gemm_sched.hip), or nullptr: set by
                             // launch_gemm_xcd, callers leave it null (the table's length is the route's grid)
  // Fused epilogues of the data-parallel launches (gemm.hip; a launch that takes the stream-K schedule cannot
  // honour them -- gemm_route().epi says what a launch carries).  Bit mask:
  //   1  mirror: square lower output, every stored element below the diagonal is also stored transposed
  //      (replaces a symmetrisation pass over the matrix)
  //   2  tile norms: sum of squares of the stored values of 128-tile (ti, tj) in sumsq[ti (ti + 1) / 2 + tj] (lower
  //      output) or sumsq[ti tiles_n + tj] (full output)
  //      (128-tile launches only; replaces a pass over the matrix; on the stream-K schedule split
  //      tiles leave theirs per fix-up band behind the per-tile table: GemmRoute::sumsq_entries)
  //   4  dual update: with D = aux (same leading dimension as C), C = alpha op(A) op(B) + D and then
  //      aux = C + D (beta is ignored; replaces a copy and an axpby pass)
  //   8  added matrix: C = alpha op(A) op(B) + aux, aux only read (beta is ignored; replaces a copy of aux into C)
  int epi;
  R* aux;
  double* sumsq;
  // Pointer batch: nptr > 0 independent problems of the same shape, problem b (= blockIdx.y) on Ap[b], Bp[b],
  // Cp[b] instead of A, B, C and the strides.  This is how the latency-bound levels of several Cholesky
  // recursions (the K~ and V chains of one unit, the chains of several units in flight) and the sibling blocks of
  // the two-sided product share their launches: the matrices live in separately allocated workspaces, so there is
  // no common stride.  Data-parallel launches only (no stream-K, no schedule table); fused epilogues take their
  // per-problem operands from auxp / sumsqp.
  int nptr;
  const R* Ap[GEMM_MAXB];
  const R* Bp[GEMM_MAXB];
  R* Cp[GEMM_MAXB];
  R* auxp[GEMM_MAXB];        // epi 4: problem b's aux
  double* sumsqp[GEMM_MAXB]; // epi 2: problem b's tile-norm table
  const R* B2;               // b_split: the matrix the columns from b_split on are read from (nullptr: B)
};
using GemmArgs = GemmArgsT<double>;

// ---- the slab plan of the triangular-operand route (GemmArgsT::k_slabs)
// op(A) is upper triangular on nt x nt tiles of SLAB_TILE: row panel ti needs the k tiles [ti, nt).  k is cut into
// slabs of ks = ceil(nt / S) tiles (live slabs: ceil(nt / ks) <= S) and an item is a (panel, slab) pair whose
// k range [max(ti, z ks), min((z + 1) ks, nt)) is not empty.  Items in launch order, heavy first: the full ones
// (ti <= z ks, slab by slab), then those that start r = ti - z ks = 1, 2, .. tiles into their slab (ks - r tiles
// each; the last slab's are clipped at nt).  Kernel and host hooks enumerate through slab_item and nothing else.
constexpr int SLAB_TILE = 64;
struct SlabPlan {
  int nt, ks, live;   // tiles per side, tiles per slab, live slabs
  int full, rb;       // number of full items; partial items with r < rb exist in every live slab, the rest in all but the last
  int items;
};
__host__ __device__ inline SlabPlan slab_plan(int M, int slabs) {
  SlabPlan p;
  p.nt = (M + SLAB_TILE - 1) / SLAB_TILE;
  p.ks = (p.nt + slabs - 1) / slabs;
  p.live = (p.nt + p.ks - 1) / p.ks;
  p.full = p.live + p.ks * (p.live * (p.live - 1) / 2);
  p.rb = p.nt - (p.live - 1) * p.ks;
  p.items = p.full + (p.rb - 1) * p.live + (p.ks - p.rb) * (p.live - 1);
  return p;
}
__host__ __device__ inline void slab_item(const SlabPlan& p, int e, int& ti, int& z) {
  if (e < p.full) {
    for (z = 0; e >= z * p.ks + 1; ++z) e -= z * p.ks + 1;
    ti = e;
    return;
  }
  e -= p.full;
  int r;
  const int head = (p.rb - 1) * p.live;
  if (e < head) {
    r = 1 + e / p.live;
    z = e % p.live;
  } else {
    e -= head;
    r = p.rb + e / (p.live - 1);
    z = e % (p.live - 1);
  }
  ti = z * p.ks + r;
}

// K step staged through LDS: 16 KiB per operand per stage at T = 128 for either type
constexpr size_t SK_WS_BYTES = (size_t)2 * 512 * TILE * TILE * sizeof(double);  // 2 partial tiles per resident workgroup

template <typename R> constexpr int ktile_of() { return 128 / (int)sizeof(R); }

// THE decision about a launch: everything launch_gemm settles before it launches.  gemm_route is the only place
// where a launch's fate is decided; launch_gemm computes it once and executes it, the callers that must know
// beforehand what a launch will do (fit.hip: will it carry the epilogue, how many norm entries does it leave) and the
// test hooks (api_dev.hip) read the same struct.
enum { GEMM_DATA_PARALLEL = 0, GEMM_XCD = 1, GEMM_STREAMK = 2 };
struct GemmRoute {
  int rc;                    // 0, or -3: the launch is refused (error says why; only tile is filled in then)
  const char* error;
  int sched;                 // GEMM_DATA_PARALLEL, GEMM_XCD (the table of gemm_sched.hip), or GEMM_STREAMK (gemm_streamk.hip)
                             // -- if its planner accepts: it declines a launch that has a tile with an empty k range
                             // (or too many k steps), which then runs as stay_data_parallel() says
  int sk_first;              // stream-K: tiles of the data-parallel head (0: every tile is cut along k); else -1
  int tile;                  // block tile 128 / 64 / 32; 0: an empty product, nothing is launched
  int tiles, tiles_n;        // tiles of one problem, tiles per tile row
  int stages;                // LDS stages of the main loop: 2, or the deep pipeline's 4 (64-tiles) / 8 (32-tiles)
  int edge;                  // predicated (ragged) instance
  int half;                  // half-occupancy launch
  int gx, gy, gz;            // grid of the data-parallel launch: the whole launch, or the head of a stream-K tail (no
                             // launch when sk_first == 0); XCD-aware table: gx is the table's length, known once
                             // launch_gemm_xcd has the plan (0 until then).  Pair launch: blockIdx.z = the member
  int epi;                   // fused epilogue the launch carries (= the one asked for: one it cannot carry is refused)
  int sumsq_entries;         // epi 2: entries of sumsq the launch writes per problem: one per tile on the data-parallel
                             // schedules, 33 per tile on stream-K (one per tile + one per fix-up band); the squared
                             // Frobenius norm is the sum over all of them either way
  int slabs;                 // k_slabs route: live slabs (0: not that route)
  // The stream-K planner declined.  sumsq_entries stays at 33 per tile although the data-parallel launch then writes
  // one per tile: as before this struct existed, a caller that sums the table must not send an epi-2 launch whose
  // planner declines (lower output with both operands upper triangular); fit.hip's are lower x lower, never declined.
  void stay_data_parallel() { sched = GEMM_DATA_PARALLEL; sk_first = -1; gx = tiles; }
};
template <typename R> GemmRoute gemm_route(const GemmArgsT<R>& a);
template <typename R> int gemm_pick_tile(const GemmArgsT<R>& a);   // block tile of the route, for callers that have not filled the batch in yet
template <typename R> int launch_gemm(const GemmArgsT<R>& a, const GemmRoute& r, hipStream_t s);   // r = gemm_route(a)
template <typename R> int launch_gemm(const GemmArgsT<R>& a, hipStream_t s) { return launch_gemm(a, gemm_route(a), s); }
// The executors of a route (launch_gemm calls them).  stream-K (gemm_streamk.hip): 0 issued, 1 the planner declined.
template <typename R> int launch_gemm_streamk(const GemmArgsT<R>& a, const GemmRoute& r, hipStream_t s);
template <typename R> int launch_gemm_xcd(const GemmArgsT<R>& a, GemmRoute r, hipStream_t s);          // gemm_sched.hip
template <typename R> int launch_gemm_plain(const GemmArgsT<R>& a, const GemmRoute& r, hipStream_t s);   // the route's grid and instance
// Two independent pointer-batched products as ONE launch (blockIdx.z picks the problem): small-tile products of the
// latency-bound levels of the recursion that depend on the same predecessor but differ in structure (lower output or
// not, operand layout, alpha / beta), so they cannot share a pointer batch.  They can share a launch (rc 0) when both
// are plain pointer batches on full tiles of the same small size (32 or 64) with a row-major op(A); the launch then
// runs exactly the tile bodies the two separate launches would have run (same bits).  The route of the shared launch:
// rc, tile, stages, the grid, tiles = the tiles of both members.
template <typename R> GemmRoute gemm_pair_shape(const GemmArgsT<R>& a, const GemmArgsT<R>& b);
template <typename R> int launch_gemm_pair(const GemmArgsT<R>& a, const GemmArgsT<R>& b, const GemmRoute& h, hipStream_t s);   // h = gemm_pair_shape(a, b)

// Arc-cosine Gram matrix from the k-major, zero-padded operands XCt[Kd][ld1], Xt[Kd][ld2]:
//   G = XCt^T Xt + s0^2 ; c = clip(G/(q1 q2 + 1e-7)) ; K = q1 q2 J(c)
// np1/np2: padded extents (multiples of 128) that the loads may touch; nv1/nv2: valid
// extents that are stored.  `lower`: only tiles on/below the diagonal (square case).
// `pad_identity`: rows/cols >= nv get the identity (Kout must then hold np1 x np2).
template <typename R>
struct GramArgsT {
  const R* XCt;
  const R* Xt;
  const R* q1;   // [np1]
  const R* q2;   // [np2]
  R* Kout;       // [..][ldk]
  R* Cos;        // same shape as Kout, or nullptr
  int64_t ld1, ld2, ldk;
  int64_t ldcos;      // leading dimension of Cos (0: same as ldk)
  int np1, np2, nv1, nv2, Kd;
  double s0sq;
  int lower;
  int pad_identity;
  int mirror;    // lower only: every element below the diagonal is also stored transposed, so Kout holds the full
                 // symmetric matrix (for callers that multiply with it: no separate symmetrisation pass); Cos stays lower
};
using GramArgs = GramArgsT<double>;
template <typename R> int launch_gram(const GramArgsT<R>& a, hipStream_t s);

}  // namespace gpfit
