// Scoring a stimulus pool in one call (gpfit_score_pool; gpfit_score_pool_batch for up to 16 cells on one pool: the
// single call is the group of one, every kernel below carries a unit index): predictive moments of lambda, firing rate and
// active-learning utility of P candidate images from a posterior folded once per model into
//   w = K~_b^-1 m_b   and   S_b = K~_b^-1 (V_b - K~_b) K~_b^-1   (symmetric),
// so that per pool row (reference utils.py:1486-1498 with the products re-associated)
//   z = k* B ,  mu = z . w ,  sigma2 = k** + z S_b z^T.
// The quadratic form is ONE triangular product per row chunk: with S'[l][c] = 2 S[c][l] above the diagonal, S[c][c]
// on it and 0 below, z S_b z^T = sum_c z_c (z S')_c, and column tile j of Z S' sums k over [0, (j + 1) 128) only.
// Its epilogue multiplies the accumulators by Z, adds each row's 128 columns in a fixed order and writes one partial
// per (row, column tile); the partial of z . w rides along on the same Z elements.  No P x k result exists, nothing
// is allocated, nothing is added atomically.  Every sum of a row runs over the same terms in the same order wherever
// the row sits -- the dense products (C xtilde once, x* C and K* B per chunk) go out as pointer batches of one problem per
// unit, which the GEMM launcher never cuts along k -- so the bits do not depend on the chunking, the row offset, the run,
// or on which other units share the call.  Each unit works in its own context's matrices.
// gpfit_pool_covariance (below the pool call) forms the full posterior covariance of a shortlist's latents from the same
// stages: Sigma = K(x, x) + (Z S_b) Z^T on one triangle of tiles, mirrored, the diagonal from the pool call's own kernels.
#include "gemm_core.h"
#include "product.h"
#include "units.h"
#include "gpfit_mi355x.h"

#include <algorithm>

namespace gpfit {
namespace {

// ---- the Gram panel K*[np1][np2] of a row chunk against the inducing images, padding written as zeros; unit blockIdx.y
struct PoolGramArgs {
  PerUnit<const double*> XCt;   // [Kd][ld1]  (x* C)^T of the chunk
  PerUnit<const double*> Xt;    // [Kd][ld2]  inducing images, k-major
  PerUnit<const double*> q1;    // [np1]
  PerUnit<const double*> q2;    // [np2]
  PerUnit<double*> Kout;        // [np1][ldk]
  PerUnit<int> nv2;             // the unit's inducing images
  PerUnit<double> s0sq;
  int64_t ld1, ld2, ldk;
  int np1, np2, nv1, Kd;
  int lower;                    // the tiles on or below the block diagonal only (a chunk against itself)
};

__global__ __launch_bounds__(GEMM_THREADS, 2) void pool_gram_kernel(PoolGramArgs p, int tiles_n) {
  __shared__ __attribute__((aligned(16))) double smem[4 * Real<double>::KT * TILE];
  const int u = blockIdx.y;
  const int ti = blockIdx.x / tiles_n, tj = blockIdx.x % tiles_n;
  if (p.lower && tj > ti) return;   // the whole workgroup, before any barrier
  const int row0 = ti * TILE, col0 = tj * TILE;
  Real<double>::acc_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = acc_zero<double>();

  // operands are zero-padded to whole tiles: no edge predication on the loads
  gemm_mainloop<double, true, true, false, TILE>(p.XCt[u], p.ld1, p.Xt[u], p.ld2, p.np1, p.np2, row0, col0, 0, p.Kd, smem, acc);

  const int nv1 = p.nv1, nv2 = p.nv2[u];
  const int64_t ldk = p.ldk;
  const double s0sq = p.s0sq[u];
  const double pi32 = PI32;
  const double* __restrict__ q1 = p.q1[u];
  const double* __restrict__ q2 = p.q2[u];
  double* __restrict__ Ko = p.Kout[u];

  for_each_acc<double, TILE>(acc, row0, col0, [&](int row, int col, double g) {
    const int64_t o = (int64_t)row * ldk + col;
    if (row >= nv1 || col >= nv2) {
      Ko[o] = 0.0;   // the next step multiplies the whole panel: what the workspace held before must not survive
      return;
    }
    const double qq = q1[row] * q2[col];
    double c = (g + s0sq) / (qq + 1e-7);
    c = fmin(1.0, fmax(-1.0, c));
    const double delta = acos(c);
    const double J = (sqrt(1.0 - c * c) + pi32 * c - delta * c) / pi32;
    Ko[o] = qq * J;
  });
}

// ---- S' and w, zero-padded (once per call).  One 32 x 32 tile per workgroup (unit blockIdx.z), transposed through
// LDS: S is read along its rows (only elements on or below its diagonal are ever loaded) and S' written along its rows.
__global__ __launch_bounds__(256) void pool_weights_kernel(PerUnit<const double*> S_u, PerUnit<int64_t> lds_u, PerUnit<int> k_u,
                                                           int kp, PerUnit<double*> Sw_u, PerUnit<const double*> w_u,
                                                           PerUnit<double*> wpad_u) {
  __shared__ double tile[32][33];
  const int u = blockIdx.z;
  const double* __restrict__ S = S_u[u];
  const double* __restrict__ w = w_u[u];
  double* __restrict__ Sw = Sw_u[u];
  double* __restrict__ wpad = wpad_u[u];
  const int64_t lds = lds_u[u];
  const int k = k_u[u];
  const int c0 = blockIdx.x * 32, l0 = blockIdx.y * 32;
  const int tx = threadIdx.x, ty = threadIdx.y;   // 32 x 8
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = c0 + ty + 8 * r, l = l0 + tx;   // S[c][l], l <= c: the lower triangle is canonical, S[l][c] = S[c][l]
    tile[ty + 8 * r][tx] = (c < k && l <= c) ? S[(int64_t)c * lds + l] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int l = l0 + ty + 8 * r, c = c0 + tx;
    const double v = tile[tx][ty + 8 * r];
    Sw[(int64_t)l * kp + c] = l < c ? 2.0 * v : (l == c ? v : 0.0);
  }
  if (blockIdx.y == 0 && ty == 0) wpad[c0 + tx] = (w && c0 + tx < k) ? w[c0 + tx] : 0.0;   // no w: the covariance call
}

// ---- the quadratic form: tile (ti, tj) of Z S', reduced against Z along its columns
struct PoolQuadArgs {
  PerUnit<const double*> Z;     // [np1][ldz], zero padded
  PerUnit<const double*> Sw;    // [kp][kp]
  PerUnit<const double*> w;     // [kp]
  PerUnit<double*> part;        // [tiles_n][2][np1]: (row, tj) partials of z S z^T and of z . w
  int64_t ldz;
  int np1, kp, tiles_m, tiles_n, n_units;
};

__global__ __launch_bounds__(GEMM_THREADS, 2) void pool_quad_kernel(PoolQuadArgs p) {
  __shared__ __attribute__((aligned(16))) double smem[4 * Real<double>::KT * TILE];   // 8192 doubles
  // long tiles first (the k range grows with the column tile), those of all units before any shorter one; the tiles
  // of a unit's column share their S' panel
  const int per_col = p.tiles_m * p.n_units, in_col = (int)blockIdx.x % per_col;
  const int tj = p.tiles_n - 1 - (int)blockIdx.x / per_col, u = in_col / p.tiles_m, ti = in_col % p.tiles_m;
  const int row0 = ti * TILE, col0 = tj * TILE;
  Real<double>::acc_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = acc_zero<double>();

  const double* __restrict__ Z = p.Z[u];
  gemm_mainloop<double, false, true, false, TILE>(Z, p.ldz, p.Sw[u], p.kp, p.np1, p.kp, row0, col0, 0, col0 + TILE, smem, acc);
  __syncthreads();   // every wave is done with the operand stages: the reduction reuses them

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, fr = lane & 15;
  const double* __restrict__ wp = p.w[u];
  double wv[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) wv[ni] = wp[col0 + wn * 64 + ni * 16 + fr];
  // smem as [2][128 rows][32 slots]: slot = 16 wn + fr holds the row's sum over the lane's four columns; the slot index
  // is XORed with the row so that neither the writes nor the row-wise reads below pile up on one bank
  const int slot = wn * 16 + fr;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lrow = wm * 64 + mi * 16 + Real<double>::crow(lane, r);
      const double* zr = Z + (int64_t)(row0 + lrow) * p.ldz + col0 + wn * 64 + fr;
      double tq = 0.0, tm = 0.0;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const double z = zr[ni * 16];
        tq += acc[mi][ni][r] * z;
        tm += z * wv[ni];
      }
      const int at = lrow * 32 + (slot ^ (lrow & 31));
      smem[at] = tq;
      smem[TILE * 32 + at] = tm;
    }
  __syncthreads();
  const int which = tid >> 7, row = tid & 127;
  const double* sr = smem + (which * TILE + row) * 32;
  double t = 0.0;
#pragma unroll
  for (int sl = 0; sl < 32; ++sl) t += sr[sl ^ (row & 31)];
  p.part[u][((int64_t)tj * 2 + which) * p.np1 + row0 + row] = t;
}

// ---- per row: the partials in ascending column-tile order, then the moments, the rate and the utility's arguments
struct PoolFinishArgs {
  PerUnit<const double*> part, Kvec;
  PerUnit<double> A, A2, lambda0;
  PerUnit<double*> mu, sigma2, rate;         // the unit's outputs at the chunk's first row; rate may be nullptr
  PerUnit<double*> s2_scaled, mu_scaled;     // nullptr without response counts
  int np1, tiles_n, rows;
};

__global__ __launch_bounds__(256) void pool_finish_kernel(PoolFinishArgs p) {
  const int i = blockIdx.x * 256 + threadIdx.x, u = blockIdx.y;
  if (i >= p.rows) return;
  const double* __restrict__ part = p.part[u];
  const int np1 = p.np1;
  const double A = p.A[u], A2 = p.A2[u], lambda0 = p.lambda0[u];
  double* __restrict__ rate = p.rate[u];
  double* __restrict__ s2_scaled = p.s2_scaled[u];
  double qf = 0.0, m = 0.0;
  for (int j = 0; j < p.tiles_n; ++j) {
    qf += part[((int64_t)j * 2) * np1 + i];
    m += part[((int64_t)j * 2 + 1) * np1 + i];
  }
  const double s2 = p.Kvec[u][i] + qf;
  p.mu[u][i] = m;
  p.sigma2[u][i] = s2;
  if (rate) rate[i] = exp(A * m + 0.5 * A * A * s2 + lambda0);   // utils.py:395
  if (s2_scaled) {
    // one rounding per operation (no fused multiply-add), as the element-wise host expressions A^2 sigma2 and
    // A mu + lambda0 round: the utility then has the bits of nd_utility on those expressions
#pragma clang fp contract(off)
    const double am = A * m;
    s2_scaled[i] = A2 * s2;
    p.mu_scaled[u][i] = am + lambda0;
  }
}

// ---- a dense product whose bits do not depend on how many rows the chunk has, nor on the units beside it.  The
// launcher's balanced schedules cut the k range of the tail tiles of a large launch (stream-K, gemm.hip:
// streamk_first_tile), and which rows sit in tail tiles depends on the tile count, hence on the chunk.  A pointer batch
// never takes such a schedule: one problem per unit, the product runs data-parallel, every tile over its whole k range
// in ascending order, whatever the tile size.
int product_whole_k(Lane lane, Dims d, const Operand<double>& a, const Operand<double>& b, const Output<double>& c) {
  return run_gemm(lane.s, batch_args(lane, d, 1.0, a, b, c));
}

// The call for 1 .. CHAIN_MAXU units; tables indexed by unit (pixels, B, rate: the table itself may be null).
int score_pool_impl(const char* name, gpfit_ctx* const* ctxs, int n_units, void* stream, const double* sigma0,
                    const double* const* xstar, const int64_t* ldxs, int64_t P, const int* const* pixels,
                    const int64_t* d_full, const double* const* xtilde, const int64_t* ldxt, const int64_t* nt, const int64_t* d,
                    const double* const* C, const int64_t* ldc, const double* const* B, const int64_t* ldb, const int64_t* k,
                    const double* const* S, const int64_t* lds, const double* const* w, const double* A, const double* lambda0,
                    const double* r, int nr, int64_t chunk_rows, double* const* mu, double* const* sigma2,
                    double* const* rate, double* const* U) {
  const Refuse refuse{name};
  if (n_units < 1 || n_units > CHAIN_MAXU) return refuse("1 .. " + std::to_string(CHAIN_MAXU) + " units per call");
  if (!ctxs || !sigma0 || !xstar || !ldxs || !d_full || !xtilde || !ldxt || !nt || !d || !C || !ldc || !k || !S || !lds || !w ||
      !A || !lambda0 || !mu || !sigma2 || P < 0 || (B && !ldb) || (r && (!U || nr <= 0)))
    return refuse("bad argument");
  auto basis = [&](int u) { return B ? B[u] : nullptr; };
  auto pix = [&](int u) { return pixels ? pixels[u] : nullptr; };
  for (int u = 0; u < n_units; ++u)
    if (!ctxs[u] || !xtilde[u] || !C[u] || !S[u] || !w[u] || nt[u] <= 0 || d[u] <= 0 || k[u] <= 0 || ldxt[u] < d[u] ||
        ldc[u] < d[u] || lds[u] < k[u] || (P > 0 && (!xstar[u] || !mu[u] || !sigma2[u])) ||
        (basis(u) ? ldb[u] < k[u] : k[u] != nt[u]) || (r && !U[u]) ||
        (pix(u) ? (d_full[u] < d[u] || ldxs[u] < d_full[u]) : ldxs[u] < d[u]))
      return refuse(unit_prefix(n_units, u) + "bad argument");
  if (chunk_rows < 0 || chunk_rows % TILE) return refuse("chunk_rows must be 0 or a multiple of 128");
  const int64_t dp64 = round_up(d[0], 32), ntp64 = round_up(nt[0], TILE), kp64 = round_up(k[0], TILE);
  int64_t cap = 0;
  for (int u = 0; u < n_units; ++u) {
    const std::string unit = unit_prefix(n_units, u);
    if (const char* why = unit_context_refusal(ctxs, u)) return refuse(unit + why);
    if (round_up(d[u], 32) > ctxs[u]->dp_cap || round_up(nt[u], TILE) > ctxs[u]->np_cap || round_up(k[u], TILE) > ctxs[u]->np_cap)
      return refuse(unit + "problem larger than the context capacity");
    if (round_up(d[u], 32) != dp64 || round_up(nt[u], TILE) != ntp64 || round_up(k[u], TILE) != kp64 || !basis(u) != !basis(0))
      return refuse(unit + "the units of one call share round_up(d, 32), round_up(nt, 128) and round_up(k, 128), and all "
                           "have a basis B or none has");
    cap = u == 0 ? ctxs[u]->np_cap : std::min<int64_t>(cap, ctxs[u]->np_cap);
  }
  DeviceGuard device_guard(ctxs[0]->device);
  if (P == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const Lane lane{s, nullptr};   // the process-wide stream-K workspace, as the other kernel entry points
  const int dp = (int)dp64, ntp = (int)ntp64, kp = (int)kp64, nu = n_units;
  const bool with_B = basis(0) != nullptr;
  const int64_t chunk = chunk_rows ? std::min<int64_t>(chunk_rows, cap) : cap;
  const Units all = Units::all(ctxs, nu);
  const PerUnit<double> s0sq = all.table<double>([&](int u) { return sigma0[u] * sigma0[u]; });
  const PerUnit<int> d_u = all.table<int>([&](int u) { return (int)d[u]; }), nt_u = all.table<int>([&](int u) { return (int)nt[u]; }),
                     k_u = all.table<int>([&](int u) { return (int)k[u]; });
  const PerUnit<const int*> no_pix = all.same<const int*>(nullptr);
  // work matrices (np_cap^2 doubles each): none of them caches the factor of V, so lv_valid / lv32_valid stand
  const auto panel = &gpfit_ctx::Cos;    // K* of a chunk [np1][ntp]
  const auto Zb = &gpfit_ctx::Zbuf;      // K* B of a chunk [np1][kp]
  const auto Sw = &gpfit_ctx::Wbuf;      // S' [kp][kp]
  const auto Bpad = &gpfit_ctx::Tbuf;    // B zero padded [ntp][kp]
  const auto part = &gpfit_ctx::Abuf;    // [kp / 128][2][np1]
  const auto wpad = &gpfit_ctx::bv;

  // once per call: the inducing side of the kernel, S' and w
  GP_TRY(launch_pad_copy_group(nu, all.from(C), all.from(ldc), d_u, d_u, all.of(&gpfit_ctx::Cmat), dp, dp, dp, s));
  GP_TRY(launch_gather_group(nu, all.from(xtilde), all.from(ldxt), nt_u, no_pix, d_u, dp, ntp, all.of(&gpfit_ctx::Xt2), ntp, s));
  GP_TRY(product_whole_k(lane, {dp, ntp, dp}, trans(all.mats(&gpfit_ctx::Cmat, dp)), plain(all.mats(&gpfit_ctx::Xt2, ntp)),
                         into(all.mats(&gpfit_ctx::XCt2, ntp))));
  GP_TRY(launch_qvec_group(nu, all.cof(&gpfit_ctx::Xt2), all.cof(&gpfit_ctx::XCt2), ntp, dp, nt_u, ntp, s0sq,
                           all.of(&gpfit_ctx::hvec), all.of(&gpfit_ctx::q2), s));
  hipLaunchKernelGGL(pool_weights_kernel, dim3(kp / 32, kp / 32, nu), dim3(32, 8), 0, s, all.from(S), all.from(lds), k_u, kp,
                     all.of(Sw), all.from(w), all.of(wpad));
  GP_HIP(hipGetLastError());
  if (with_B) GP_TRY(launch_pad_copy_group(nu, all.from(B), all.from(ldb), nt_u, k_u, all.of(Bpad), kp, ntp, kp, s));

  PoolFinishArgs f{};
  f.part = all.cof(part); f.Kvec = all.cof(&gpfit_ctx::Kvec); f.tiles_n = kp / TILE;
  f.A = all.from(A); f.A2 = all.table<double>([&](int u) { return A[u] * A[u]; }); f.lambda0 = all.from(lambda0);
  if (r) {
    f.s2_scaled = all.of(&gpfit_ctx::lam_var);
    f.mu_scaled = all.of(&gpfit_ctx::lam_m);
  }
  for (int64_t off = 0; off < P; off += chunk) {
    const int rows = (int)std::min<int64_t>(chunk, P - off);
    const int np1 = (int)round_up(rows, TILE);
    GP_TRY(launch_gather_group(nu, all.table<const double*>([&](int u) { return xstar[u] + off * ldxs[u]; }), all.from(ldxs),
                               all.same(rows), all.table<const int*>(pix), d_u, dp, np1, all.of(&gpfit_ctx::Xt), np1, s));
    GP_TRY(product_whole_k(lane, {dp, np1, dp}, trans(all.mats(&gpfit_ctx::Cmat, dp)), plain(all.mats(&gpfit_ctx::Xt, np1)),
                           into(all.mats(&gpfit_ctx::XCt, np1))));
    GP_TRY(launch_qvec_group(nu, all.cof(&gpfit_ctx::Xt), all.cof(&gpfit_ctx::XCt), np1, dp, all.same(rows), np1, s0sq,
                             all.of(&gpfit_ctx::Kvec), all.of(&gpfit_ctx::q), s));
    {
      PoolGramArgs g{};
      g.XCt = all.cof(&gpfit_ctx::XCt); g.Xt = all.cof(&gpfit_ctx::Xt2); g.q1 = all.cof(&gpfit_ctx::q);
      g.q2 = all.cof(&gpfit_ctx::q2); g.Kout = all.of(panel); g.nv2 = nt_u; g.s0sq = s0sq;
      g.ld1 = np1; g.ld2 = ntp; g.ldk = ntp; g.np1 = np1; g.np2 = ntp; g.nv1 = rows; g.Kd = dp;
      hipLaunchKernelGGL(pool_gram_kernel, dim3((np1 / TILE) * (ntp / TILE), nu), dim3(GEMM_THREADS), 0, s, g, ntp / TILE);
      GP_HIP(hipGetLastError());
    }
    if (with_B)
      GP_TRY(product_whole_k(lane, {np1, kp, ntp}, plain(all.mats(panel, ntp)), plain(all.mats(Bpad, kp)), into(all.mats(Zb, kp))));
    {
      PoolQuadArgs q{};
      q.Z = all.cof(with_B ? Zb : panel); q.Sw = all.cof(Sw); q.w = all.cof(wpad); q.part = all.of(part);
      q.ldz = with_B ? kp : ntp;
      q.np1 = np1; q.kp = kp; q.tiles_m = np1 / TILE; q.tiles_n = kp / TILE; q.n_units = nu;
      hipLaunchKernelGGL(pool_quad_kernel, dim3(q.tiles_m * q.tiles_n * nu), dim3(GEMM_THREADS), 0, s, q);
      GP_HIP(hipGetLastError());
    }
    f.np1 = np1; f.rows = rows;
    f.mu = all.table<double*>([&](int u) { return mu[u] + off; });
    f.sigma2 = all.table<double*>([&](int u) { return sigma2[u] + off; });
    f.rate = all.table<double*>([&](int u) { return rate && rate[u] ? rate[u] + off : nullptr; });
    hipLaunchKernelGGL(pool_finish_kernel, dim3((rows + 255) / 256, nu), dim3(256), 0, s, f);
    GP_HIP(hipGetLastError());
    if (r)
      GP_TRY(launch_nd_utility_group(nu, all.cof(&gpfit_ctx::lam_var), all.cof(&gpfit_ctx::lam_m), rows, r, nr,
                                     all.table<double*>([&](int u) { return U[u] + off; }), s));
  }
  return 0;
}

// ---- the posterior covariance of a shortlist (gpfit_pool_covariance): the stages above on ONE chunk that holds every
// row, then  Sigma = K(x, x) + (Z S) Z^T  on the tiles on or below the block diagonal, mirrored on the way out.

// S as the full symmetric matrix, zero padded to [kp][kp]; only elements on or below S's diagonal are read
__global__ __launch_bounds__(256) void pool_symmetric_kernel(const double* __restrict__ S, int64_t lds, int k, int kp,
                                                             double* __restrict__ Sf) {
  const int c = blockIdx.x * 32 + (threadIdx.x & 31), l = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (l >= kp || c >= kp) return;
  const int hi = l > c ? l : c, lo = l > c ? c : l;
  Sf[(int64_t)l * kp + c] = hi < k ? S[(int64_t)hi * lds + lo] : 0.0;
}

// Sigma[i][j] = G[max(i, j)][min(i, j)] off the diagonal (both halves from ONE computed element: the same bits), the
// pool call's sigma2 on it.  A 32 x 32 block per workgroup; blocks above the diagonal read G's block transposed through LDS.
__global__ __launch_bounds__(256) void pool_cov_store_kernel(const double* __restrict__ G, int64_t ldg,
                                                             const double* __restrict__ sigma2, int M,
                                                             double* __restrict__ Sigma, int64_t ldsig) {
  __shared__ double tile[32][33];
  const int bi = blockIdx.y, bj = blockIdx.x;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  const bool upper = bj > bi;
  const int g0r = (upper ? bj : bi) * 32, g0c = (upper ? bi : bj) * 32;   // the block of G at or below the diagonal
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int gr = g0r + ty + 8 * r, gc = g0c + tx;
    // inside a diagonal block the element above the diagonal comes from its mirror image
    double v = 0.0;
    if (gr < M && gc < M) v = gc <= gr ? G[(int64_t)gr * ldg + gc] : G[(int64_t)gc * ldg + gr];
    tile[ty + 8 * r][tx] = v;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = bi * 32 + ty + 8 * r, j = bj * 32 + tx;
    if (i >= M || j >= M) continue;
    const double v = upper ? tile[tx][ty + 8 * r] : tile[ty + 8 * r][tx];
    Sigma[(int64_t)i * ldsig + j] = i == j ? sigma2[i] : v;
  }
}

int pool_covariance_impl(gpfit_ctx* ctx, void* stream, double sigma0, const double* xstar, int64_t ldxs, int64_t M,
                         const int* pixels, int64_t d_full, const double* xtilde, int64_t ldxt, int64_t nt, int64_t d,
                         const double* C, int64_t ldc, const double* B, int64_t ldb, int64_t k, const double* S, int64_t lds,
                         double* Sigma, int64_t ldsig) {
  const Refuse refuse{"gpfit_pool_covariance"};
  if (!ctx || !xtilde || !C || !S || M < 0 || nt <= 0 || d <= 0 || k <= 0 || ldxt < d || ldc < d || lds < k ||
      (M > 0 && (!xstar || !Sigma || ldsig < M)) || (B ? ldb < k : k != nt) ||
      (pixels ? (d_full < d || ldxs < d_full) : ldxs < d))
    return refuse("bad argument");
  if (ctx->pend.active) return refuse(GP_PENDING_REFUSAL);
  if (round_up(d, 32) > ctx->dp_cap || round_up(nt, TILE) > ctx->np_cap || round_up(k, TILE) > ctx->np_cap ||
      round_up(M, TILE) > ctx->np_cap)
    return refuse("problem larger than the context capacity");
  DeviceGuard device_guard(ctx->device);
  if (M == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const Lane lane{s, nullptr};
  const int dp = (int)round_up(d, 32), ntp = (int)round_up(nt, TILE), kp = (int)round_up(k, TILE);
  const int rows = (int)M, np1 = (int)round_up(M, TILE);
  const bool with_B = B != nullptr;
  gpfit_ctx* const ctxs[1] = {ctx};
  const Units one = Units::all(ctxs, 1);
  const PerUnit<double> s0sq = one.same(sigma0 * sigma0);
  const PerUnit<int> d_u = one.same((int)d), nt_u = one.same((int)nt), k_u = one.same((int)k);
  const PerUnit<const int*> no_pix = one.same<const int*>(nullptr);
  // the pool call's work matrices in the pool call's roles, and three more: none caches the factor of V
  const auto panel = &gpfit_ctx::Cos;    // K* [np1][ntp]
  const auto Zb = &gpfit_ctx::Zbuf;      // K* B [np1][kp]
  const auto Sw = &gpfit_ctx::Wbuf;      // S' [kp][kp] (the diagonal's quadratic form)
  const auto Bpad = &gpfit_ctx::Tbuf;    // B zero padded [ntp][kp]
  const auto part = &gpfit_ctx::Abuf;    // [kp / 128][2][np1]
  const auto wpad = &gpfit_ctx::bv;      // zeros: no mean is asked for
  const auto Sf = &gpfit_ctx::Tmp;       // S, full and symmetric [kp][kp]
  const auto Wm = &gpfit_ctx::TmpV;      // W = Z S [np1][kp]
  const auto Gm = &gpfit_ctx::Kbuf;      // K(x, x) + W Z^T, the tiles on or below the block diagonal [np1][np1]

  // the inducing side, S' and B exactly as the pool call forms them
  GP_TRY(launch_pad_copy_group(1, one.same(C), one.same(ldc), d_u, d_u, one.of(&gpfit_ctx::Cmat), dp, dp, dp, s));
  GP_TRY(launch_gather_group(1, one.same(xtilde), one.same(ldxt), nt_u, no_pix, d_u, dp, ntp, one.of(&gpfit_ctx::Xt2), ntp, s));
  GP_TRY(product_whole_k(lane, {dp, ntp, dp}, trans(one.mats(&gpfit_ctx::Cmat, dp)), plain(one.mats(&gpfit_ctx::Xt2, ntp)),
                         into(one.mats(&gpfit_ctx::XCt2, ntp))));
  GP_TRY(launch_qvec_group(1, one.cof(&gpfit_ctx::Xt2), one.cof(&gpfit_ctx::XCt2), ntp, dp, nt_u, ntp, s0sq,
                           one.of(&gpfit_ctx::hvec), one.of(&gpfit_ctx::q2), s));
  hipLaunchKernelGGL(pool_weights_kernel, dim3(kp / 32, kp / 32, 1), dim3(32, 8), 0, s, one.same(S), one.same(lds), k_u, kp,
                     one.of(Sw), one.same<const double*>(nullptr), one.of(wpad));
  GP_HIP(hipGetLastError());
  hipLaunchKernelGGL(pool_symmetric_kernel, dim3(kp / 32, kp / 8), dim3(256), 0, s, S, lds, (int)k, kp, ctx->*Sf);
  GP_HIP(hipGetLastError());
  if (with_B) GP_TRY(launch_pad_copy_group(1, one.same(B), one.same(ldb), nt_u, k_u, one.of(Bpad), kp, ntp, kp, s));

  // the shortlist: one chunk
  GP_TRY(launch_gather_group(1, one.same(xstar), one.same(ldxs), one.same(rows), one.same(pixels), d_u, dp, np1,
                             one.of(&gpfit_ctx::Xt), np1, s));
  GP_TRY(product_whole_k(lane, {dp, np1, dp}, trans(one.mats(&gpfit_ctx::Cmat, dp)), plain(one.mats(&gpfit_ctx::Xt, np1)),
                         into(one.mats(&gpfit_ctx::XCt, np1))));
  GP_TRY(launch_qvec_group(1, one.cof(&gpfit_ctx::Xt), one.cof(&gpfit_ctx::XCt), np1, dp, one.same(rows), np1, s0sq,
                           one.of(&gpfit_ctx::Kvec), one.of(&gpfit_ctx::q), s));
  PoolGramArgs g{};
  g.XCt = one.cof(&gpfit_ctx::XCt); g.Xt = one.cof(&gpfit_ctx::Xt2); g.q1 = one.cof(&gpfit_ctx::q);
  g.q2 = one.cof(&gpfit_ctx::q2); g.Kout = one.of(panel); g.nv2 = nt_u; g.s0sq = s0sq;
  g.ld1 = np1; g.ld2 = ntp; g.ldk = ntp; g.np1 = np1; g.np2 = ntp; g.nv1 = rows; g.Kd = dp;
  hipLaunchKernelGGL(pool_gram_kernel, dim3((np1 / TILE) * (ntp / TILE), 1), dim3(GEMM_THREADS), 0, s, g, ntp / TILE);
  GP_HIP(hipGetLastError());
  // the chunk against itself: x_i C x_j for i >= j
  g.Xt = one.cof(&gpfit_ctx::Xt); g.q2 = one.cof(&gpfit_ctx::q); g.Kout = one.of(Gm); g.nv2 = one.same(rows);
  g.ld2 = np1; g.ldk = np1; g.np2 = np1; g.lower = 1;
  hipLaunchKernelGGL(pool_gram_kernel, dim3((np1 / TILE) * (np1 / TILE), 1), dim3(GEMM_THREADS), 0, s, g, np1 / TILE);
  GP_HIP(hipGetLastError());
  if (with_B)
    GP_TRY(product_whole_k(lane, {np1, kp, ntp}, plain(one.mats(panel, ntp)), plain(one.mats(Bpad, kp)), into(one.mats(Zb, kp))));
  const auto Zm = with_B ? Zb : panel;
  const int64_t ldz = with_B ? kp : ntp;

  // the diagonal: the pool call's quadratic form and finish, so that it holds the bits of its sigma2
  PoolQuadArgs q{};
  q.Z = one.cof(Zm); q.Sw = one.cof(Sw); q.w = one.cof(wpad); q.part = one.of(part);
  q.ldz = ldz; q.np1 = np1; q.kp = kp; q.tiles_m = np1 / TILE; q.tiles_n = kp / TILE; q.n_units = 1;
  hipLaunchKernelGGL(pool_quad_kernel, dim3(q.tiles_m * q.tiles_n), dim3(GEMM_THREADS), 0, s, q);
  GP_HIP(hipGetLastError());
  PoolFinishArgs f{};
  f.part = one.cof(part); f.Kvec = one.cof(&gpfit_ctx::Kvec); f.tiles_n = kp / TILE;
  f.A = one.same(0.0); f.A2 = one.same(0.0); f.lambda0 = one.same(0.0);
  f.mu = one.of(&gpfit_ctx::lam_m); f.sigma2 = one.of(&gpfit_ctx::lam_var);
  f.np1 = np1; f.rows = rows;
  hipLaunchKernelGGL(pool_finish_kernel, dim3((rows + 255) / 256, 1), dim3(256), 0, s, f);
  GP_HIP(hipGetLastError());

  // off the diagonal: W = Z S, then G += W Z^T on the tiles on or below the block diagonal
  GP_TRY(product_whole_k(lane, {np1, kp, kp}, plain(one.mats(Zm, ldz)), plain(one.mats(Sf, kp)), into(one.mats(Wm, kp))));
  GP_TRY(product_whole_k(lane, {np1, np1, kp}, plain(one.mats(Wm, kp)), trans(one.mats(Zm, ldz)),
                         into_lower(one.mats(Gm, np1), 1.0)));
  const int nb = (rows + 31) / 32;
  hipLaunchKernelGGL(pool_cov_store_kernel, dim3(nb, nb), dim3(256), 0, s, ctx->*Gm, (int64_t)np1, ctx->lam_var, rows, Sigma,
                     ldsig);
  GP_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace gpfit

using namespace gpfit;

extern "C" int gpfit_score_pool(gpfit_ctx* c, void* stream, double sigma0, const double* xstar, int64_t ldxs, int64_t P,
                                const int* pixels, int64_t d_full, const double* xtilde, int64_t ldxt, int64_t nt,
                                int64_t d, const double* C, int64_t ldc, const double* B, int64_t ldb, int64_t k,
                                const double* S, int64_t lds, const double* w, double A, double lambda0,
                                const double* r, int nr, int64_t chunk_rows, double* mu, double* sigma2, double* rate,
                                double* U) {
  return score_pool_impl("gpfit_score_pool", &c, 1, stream, &sigma0, &xstar, &ldxs, P, &pixels, &d_full, &xtilde, &ldxt, &nt, &d,
                         &C, &ldc, &B, &ldb, &k, &S, &lds, &w, &A, &lambda0, r, nr, chunk_rows, &mu, &sigma2, &rate, &U);
}

extern "C" int gpfit_pool_covariance(gpfit_ctx* ctx, void* stream, double sigma0, const double* xstar, int64_t ldxs, int64_t M,
                                     const int* pixels, int64_t d_full, const double* xtilde, int64_t ldxt, int64_t nt,
                                     int64_t d, const double* C, int64_t ldc, const double* B, int64_t ldb, int64_t k,
                                     const double* S, int64_t lds, double* Sigma, int64_t ldsig) {
  return pool_covariance_impl(ctx, stream, sigma0, xstar, ldxs, M, pixels, d_full, xtilde, ldxt, nt, d, C, ldc, B, ldb, k, S, lds,
                              Sigma, ldsig);
}

extern "C" int gpfit_score_pool_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* sigma0,
                                      const double* const* xstar, const int64_t* ldxs, int64_t P, const int* const* pixels,
                                      const int64_t* d_full, const double* const* xtilde, const int64_t* ldxt,
                                      const int64_t* nt, const int64_t* d, const double* const* C, const int64_t* ldc,
                                      const double* const* B, const int64_t* ldb, const int64_t* k, const double* const* S,
                                      const int64_t* lds, const double* const* w, const double* A, const double* lambda0,
                                      const double* r, int nr, int64_t chunk_rows, double* const* mu, double* const* sigma2,
                                      double* const* rate, double* const* U) {
  return score_pool_impl("gpfit_score_pool_batch", ctxs, n_units, stream, sigma0, xstar, ldxs, P, pixels, d_full, xtilde, ldxt,
                         nt, d, C, ldc, B, ldb, k, S, lds, w, A, lambda0, r, nr, chunk_rows, mu, sigma2, rate, U);
}
