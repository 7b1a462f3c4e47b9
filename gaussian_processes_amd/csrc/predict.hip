// Scoring a stimulus pool in one call (gpfit_score_pool): predictive moments of lambda, firing rate and
// active-learning utility of P candidate images from a posterior folded once per model into
//   w = K~_b^-1 m_b   and   S_b = K~_b^-1 (V_b - K~_b) K~_b^-1   (symmetric),
// so that per pool row (reference utils.py:1486-1498 with the products re-associated)
//   z = k* B ,  mu = z . w ,  sigma2 = k** + z S_b z^T.
// The quadratic form is ONE triangular product per row chunk: with S'[l][c] = 2 S[c][l] above the diagonal, S[c][c]
// on it and 0 below, z S_b z^T = sum_c z_c (z S')_c, and column tile j of Z S' sums k over [0, (j + 1) 128) only.
// Its epilogue multiplies the accumulators by Z, adds each row's 128 columns in a fixed order and writes one partial
// per (row, column tile); the partial of z . w rides along on the same Z elements.  No P x k result exists, nothing
// is allocated, nothing is added atomically.  Every sum of a row runs over the same terms in the same order wherever
// the row sits -- the two dense products of a chunk (x* C and K* B) go out as pointer batches of one, which the GEMM
// launcher never cuts along k -- so the bits do not depend on the chunking, the row offset or the run.
#include "gemm_core.h"
#include "product.h"
#include "gpfit_mi355x.h"

#include <algorithm>

namespace gpfit {
namespace {

// ---- the Gram panel K*[np1][np2] of a row chunk against the inducing images, padding written as zeros
struct PoolGramArgs {
  const double* XCt;   // [Kd][ld1]  (x* C)^T of the chunk
  const double* Xt;    // [Kd][ld2]  inducing images, k-major
  const double* q1;    // [np1]
  const double* q2;    // [np2]
  double* Kout;        // [np1][ldk]
  int64_t ld1, ld2, ldk;
  int np1, np2, nv1, nv2, Kd;
  double s0sq;
};

__global__ __launch_bounds__(GEMM_THREADS, 2) void pool_gram_kernel(PoolGramArgs p, int tiles_n) {
  __shared__ __attribute__((aligned(16))) double smem[4 * Real<double>::KT * TILE];
  const int ti = blockIdx.x / tiles_n, tj = blockIdx.x % tiles_n;
  const int row0 = ti * TILE, col0 = tj * TILE;
  Real<double>::acc_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = acc_zero<double>();

  // operands are zero-padded to whole tiles: no edge predication on the loads
  gemm_mainloop<double, true, true, false, TILE>(p.XCt, p.ld1, p.Xt, p.ld2, p.np1, p.np2, row0, col0, 0, p.Kd, smem, acc);

  const int nv1 = p.nv1, nv2 = p.nv2;
  const int64_t ldk = p.ldk;
  const double s0sq = p.s0sq;
  const double pi32 = PI32;
  const double* __restrict__ q1 = p.q1;
  const double* __restrict__ q2 = p.q2;
  double* __restrict__ Ko = p.Kout;

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

// ---- S' and w, zero-padded (once per call).  One 32 x 32 tile per workgroup, transposed through LDS: S is read
// along its rows (only elements on or below its diagonal are ever loaded) and S' written along its rows.
__global__ __launch_bounds__(256) void pool_weights_kernel(const double* __restrict__ S, int64_t lds, int k, int kp,
                                                           double* __restrict__ Sw, const double* __restrict__ w,
                                                           double* __restrict__ wpad) {
  __shared__ double tile[32][33];
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
  if (blockIdx.y == 0 && ty == 0) wpad[c0 + tx] = c0 + tx < k ? w[c0 + tx] : 0.0;
}

// ---- the quadratic form: tile (ti, tj) of Z S', reduced against Z along its columns
struct PoolQuadArgs {
  const double* Z;     // [np1][ldz], zero padded
  const double* Sw;    // [kp][kp]
  const double* w;     // [kp]
  double* part;        // [tiles_n][2][np1]: (row, tj) partials of z S z^T and of z . w
  int64_t ldz;
  int np1, kp, tiles_m, tiles_n;
};

__global__ __launch_bounds__(GEMM_THREADS, 2) void pool_quad_kernel(PoolQuadArgs p) {
  __shared__ __attribute__((aligned(16))) double smem[4 * Real<double>::KT * TILE];   // 8192 doubles
  // long tiles first (the k range grows with the column tile); the tiles of a column share their S' panel
  const int tj = p.tiles_n - 1 - (int)blockIdx.x / p.tiles_m, ti = (int)blockIdx.x % p.tiles_m;
  const int row0 = ti * TILE, col0 = tj * TILE;
  Real<double>::acc_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = acc_zero<double>();

  gemm_mainloop<double, false, true, false, TILE>(p.Z, p.ldz, p.Sw, p.kp, p.np1, p.kp, row0, col0, 0, col0 + TILE, smem, acc);
  __syncthreads();   // every wave is done with the operand stages: the reduction reuses them

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, fr = lane & 15;
  const double* __restrict__ Z = p.Z;
  double wv[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) wv[ni] = p.w[col0 + wn * 64 + ni * 16 + fr];
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
  p.part[((int64_t)tj * 2 + which) * p.np1 + row0 + row] = t;
}

// ---- per row: the partials in ascending column-tile order, then the moments, the rate and the utility's arguments
__global__ __launch_bounds__(256) void pool_finish_kernel(const double* __restrict__ part, int np1, int tiles_n,
                                                          const double* __restrict__ Kvec, int rows, double A, double A2,
                                                          double lambda0, double* __restrict__ mu,
                                                          double* __restrict__ sigma2, double* __restrict__ rate,
                                                          double* __restrict__ s2_scaled, double* __restrict__ mu_scaled) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  double qf = 0.0, m = 0.0;
  for (int j = 0; j < tiles_n; ++j) {
    qf += part[((int64_t)j * 2) * np1 + i];
    m += part[((int64_t)j * 2 + 1) * np1 + i];
  }
  const double s2 = Kvec[i] + qf;
  mu[i] = m;
  sigma2[i] = s2;
  if (rate) rate[i] = exp(A * m + 0.5 * A * A * s2 + lambda0);   // utils.py:395
  if (s2_scaled) {
    // one rounding per operation (no fused multiply-add), as the element-wise host expressions A^2 sigma2 and
    // A mu + lambda0 round: the utility then has the bits of nd_utility on those expressions
#pragma clang fp contract(off)
    const double am = A * m;
    s2_scaled[i] = A2 * s2;
    mu_scaled[i] = am + lambda0;
  }
}

// ---- a dense product whose bits do not depend on how many rows the chunk has.  The launcher's balanced schedules cut
// the k range of the tail tiles of a large launch (stream-K, gemm.hip: streamk_first_tile), and which rows sit in tail
// tiles depends on the tile count, hence on the chunk.  A pointer batch never takes such a schedule: as a batch of one
// the product runs data-parallel, every tile over its whole k range in ascending order, whatever the tile size.
int product_whole_k(Lane lane, Dims d, const Operand<double>& a, const Operand<double>& b, const Output<double>& c) {
  return run_gemm(lane.s, batch_args(lane, d, 1.0, a, b, c));
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
  if (!c || P < 0 || !xtilde || !C || !S || !w || nt <= 0 || d <= 0 || k <= 0 || ldxt < d || ldc < d || lds < k ||
      (P > 0 && (!xstar || !mu || !sigma2)) || (B ? ldb < k : k != nt) || (r && (!U || nr <= 0)) ||
      (pixels ? (d_full < d || ldxs < d_full) : ldxs < d)) {
    set_error("gpfit_score_pool: bad argument");
    return -3;
  }
  if (chunk_rows < 0 || chunk_rows % TILE) {
    set_error("gpfit_score_pool: chunk_rows must be 0 or a multiple of 128");
    return -3;
  }
  GP_CTX_ENTER(c, "gpfit_score_pool");
  hipStream_t s = (hipStream_t)stream;
  const Lane lane{s, nullptr};   // the process-wide stream-K workspace, as the other kernel entry points
  const int dp = (int)round_up(d, 32), ntp = (int)round_up(nt, TILE), kp = (int)round_up(k, TILE);
  if (dp > c->dp_cap || ntp > c->np_cap || kp > c->np_cap) {
    set_error("gpfit_score_pool: problem larger than the context capacity");
    return -3;
  }
  if (P == 0) return 0;
  const int64_t chunk = chunk_rows ? std::min<int64_t>(chunk_rows, c->np_cap) : c->np_cap;
  const double s0sq = sigma0 * sigma0;
  // work matrices (np_cap^2 doubles each): none of them caches the factor of V, so lv_valid / lv32_valid stand
  double* panel = c->Cos;    // K* of a chunk [np1][ntp]
  double* Zb = c->Zbuf;      // K* B of a chunk [np1][kp]
  double* Sw = c->Wbuf;      // S' [kp][kp]
  double* Bpad = c->Tbuf;    // B zero padded [ntp][kp]
  double* part = c->Abuf;    // [kp / 128][2][np1]
  double* wpad = c->bv;

  // once per call: the inducing side of the kernel, S' and w
  GP_TRY(launch_pad_copy(C, ldc, (int)d, (int)d, c->Cmat, dp, dp, dp, s));
  GP_TRY(launch_gather<double>(xtilde, ldxt, (int)nt, nullptr, (int)d, dp, ntp, c->Xt2, ntp, nullptr, 0, s));
  GP_TRY(product(lane, {dp, ntp, dp}, 1.0, trans(mat(c->Cmat, dp)), plain(mat(c->Xt2, ntp)), into(mat(c->XCt2, ntp))));
  GP_TRY(launch_qvec(c->Xt2, c->XCt2, ntp, dp, (int)nt, ntp, s0sq, c->hvec, c->q2, s));
  hipLaunchKernelGGL(pool_weights_kernel, dim3(kp / 32, kp / 32), dim3(32, 8), 0, s, S, lds, (int)k, kp, Sw, w, wpad);
  GP_HIP(hipGetLastError());
  if (B) GP_TRY(launch_pad_copy(B, ldb, (int)nt, (int)k, Bpad, kp, ntp, kp, s));

  for (int64_t off = 0; off < P; off += chunk) {
    const int rows = (int)std::min<int64_t>(chunk, P - off);
    const int np1 = (int)round_up(rows, TILE);
    const double* xs = xstar + off * ldxs;
    GP_TRY(launch_gather<double>(xs, ldxs, rows, pixels, (int)d, dp, np1, c->Xt, np1, nullptr, 0, s));
    GP_TRY(product_whole_k(lane, {dp, np1, dp}, trans(mat(c->Cmat, dp)), plain(mat(c->Xt, np1)), into(mat(c->XCt, np1))));
    GP_TRY(launch_qvec(c->Xt, c->XCt, np1, dp, rows, np1, s0sq, c->Kvec, c->q, s));
    {
      PoolGramArgs g{};
      g.XCt = c->XCt; g.Xt = c->Xt2; g.q1 = c->q; g.q2 = c->q2; g.Kout = panel;
      g.ld1 = np1; g.ld2 = ntp; g.ldk = ntp; g.np1 = np1; g.np2 = ntp; g.nv1 = rows; g.nv2 = (int)nt; g.Kd = dp;
      g.s0sq = s0sq;
      hipLaunchKernelGGL(pool_gram_kernel, dim3((np1 / TILE) * (ntp / TILE)), dim3(GEMM_THREADS), 0, s, g, ntp / TILE);
      GP_HIP(hipGetLastError());
    }
    const double* Z = panel;
    int64_t ldz = ntp;
    if (B) {
      GP_TRY(product_whole_k(lane, {np1, kp, ntp}, plain(mat(panel, ntp)), plain(mat(Bpad, kp)), into(mat(Zb, kp))));
      Z = Zb;
      ldz = kp;
    }
    {
      PoolQuadArgs q{};
      q.Z = Z; q.Sw = Sw; q.w = wpad; q.part = part; q.ldz = ldz;
      q.np1 = np1; q.kp = kp; q.tiles_m = np1 / TILE; q.tiles_n = kp / TILE;
      hipLaunchKernelGGL(pool_quad_kernel, dim3(q.tiles_m * q.tiles_n), dim3(GEMM_THREADS), 0, s, q);
      GP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(pool_finish_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, part, np1, kp / TILE, c->Kvec, rows,
                       A, A * A, lambda0, mu + off, sigma2 + off, rate ? rate + off : nullptr,
                       r ? c->lam_var : nullptr, r ? c->lam_m : nullptr);
    GP_HIP(hipGetLastError());
    if (r) GP_TRY(launch_nd_utility(c->lam_var, c->lam_m, rows, r, nr, U + off, s));
  }
  return 0;
}
