// Products with a skinny (<= 128 columns) side and a long reduction, in fixed slabs: the hot path of
// gpfit_potrf_append_block (api_solve.hip).
//
//   out(z)[m][c] = alpha * sum_{r in slab z} op(A)(m, r) B(r, c)          m < M, c < kc <= 128, r < K
//
// The library's GEMM is laid out badly for these: Y^T Y with Y n x 128 is ONE 128 x 128 output tile with K = n, i.e.
// one workgroup on a 256-CU part, and its operands must be padded to the K step.  Here the reduction is cut into
// slabs of SKINNY_SLAB rows ACROSS workgroups: workgroup (mt, z) forms the 64 x kc partial of row panel mt over slab z
// with the fp64 MFMA (v_mfma_f64_16x16x4_f64; fragment layout: gemm_core.h) and writes it to its own place; a second
// launch (launch_skinny_sum) adds the partials of a row in slab order.  No floating-point atomics: the cut is a
// function of the sizes alone and every sum has one fixed order, so the same inputs give the same bits on every run.
// A triangular op(A) skips the slabs that hold only its zero half (skinny_slab_live, the one rule both launches
// enumerate by) and masks the other half inside the live ones, so what lies beyond the diagonal is never used.
// Operands are addressed by a stride pair each, any alignment, every access predicated: ragged n and k need no padding.
//
// Workgroup: 256 threads = 4 waves; wave w owns rows 16 w .. 16 w + 15 of the panel in up to eight 16 x 16
// accumulators (only ceil(kc / 16) of them are touched).  K step 16: one 16 x 64 image of op(A) and one 16 x 128 of B in
// LDS (28 KiB; row strides 80 / 144 doubles = 16 mod 32: the four k rows a fragment read touches fall on different
// halves of the 64 banks, conflict-free for ds_read_b64), the next step's elements fetched into registers before the
// products of the current one.  At k = 128 the two long products are bound by the fp64 MFMA rate, not by memory
// (n^2 k multiply-adds each over n^2 / 2 doubles read: 32 flops a byte): 4.3 GFLOP = 55 us of the matrix peak at
// n = 4096, measured 91 us.  A K step of 32 (56 KiB, 124 VGPRs, two waves a SIMD) was slower there (118 us) and no
// faster at n = 2048: the step stays at 16.
#include "gemm_core.h"
#include "kernels.h"

namespace gpfit {
namespace {

constexpr int SK_KS = 16;                 // K step
constexpr int SK_H = SK_KS / 16;          // 16-row halves of a step: the fetch pattern below covers 16 rows
constexpr int SK_LDA = SKINNY_MT + 16;    // LDS row strides (doubles)
constexpr int SK_LDB = SKINNY_LD + 16;

__global__ __launch_bounds__(256) void skinny_slab_kernel(SkinnyArgs a) {
  const int mt0 = blockIdx.x * SKINNY_MT, z = blockIdx.y;
  if (!skinny_slab_live(a.tri, z, mt0)) return;
  __shared__ double As[SK_KS * SK_LDA];
  __shared__ double Bs[SK_KS * SK_LDB];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, g = lane >> 4;
  const int nct = (a.kc + 15) >> 4;
  // the slab's rows, clipped to the triangle's extent for this panel
  int r_begin = z * SKINNY_SLAB, r_end = min((z + 1) * SKINNY_SLAB, a.K);
  if (a.tri == 1) r_end = min(r_end, mt0 + SKINNY_MT);
  if (a.tri == 2) r_begin = max(r_begin, mt0 & ~(SK_KS - 1));
  // who fetches what: along the contiguous index of each operand
  const bool a_mfast = a.sam == 1;
  const int am = a_mfast ? (tid & 15) * 4 : tid >> 2, ar = a_mfast ? tid >> 4 : (tid & 3) * 4;
  const bool b_cfast = a.sbc == 1;
  const int bc = b_cfast ? (tid & 15) * 8 : tid >> 1, br = b_cfast ? tid >> 4 : (tid & 1) * 8;
  double ra[SK_H][4], rb[SK_H][8];
  auto fetch = [&](int r0) {
#pragma unroll
    for (int h = 0; h < SK_H; ++h) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = mt0 + am + (a_mfast ? e : 0), r = r0 + 16 * h + ar + (a_mfast ? 0 : e);
        bool ok = m < a.M && r < r_end;
        if (a.tri == 1) ok = ok && r <= m;
        if (a.tri == 2) ok = ok && r >= m;
        ra[h][e] = ok ? a.A[(int64_t)m * a.sam + (int64_t)r * a.sar] : 0.0;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = bc + (b_cfast ? e : 0), r = r0 + 16 * h + br + (b_cfast ? 0 : e);
        rb[h][e] = (c < a.kc && r < r_end) ? a.B[(int64_t)r * a.sbr + (int64_t)c * a.sbc] : 0.0;
      }
    }
  };
  v4d acc[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) acc[t] = acc_zero<double>();
  if (r_begin < r_end) fetch(r_begin);
  for (int r0 = r_begin; r0 < r_end; r0 += SK_KS) {
#pragma unroll
    for (int h = 0; h < SK_H; ++h) {
#pragma unroll
      for (int e = 0; e < 4; ++e) As[(16 * h + ar + (a_mfast ? 0 : e)) * SK_LDA + am + (a_mfast ? e : 0)] = ra[h][e];
#pragma unroll
      for (int e = 0; e < 8; ++e) Bs[(16 * h + br + (b_cfast ? 0 : e)) * SK_LDB + bc + (b_cfast ? e : 0)] = rb[h][e];
    }
    __syncthreads();
    if (r0 + SK_KS < r_end) fetch(r0 + SK_KS);
#pragma unroll
    for (int kk = 0; kk < SK_KS / 4; ++kk) {
      const double fa = As[(4 * kk + g) * SK_LDA + 16 * w + fr];
#pragma unroll
      for (int t = 0; t < 8; ++t)
        if (t < nct) acc[t] = Real<double>::mfma(fa, Bs[(4 * kk + g) * SK_LDB + 16 * t + fr], acc[t]);
    }
    __syncthreads();
  }
  double* O = a.O + (int64_t)z * a.soz;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    if (t >= nct) continue;
    const int c = 16 * t + fr;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int m = mt0 + 16 * w + Real<double>::crow(lane, reg);
      if (m < a.M && c < a.kc) O[(int64_t)m * a.som + (int64_t)c * a.soc] = a.alpha * acc[t][reg];
    }
  }
}

// the partials of element (m, c) added in slab order (the live slabs of m's panel only), then what the caller makes of
// the sum; two rows of 128 columns per workgroup
__global__ __launch_bounds__(256) void skinny_sum_kernel(SkinnySumArgs a) {
  const int m = blockIdx.x * 2 + (threadIdx.x >> 7), c = threadIdx.x & 127;
  const int rows = a.mode == SKINNY_SUM_SCHUR ? SKINNY_LD : a.M;
  if (m >= rows) return;
  double v = 0.0;
  if (m < a.M && c < a.kc) {
    const int mt0 = (m / SKINNY_MT) * SKINNY_MT;
    for (int z = 0; z < a.nslab; ++z)
      if (skinny_slab_live(a.tri, z, mt0)) v += a.P[(int64_t)z * a.pz + (int64_t)m * SKINNY_LD + c];
  }
  if (a.mode == SKINNY_SUM_SCHUR) {
    // S = K22 - Y^T Y from K22's lower triangle, mirrored, in a 128 x 128 tile with a unit diagonal behind it
    const int hi = max(m, c), lo = min(m, c);
    a.dst[(int64_t)m * SKINNY_LD + c] =
        hi < a.kc ? a.Kc[(int64_t)(a.n + hi) * a.ldk + lo] - v : (m == c ? 1.0 : 0.0);
    return;
  }
  if (c >= a.kc) return;
  a.dst[(int64_t)m * SKINNY_LD + c] = v;
  if (a.mode == SKINNY_SUM_ROWS) {
    // Y = L^-1 K12: L21 = Y^T, and columns n .. n + k - 1 of the rows above are zero in both factors
    a.L[(int64_t)(a.n + c) * a.ldl + m] = v;
    a.L[(int64_t)m * a.ldl + a.n + c] = 0.0;
    a.Li[(int64_t)m * a.ldi + a.n + c] = 0.0;
  }
}

// the k x k diagonal blocks out of the leaf's 128-tiles (zero above the diagonal) and 2 sum log diag L22; one
// workgroup per row, the logarithms side by side and their sum by one thread in index order
__global__ __launch_bounds__(128) void append_block_finish_kernel(const double* __restrict__ Lt, const double* __restrict__ Lit,
                                                                   double* __restrict__ L, int64_t ldl, double* __restrict__ Li,
                                                                   int64_t ldi, int n, int k, double* __restrict__ logdet) {
  const int r = blockIdx.x, c = threadIdx.x;
  if (c < k) {
    L[(int64_t)(n + r) * ldl + n + c] = c <= r ? Lt[r * SKINNY_LD + c] : 0.0;
    Li[(int64_t)(n + r) * ldi + n + c] = c <= r ? Lit[r * SKINNY_LD + c] : 0.0;
  }
  if (r == 0) {
    __shared__ double lg[SKINNY_LD];
    if (c < k) lg[c] = log(Lt[c * SKINNY_LD + c]);
    __syncthreads();
    if (c == 0) {
      double s = 0.0;
      for (int j = 0; j < k; ++j) s += lg[j];
      logdet[0] = 2.0 * s;
    }
  }
}

}  // namespace

int launch_skinny_slabs(const SkinnyArgs& a, hipStream_t s) {
  if (a.M < 1 || a.K < 1 || a.kc < 1 || a.kc > SKINNY_LD || a.tri < 0 || a.tri > 2) {
    set_error("launch_skinny_slabs: bad shape (M, K >= 1, 1 .. 128 columns)");
    return -3;
  }
  hipLaunchKernelGGL(skinny_slab_kernel, dim3((a.M + SKINNY_MT - 1) / SKINNY_MT, skinny_slabs(a.K)), dim3(256), 0, s, a);
  GP_HIP(hipGetLastError());
  return 0;
}

int launch_skinny_sum(const SkinnySumArgs& a, hipStream_t s) {
  const int rows = a.mode == SKINNY_SUM_SCHUR ? SKINNY_LD : a.M;
  if (a.M < 1 || a.kc < 1 || a.kc > SKINNY_LD || a.nslab < 1) {
    set_error("launch_skinny_sum: bad shape");
    return -3;
  }
  hipLaunchKernelGGL(skinny_sum_kernel, dim3((rows + 1) / 2), dim3(256), 0, s, a);
  GP_HIP(hipGetLastError());
  return 0;
}

int launch_append_block_finish(const double* Lt, const double* Lit, double* L, int64_t ldl, double* Li, int64_t ldi, int n,
                               int k, double* logdet, hipStream_t s) {
  hipLaunchKernelGGL(append_block_finish_kernel, dim3(k), dim3(128), 0, s, Lt, Lit, L, ldl, Li, ldi, n, k, logdet);
  GP_HIP(hipGetLastError());
  return 0;
}

}  // namespace gpfit
