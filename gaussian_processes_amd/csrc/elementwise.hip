// Element-wise / reduction kernels of the GP fit path (everything that is not an MFMA GEMM
// or the Cholesky leaf).  All of them are HBM- or latency-bound and tiny next to the N^3
// work; they are written for coalesced access and deterministic (atomic-free) reductions.
#include "kernels.h"

#include <algorithm>

namespace gpfit {

// ------------------------------------------------------------------ helpers
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

// Sum over the whole block; result valid in every thread.  sh: >= 17 doubles.
__device__ __forceinline__ double block_sum(double v, double* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nw = (blockDim.x + 63) >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  if (wave == 0) {
    double t = (lane < nw) ? sh[lane] : 0.0;
    t = wave_sum(t);
    if (lane == 0) sh[16] = t;
  }
  __syncthreads();
  return sh[16];
}

// torch.linspace(-1, 1, n)[i] in fp64: two-sided fused form (matches ATen bit for bit;
// the pixel mesh of reference utils.py:876).
__device__ __forceinline__ double lin_pm1(int i, int n) {
  if (n <= 1) return -1.0;
  const double step = 2.0 / (double)(n - 1);
  return (i < n / 2) ? fma(step, (double)i, -1.0) : fma(-step, (double)(n - 1 - i), 1.0);
}

// ------------------------------------------------------------------ localker
template <typename R>
__global__ void localker_kernel(Theta th, const int* __restrict__ pix, int d, int dp, int n_rows, int n_cols,
                                R* __restrict__ C, int64_t ldc, R* __restrict__ dC) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= dp || j >= dp) return;
  if (i >= d || j >= d) {
    C[(int64_t)i * ldc + j] = (R)0;
    return;
  }
  const int pi = pix[i], pj = pix[j];
  const double xi = lin_pm1(pi % n_cols, n_cols), yi = lin_pm1(pi / n_cols, n_rows);
  const double xj = lin_pm1(pj % n_cols, n_cols), yj = lin_pm1(pj / n_cols, n_rows);
  const double dxi = xi - th.eps0x, dyi = yi - th.eps0y, dxj = xj - th.eps0x, dyj = yj - th.eps0y;
  const double lai = -th.eb * (dxi * dxi + dyi * dyi);  // utils.py:880
  const double laj = -th.eb * (dxj * dxj + dyj * dyj);
  const double ai = exp(lai), aj = exp(laj);            // :881
  const double ex = xj - xi, ey = yj - yi;
  const double ls = -th.er * (ex * ex + ey * ey);       // :890
  const double es = exp(ls);                            // :892
  const double cij = th.amp * ai * es * aj;             // :895
  const double cji = th.amp * aj * es * ai;
  const double c = (cij + cji) / 2.0;                   // :898
  C[(int64_t)i * ldc + j] = (R)c;
  if (dC) {
    const int64_t dd = (int64_t)d * d, o = (int64_t)i * d + j;
    dC[o] = (R)(c / th.amp);                                           // Amp        :902
    dC[dd + o] = (R)(c * (lai + laj));                                 // -2log2beta :907
    dC[2 * dd + o] = (R)(c * ls);                                      // -log2rho2  :909
    dC[3 * dd + o] = (R)(2.0 * th.eb * c * (xi + xj - 2.0 * th.eps0x));  // eps_0x   :904
    dC[4 * dd + o] = (R)(2.0 * th.eb * c * (yi + yj - 2.0 * th.eps0y));  // eps_0y   :905
  }
}

template <typename R>
int launch_localker(const Theta& th, const int* pix, int d, int dp, int n_rows, int n_cols, R* C, int64_t ldc,
                    R* dC, hipStream_t s) {
  dim3 block(32, 8), grid((dp + 31) / 32, (dp + 7) / 8);
  hipLaunchKernelGGL(localker_kernel<R>, grid, block, 0, s, th, pix, d, dp, n_rows, n_cols, C, ldc, dC);
  GP_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ gather / transpose
template <typename R>
__device__ __forceinline__ void gather_body(const R* __restrict__ X, int64_t ldx, int n, const int* __restrict__ pix, int d,
                                            R* __restrict__ Xt, int64_t ldt, R* __restrict__ Xm, int64_t ldm) {
  __shared__ R tile[32][33];
  const int k0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
  const int tx = threadIdx.x, ty = threadIdx.y;  // 32 x 8
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int nn = n0 + ty + 8 * r, k = k0 + tx;
    R v = 0;
    if (nn < n && k < d) v = X[(int64_t)nn * ldx + (pix ? pix[k] : k)];
    tile[ty + 8 * r][tx] = v;
    if (Xm) Xm[(int64_t)nn * ldm + k] = v;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = k0 + ty + 8 * r, nn = n0 + tx;
    Xt[(int64_t)k * ldt + nn] = tile[tx][ty + 8 * r];
  }
}
template <typename R>
__global__ void gather_kernel(const R* __restrict__ X, int64_t ldx, int n, const int* __restrict__ pix, int d,
                              R* __restrict__ Xt, int64_t ldt, R* __restrict__ Xm, int64_t ldm) {
  gather_body(X, ldx, n, pix, d, Xt, ldt, Xm, ldm);
}
// unit u = blockIdx.z of a group: its own images, pixel list and extents, the k-major copy only
__global__ void gather_group_kernel(PerUnit<const double*> X, PerUnit<int64_t> ldx, PerUnit<int> n, PerUnit<const int*> pix,
                                    PerUnit<int> d, PerUnit<double*> Xt, int64_t ldt) {
  const int u = blockIdx.z;
  gather_body<double>(X[u], ldx[u], n[u], pix[u], d[u], Xt[u], ldt, nullptr, 0);
}
int launch_gather_group(int n_units, PerUnit<const double*> X, PerUnit<int64_t> ldx, PerUnit<int> n, PerUnit<const int*> pix,
                        PerUnit<int> d, int dp, int np, PerUnit<double*> Xt, int64_t ldt, hipStream_t s) {
  if (dp % 32 || np % 32) {
    set_error("launch_gather: padded extents must be multiples of 32");
    return -3;
  }
  hipLaunchKernelGGL(gather_group_kernel, dim3(dp / 32, np / 32, n_units), dim3(32, 8), 0, s, X, ldx, n, pix, d, Xt, ldt);
  GP_HIP(hipGetLastError());
  return 0;
}

template <typename R>
int launch_gather(const R* X, int64_t ldx, int n, const int* pix, int d, int dp, int np, R* Xt, int64_t ldt, R* Xm,
                  int64_t ldm, hipStream_t s) {
  if (dp % 32 || np % 32) {
    set_error("launch_gather: padded extents must be multiples of 32");
    return -3;
  }
  hipLaunchKernelGGL(gather_kernel<R>, dim3(dp / 32, np / 32), dim3(32, 8), 0, s, X, ldx, n, pix, d, Xt, ldt, Xm,
                     ldm);
  GP_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ q / Kvec
// One block = 32 samples x 8 slices of the pixel range: a thread sums every eighth pixel of its sample (coalesced over
// the samples), the eight partial sums meet in LDS in a fixed order.  (One thread per sample walked all dp pixels
// with one load in flight: 37 us at N = 4096, 67 us at N = 8192 -- latency, not bandwidth.)
template <typename R>
__device__ __forceinline__ void qvec_body(const R* __restrict__ Xt, const R* __restrict__ XCt, int64_t ld, int dp, int n,
                                          int np, double s0sq, R* __restrict__ Kvec, R* __restrict__ q) {
  __shared__ double part[8][33];
  const int li = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + li;
  double h = 0.0;
  if (i < n) {
#pragma unroll 4
    for (int k = sl; k < dp; k += 8) h += (double)Xt[(int64_t)k * ld + i] * (double)XCt[(int64_t)k * ld + i];
  }
  part[sl][li] = h;
  __syncthreads();
  if (sl != 0 || i >= np) return;
  if (i >= n) {
    Kvec[i] = (R)1;
    q[i] = (R)1;
    return;
  }
  double t = part[0][li];
#pragma unroll
  for (int z = 1; z < 8; ++z) t += part[z][li];
  const double kv = t + s0sq;  // utils.py:1029
  Kvec[i] = (R)kv;
  q[i] = (R)sqrt(kv);          // utils.py:978
}
template <typename R>
__global__ __launch_bounds__(256) void qvec_kernel(const R* __restrict__ Xt, const R* __restrict__ XCt, int64_t ld, int dp,
                                                   int n, int np, double s0sq, R* __restrict__ Kvec, R* __restrict__ q) {
  qvec_body(Xt, XCt, ld, dp, n, np, s0sq, Kvec, q);
}
// unit u = blockIdx.y of a group: its own operands, sample count and sigma_0^2
__global__ __launch_bounds__(256) void qvec_group_kernel(PerUnit<const double*> Xt, PerUnit<const double*> XCt, int64_t ld,
                                                         int dp, PerUnit<int> n, int np, PerUnit<double> s0sq,
                                                         PerUnit<double*> Kvec, PerUnit<double*> q) {
  const int u = blockIdx.y;
  qvec_body<double>(Xt[u], XCt[u], ld, dp, n[u], np, s0sq[u], Kvec[u], q[u]);
}
int launch_qvec_group(int n_units, PerUnit<const double*> Xt, PerUnit<const double*> XCt, int64_t ld, int dp, PerUnit<int> n,
                      int np, PerUnit<double> s0sq, PerUnit<double*> Kvec, PerUnit<double*> q, hipStream_t s) {
  hipLaunchKernelGGL(qvec_group_kernel, dim3((np + 31) / 32, n_units), dim3(256), 0, s, Xt, XCt, ld, dp, n, np, s0sq, Kvec, q);
  GP_HIP(hipGetLastError());
  return 0;
}

template <typename R>
int launch_qvec(const R* Xt, const R* XCt, int64_t ld, int dp, int n, int np, double s0sq, R* Kvec, R* q,
                hipStream_t s) {
  hipLaunchKernelGGL(qvec_kernel<R>, dim3((np + 31) / 32), dim3(256), 0, s, Xt, XCt, ld, dp, n, np, s0sq, Kvec, q);
  GP_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ group housekeeping (kernels.h)
template <typename R>
__global__ __launch_bounds__(256) void group_prepare_kernel(GroupPrepT<R> g) {
  const int u = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < g.np) g.mpad[u][i] = (i < g.n) ? g.m[u][i] : (R)0;
  if (blockIdx.x == 0) {
    for (int k = threadIdx.x; k < g.d[u]; k += 256) g.pix[u][k] = g.pix_host[u][k];
    if (threadIdx.x < 4) g.info[u][threadIdx.x] = 0;
  }
}

template <typename R>
int launch_group_prepare(const GroupPrepT<R>& g, hipStream_t s) {
  hipLaunchKernelGGL(group_prepare_kernel<R>, dim3((g.np + 255) / 256, g.n_units), dim3(256), 0, s, g);
  GP_HIP(hipGetLastError());
  return 0;
}

__global__ void group_collect_kernel(GroupCollectT g) {
  const int u = blockIdx.x, t = threadIdx.x;
  if (t < 64) g.scal_host[u][t] = g.scal[u][t];
  else if (t < 68) g.info_host[u][t - 64] = g.info[u][t - 64];
  __threadfence_system();
}

int launch_group_collect(const GroupCollectT& g, hipStream_t s) {
  hipLaunchKernelGGL(group_collect_kernel, dim3(g.n_units), dim3(128), 0, s, g);
  GP_HIP(hipGetLastError());
  return 0;
}

// the same beginning for the sparse closures of a group (gpfit_fit_eval_sparse_batch): unit = blockIdx.y
__global__ __launch_bounds__(256) void closure_prepare_kernel(ClosurePrepT g) {
  const int u = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int nk = g.nk[u];
  if (i < g.nb) g.mpad[u][i] = (i < nk) ? g.m_b[u][i] : 0.0;
  if (i < g.cap[u]) { g.bv[u][i] = 0.0; g.wl[u][i] = 0.0; }
  if (blockIdx.x == 0) {
    const int d = g.d[u];
    const int* src = g.pix_host[u];
    int* dst = g.pix[u];
    for (int k = threadIdx.x; k < d; k += 256) dst[k] = src[k];
    if (threadIdx.x < 4) g.info[u][threadIdx.x] = 0;
  }
}
int launch_closure_prepare(const ClosurePrepT& g, hipStream_t s) {
  hipLaunchKernelGGL(closure_prepare_kernel, dim3((std::max(g.cap_max, g.nb) + 255) / 256, g.n_units), dim3(256), 0, s, g);
  GP_HIP(hipGetLastError());
  return 0;
}
// count zeros into each of three matrices per unit: blockIdx.y = which, blockIdx.z = unit
__global__ __launch_bounds__(256) void zero3_group_kernel(PerUnit<double*> a, PerUnit<double*> b, PerUnit<double*> c, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const int u = blockIdx.z;
  double* p = blockIdx.y == 0 ? a[u] : (blockIdx.y == 1 ? b[u] : c[u]);
  p[i] = 0.0;
}
int launch_zero3_group(int n_units, PerUnit<double*> a, PerUnit<double*> b, PerUnit<double*> c, int64_t count, hipStream_t s) {
  hipLaunchKernelGGL(zero3_group_kernel, dim3((unsigned)((count + 255) / 256), 3, n_units), dim3(256), 0, s, a, b, c, count);
  GP_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ pack / symmetrize
// (a tile is copied by eight blocks, sixteen rows each: with one block per tile a 640 x 640 matrix had 15 blocks on
// the chip and the copy took 21-33 us; 64 us at N = 4096)
template <typename R>
__device__ __forceinline__ void pack_lower_body(const R* __restrict__ src, int64_t lds, int n, R* __restrict__ dst, int64_t ldd,
                                                int bz) {
  const int tj = blockIdx.x, ti = blockIdx.y;
  if (tj > ti) return;
  const int r0 = ti * TILE + 16 * bz, c0 = tj * TILE;
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int e = threadIdx.x + 256 * it;
    const int i = r0 + (e >> 7), j = c0 + (e & 127);
    R v;
    if (i < n && j < n) v = src[(int64_t)i * lds + j];
    else v = (i == j) ? (R)1 : (R)0;
    dst[(int64_t)i * ldd + j] = v;
  }
}
template <typename R>
__global__ __launch_bounds__(256) void pack_lower_kernel(const R* __restrict__ src, int64_t lds, int n, R* __restrict__ dst,
                                                         int64_t ldd) {
  pack_lower_body(src, lds, n, dst, ldd, (int)blockIdx.z);
}
// the same for every unit of a group: blockIdx.z = unit * (TILE / 16) + the sixteen-row slice
__global__ __launch_bounds__(256) void pack_lower_group_kernel(PerUnit<const double*> src, PerUnit<int64_t> lds, PerUnit<int> n,
                                                               PerUnit<double*> dst, int64_t ldd) {
  const int u = blockIdx.z / (TILE / 16);
  pack_lower_body(src[u], lds[u], n[u], dst[u], ldd, (int)(blockIdx.z % (TILE / 16)));
}

template <typename R>
int launch_pack_lower(const R* src, int64_t lds, int n, R* dst, int64_t ldd, int np, hipStream_t s) {
  hipLaunchKernelGGL(pack_lower_kernel<R>, dim3(np / TILE, np / TILE, TILE / 16), dim3(256), 0, s, src, lds, n, dst, ldd);
  GP_HIP(hipGetLastError());
  return 0;
}
int launch_pack_lower_group(int n_units, PerUnit<const double*> src, PerUnit<int64_t> lds, PerUnit<int> n, PerUnit<double*> dst,
                            int64_t ldd, int np, hipStream_t s) {
  hipLaunchKernelGGL(pack_lower_group_kernel, dim3(np / TILE, np / TILE, n_units * (TILE / 16)), dim3(256), 0, s, src, lds, n,
                     dst, ldd);
  GP_HIP(hipGetLastError());
  return 0;
}

template <typename R>
__device__ __forceinline__ void symmetrize_body(R* __restrict__ A, int64_t lda, int n, R (*tile)[33]) {
  const int tj = blockIdx.x, ti = blockIdx.y;
  if (tj > ti) return;
  const int tx = threadIdx.x, ty = threadIdx.y;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ti * 32 + ty + 8 * r, j = tj * 32 + tx;
    tile[ty + 8 * r][tx] = (i < n && j < n) ? A[(int64_t)i * lda + j] : (R)0;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    // element (jj, ii) of the upper triangle <- (ii, jj) of the lower one
    const int jj = tj * 32 + ty + 8 * r, ii = ti * 32 + tx;
    if (ii < n && jj < n && ii > jj) A[(int64_t)jj * lda + ii] = tile[tx][ty + 8 * r];
  }
}
template <typename R>
__global__ void symmetrize_kernel(R* __restrict__ A, int64_t lda, int n) {
  __shared__ R tile[32][33];
  symmetrize_body(A, lda, n, tile);
}
__global__ void symmetrize_group_kernel(PerUnit<double*> A, int64_t lda, int n) {
  __shared__ double tile[32][33];
  symmetrize_body<double>(A[blockIdx.z], lda, n, tile);
}

template <typename R>
int launch_symmetrize(R* A, int64_t lda, int n, hipStream_t s) {
  const int t = (n + 31) / 32;
  hipLaunchKernelGGL(symmetrize_kernel<R>, dim3(t, t), dim3(32, 8), 0, s, A, lda, n);
  GP_HIP(hipGetLastError());
  return 0;
}
int launch_symmetrize_group(int n_units, PerUnit<double*> A, int64_t lda, int n, hipStream_t s) {
  const int t = (n + 31) / 32;
  hipLaunchKernelGGL(symmetrize_group_kernel, dim3(t, t, n_units), dim3(32, 8), 0, s, A, lda, n);
  GP_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ small reductions
template <typename R>
__device__ __forceinline__ void logdet_body(const R* __restrict__ L0, double* __restrict__ out0, const R* __restrict__ L1,
                                            double* __restrict__ out1, int64_t ldl, int n, double* sh) {
  const R* __restrict__ L = blockIdx.x == 0 ? L0 : L1;
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) v += log((double)L[(int64_t)i * ldl + i]);
  v = block_sum(v, sh);
  if (threadIdx.x == 0) (blockIdx.x == 0 ? out0 : out1)[0] = 2.0 * v;  // utils.py:1278
}
template <typename R>
__global__ void logdet_kernel(const R* __restrict__ L0, double* __restrict__ out0, const R* __restrict__ L1,
                              double* __restrict__ out1, int64_t ldl, int n) {
  __shared__ double sh[17];
  logdet_body(L0, out0, L1, out1, ldl, n, sh);
}
// two factors of every unit of a group: unit = blockIdx.y
__global__ void logdet_pair_group_kernel(PerUnit<const double*> L0, PerUnit<double*> out0, PerUnit<const double*> L1,
                                         PerUnit<double*> out1, int64_t ldl, PerUnit<int> n) {
  __shared__ double sh[17];
  const int u = blockIdx.y;
  logdet_body<double>(L0[u], out0[u], L1[u], out1[u], ldl, n[u], sh);
}
int launch_logdet_pair_group(int n_units, PerUnit<const double*> L0, PerUnit<double*> out0, PerUnit<const double*> L1,
                             PerUnit<double*> out1, int64_t ldl, PerUnit<int> n, hipStream_t s) {
  hipLaunchKernelGGL(logdet_pair_group_kernel, dim3(2, n_units), dim3(1024), 0, s, L0, out0, L1, out1, ldl, n);
  GP_HIP(hipGetLastError());
  return 0;
}

template <typename R>
int launch_logdet(const R* L, int64_t ldl, int n, double* out, hipStream_t s) {
  hipLaunchKernelGGL(logdet_kernel<R>, dim3(1), dim3(1024), 0, s, L, out, L, out, ldl, n);
  GP_HIP(hipGetLastError());
  return 0;
}

// two factors of the same size in one launch
template <typename R>
int launch_logdet_pair(const R* L0, double* out0, const R* L1, double* out1, int64_t ldl, int n, hipStream_t s) {
  hipLaunchKernelGGL(logdet_kernel<R>, dim3(2), dim3(1024), 0, s, L0, out0, L1, out1, ldl, n);
  GP_HIP(hipGetLastError());
  return 0;
}

template <typename R>
__global__ void sum_kernel(const R* __restrict__ x, int n, double scale, double* __restrict__ out) {
  __shared__ double sh[17];
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) v += (double)x[i];
  v = block_sum(v, sh);
  if (threadIdx.x == 0) out[0] = scale * v;
}

template <typename R>
__global__ void frob_tile_kernel(const R* __restrict__ T, int64_t ldt, double* __restrict__ partial) {
  __shared__ double sh[17];
  int ti, tj;
  {
    const int t = blockIdx.x;
    int i = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    while (i * (i + 1) / 2 > t) --i;
    ti = i;
    tj = t - i * (i + 1) / 2;
  }
  const R* base = T + (int64_t)ti * TILE * ldt + tj * TILE;
  double v = 0.0;
#pragma unroll 8
  for (int e = threadIdx.x; e < TILE * TILE; e += 256) {
    const double x = (double)base[(int64_t)(e >> 7) * ldt + (e & 127)];
    v += x * x;
  }
  v = block_sum(v, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

template <typename R>
int launch_frob_lower(const R* T, int64_t ldt, int np, double* out, double* partial, hipStream_t s) {
  const int t = np / TILE, nt = t * (t + 1) / 2;
  hipLaunchKernelGGL(frob_tile_kernel<R>, dim3(nt), dim3(256), 0, s, T, ldt, partial);
  hipLaunchKernelGGL(sum_kernel<double>, dim3(1), dim3(1024), 0, s, partial, nt, 1.0, out);
  GP_HIP(hipGetLastError());
  return 0;
}

// out = sum of the nt per-tile sums of squares a GEMM with the tile-norm epilogue left in partial
int launch_frob_finish(const double* partial, int nt, double* out, hipStream_t s) {
  hipLaunchKernelGGL(sum_kernel<double>, dim3(1), dim3(1024), 0, s, partial, nt, 1.0, out);
  GP_HIP(hipGetLastError());
  return 0;
}

template <typename R>
__device__ __forceinline__ void trmv_lower_body(const R* __restrict__ L, int64_t ldl, int np, const R* __restrict__ x,
                                                R* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (i >= np) return;
  const R* row = L + (int64_t)i * ldl;
  double v = 0.0;
#pragma unroll 8
  for (int j = lane; j <= i; j += 64) v += (double)row[j] * (double)x[j];
  v = wave_sum(v);
  if (lane == 0) y[i] = (R)v;
}
template <typename R>
__global__ void trmv_lower_kernel(const R* __restrict__ L, int64_t ldl, int np, const R* __restrict__ x,
                                  R* __restrict__ y) {
  trmv_lower_body(L, ldl, np, x, y);
}
__global__ void trmv_lower_group_kernel(PerUnit<double*> L, int64_t ldl, int np, PerUnit<double*> x, PerUnit<double*> y) {
  const int u = blockIdx.y;
  trmv_lower_body<double>(L[u], ldl, np, x[u], y[u]);
}

template <typename R>
int launch_trmv_lower(const R* L, int64_t ldl, int np, const R* x, R* y, hipStream_t s) {
  hipLaunchKernelGGL(trmv_lower_kernel<R>, dim3((np + 3) / 4), dim3(256), 0, s, L, ldl, np, x, y);
  GP_HIP(hipGetLastError());
  return 0;
}
int launch_trmv_lower_group(int n_units, PerUnit<double*> L, int64_t ldl, int np, PerUnit<double*> x, PerUnit<double*> y,
                            hipStream_t s) {
  hipLaunchKernelGGL(trmv_lower_group_kernel, dim3((np + 3) / 4, n_units), dim3(256), 0, s, L, ldl, np, x, y);
  GP_HIP(hipGetLastError());
  return 0;
}

// z_j = sum_{i >= j} L[i][j] x_i : block = 64 columns x one chunk of TRMV_ROWS rows
template <typename R>
__device__ __forceinline__ void trmv_lower_t_body(const R* __restrict__ L, int64_t ldl, int np, const R* __restrict__ x,
                                                  double* __restrict__ partial, double (*sh)[64]) {
  const int c = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + c;
  const int i0 = blockIdx.y * TRMV_ROWS, i1 = min(np, i0 + TRMV_ROWS);
  double v = 0.0;
  if (i1 > blockIdx.x * 64) {
#pragma unroll 8
    for (int i = i0 + rl; i < i1; i += 4)
      if (i >= j) v += (double)L[(int64_t)i * ldl + j] * (double)x[i];
  }
  sh[rl][c] = v;
  __syncthreads();
  if (rl == 0) partial[(int64_t)blockIdx.y * np + j] = sh[0][c] + sh[1][c] + sh[2][c] + sh[3][c];
}
template <typename R>
__global__ void trmv_lower_t_kernel(const R* __restrict__ L, int64_t ldl, int np, const R* __restrict__ x,
                                    double* __restrict__ partial) {
  __shared__ double sh[4][64];
  trmv_lower_t_body(L, ldl, np, x, partial, sh);
}
__global__ void trmv_lower_t_group_kernel(PerUnit<double*> L, int64_t ldl, int np, PerUnit<double*> x, PerUnit<double*> partial) {
  __shared__ double sh[4][64];
  const int u = blockIdx.z;
  trmv_lower_t_body<double>(L[u], ldl, np, x[u], partial[u], sh);
}

template <typename RI, typename RO>
__device__ __forceinline__ void reduce_slices_body(const RI* __restrict__ src, int64_t stride, int nslice, RO* __restrict__ dst,
                                                   int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  double v = 0.0;
  for (int z = 0; z < nslice; ++z) v += (double)src[(int64_t)z * stride + i];
  dst[i] = (RO)v;
}
template <typename RI, typename RO>
__global__ void reduce_slices_kernel(const RI* __restrict__ src, int64_t stride, int nslice, RO* __restrict__ dst,
                                     int64_t count) {
  reduce_slices_body(src, stride, nslice, dst, count);
}
__global__ void reduce_slices_group_kernel(PerUnit<double*> src, int64_t stride, int nslice, PerUnit<double*> dst, int64_t count) {
  const int u = blockIdx.y;
  reduce_slices_body<double, double>(src[u], stride, nslice, dst[u], count);
}
int launch_reduce_slices_group(int n_units, PerUnit<double*> src, int64_t slice_stride, int nslice, PerUnit<double*> dst,
                               int64_t count, hipStream_t s) {
  hipLaunchKernelGGL(reduce_slices_group_kernel, dim3((unsigned)((count + 255) / 256), n_units), dim3(256), 0, s, src,
                     slice_stride, nslice, dst, count);
  GP_HIP(hipGetLastError());
  return 0;
}

template <typename RI, typename RO>
int launch_reduce_slices(const RI* src, int64_t slice_stride, int nslice, RO* dst, int64_t count, hipStream_t s) {
  hipLaunchKernelGGL((reduce_slices_kernel<RI, RO>), dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, src,
                     slice_stride, nslice, dst, count);
  GP_HIP(hipGetLastError());
  return 0;
}

// dst[i][c] = sum of the live slabs z >= i / slab_rows of src[z][i][c], in slab order: the k slabs of a product with
// an upper triangular op(A) (GemmArgsT::k_slabs) -- the slabs below a row's own never were written
template <typename R>
__global__ void reduce_slabs_kernel(const R* __restrict__ src, int64_t stride, int nslab, int slab_rows,
                                    R* __restrict__ dst, int cols, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  double v = 0.0;
  for (int z = min(nslab - 1, (int)(i / cols) / slab_rows); z < nslab; ++z) v += (double)src[(int64_t)z * stride + i];
  dst[i] = (R)v;
}
template <typename R>
int launch_reduce_slabs(const R* src, int64_t slab_stride, int nslab, int slab_rows, R* dst, int rows, int cols, hipStream_t s) {
  const int64_t count = (int64_t)rows * cols;
  hipLaunchKernelGGL(reduce_slabs_kernel<R>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, src, slab_stride,
                     nslab, slab_rows, dst, cols, count);
  GP_HIP(hipGetLastError());
  return 0;
}

// dst = G + G^T with G = sum_z src[z] (n x n, in slice order): exactly symmetric, one pass
template <typename R>
__global__ void reduce_slices_sym_kernel(const R* __restrict__ src, int64_t stride, int nslice, R* __restrict__ dst, int n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n * n) return;
  const int r = (int)(i / n), c = (int)(i % n);
  const int64_t it = (int64_t)c * n + r;
  double v = 0.0, w = 0.0;
  for (int z = 0; z < nslice; ++z) {
    v += (double)src[(int64_t)z * stride + i];
    w += (double)src[(int64_t)z * stride + it];
  }
  dst[i] = (R)(v + w);
}
template <typename R>
int launch_reduce_slices_sym(const R* src, int64_t slice_stride, int nslice, R* dst, int n, hipStream_t s) {
  hipLaunchKernelGGL(reduce_slices_sym_kernel<R>, dim3((unsigned)(((int64_t)n * n + 255) / 256)), dim3(256), 0, s, src,
                     slice_stride, nslice, dst, n);
  GP_HIP(hipGetLastError());
  return 0;
}

template <typename R>
int launch_trmv_lower_t(const R* L, int64_t ldl, int np, const R* x, R* z, double* partial, hipStream_t s) {
  const int chunks = (np + TRMV_ROWS - 1) / TRMV_ROWS;
  hipLaunchKernelGGL(trmv_lower_t_kernel<R>, dim3(np / 64, chunks), dim3(256), 0, s, L, ldl, np, x, partial);
  GP_HIP(hipGetLastError());
  return launch_reduce_slices(partial, np, chunks, z, np, s);
}
int launch_trmv_lower_t_group(int n_units, PerUnit<double*> L, int64_t ldl, int np, PerUnit<double*> x, PerUnit<double*> z,
                              PerUnit<double*> partial, hipStream_t s) {
  const int chunks = (np + TRMV_ROWS - 1) / TRMV_ROWS;
  hipLaunchKernelGGL(trmv_lower_t_group_kernel, dim3(np / 64, chunks, n_units), dim3(256), 0, s, L, ldl, np, x, partial);
  GP_HIP(hipGetLastError());
  return launch_reduce_slices_group(n_units, partial, np, chunks, z, np, s);
}

// ---- block forms beside the two triangular products: the dense off-diagonal block of a factor applied to a vector
// (solve_mean in fit.hip substitutes with L21 instead of multiplying by [L^-1]21).  Same summation patterns as the
// trmv kernels: a wave per row, or 64 columns x one chunk of TRMV_ROWS rows with the chunks added in order.
// out_i = y_i - sum_j M[i][j] x_j   (M rows x cols, row-major)
template <typename R>
__global__ void gemv_sub_kernel(const R* __restrict__ M, int64_t ldm, int rows, int cols, const R* __restrict__ x,
                                const R* __restrict__ y, R* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (i >= rows) return;
  const R* row = M + (int64_t)i * ldm;
  double v = 0.0;
#pragma unroll 8
  for (int j = lane; j < cols; j += 64) v += (double)row[j] * (double)x[j];
  v = wave_sum(v);
  if (lane == 0) out[i] = (R)((double)y[i] - v);
}

template <typename R>
int launch_gemv_sub(const R* M, int64_t ldm, int rows, int cols, const R* x, const R* y, R* out, hipStream_t s) {
  if (rows <= 0) return 0;
  hipLaunchKernelGGL(gemv_sub_kernel<R>, dim3((rows + 3) / 4), dim3(256), 0, s, M, ldm, rows, cols, x, y, out);
  GP_HIP(hipGetLastError());
  return 0;
}

// partial[chunk][j] = sum over the chunk's rows of M[i][j] x_i   (cols a multiple of 64)
template <typename R>
__global__ void gemv_t_kernel(const R* __restrict__ M, int64_t ldm, int rows, int cols, const R* __restrict__ x,
                              double* __restrict__ partial) {
  __shared__ double sh[4][64];
  const int c = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + c;
  const int i0 = blockIdx.y * TRMV_ROWS, i1 = min(rows, i0 + TRMV_ROWS);
  double v = 0.0;
#pragma unroll 8
  for (int i = i0 + rl; i < i1; i += 4) v += (double)M[(int64_t)i * ldm + j] * (double)x[i];
  sh[rl][c] = v;
  __syncthreads();
  if (rl == 0) partial[(int64_t)blockIdx.y * cols + j] = sh[0][c] + sh[1][c] + sh[2][c] + sh[3][c];
}

// out_j = y_j - sum_z partial[z][j]
template <typename R>
__global__ void sub_slices_kernel(const double* __restrict__ partial, int cols, int nslice, const R* __restrict__ y,
                                  R* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cols) return;
  double v = 0.0;
  for (int z = 0; z < nslice; ++z) v += partial[(int64_t)z * cols + j];
  out[j] = (R)((double)y[j] - v);
}

// out = y - M^T x   (partial: ceil(rows / TRMV_ROWS) * cols doubles)
template <typename R>
int launch_gemv_t_sub(const R* M, int64_t ldm, int rows, int cols, const R* x, const R* y, R* out, double* partial,
                      hipStream_t s) {
  if (rows <= 0 || cols <= 0) return 0;
  if (cols % 64) {
    set_error("launch_gemv_t_sub: the column count must be a multiple of 64");
    return -3;
  }
  const int chunks = (rows + TRMV_ROWS - 1) / TRMV_ROWS;
  hipLaunchKernelGGL(gemv_t_kernel<R>, dim3(cols / 64, chunks), dim3(256), 0, s, M, ldm, rows, cols, x, partial);
  hipLaunchKernelGGL(sub_slices_kernel<R>, dim3((cols + 255) / 256), dim3(256), 0, s, partial, cols, chunks, y, out);
  GP_HIP(hipGetLastError());
  return 0;
}

// partial[t] = sum of squares of 128-tile t of a block of tm x tn tiles (row-major tile order); lower: the tiles
// on / below the block diagonal only, in the order of the GEMM's tile-norm epilogue (ti (ti + 1) / 2 + tj)
template <typename R>
__global__ void frob_block_kernel(const R* __restrict__ T, int64_t ldt, int tn, double* __restrict__ partial) {
  __shared__ double sh[17];
  const int ti = blockIdx.x / tn, tj = blockIdx.x % tn;
  const R* base = T + (int64_t)ti * TILE * ldt + tj * TILE;
  double v = 0.0;
#pragma unroll 8
  for (int e = threadIdx.x; e < TILE * TILE; e += 256) {
    const double x = (double)base[(int64_t)(e >> 7) * ldt + (e & 127)];
    v += x * x;
  }
  v = block_sum(v, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

template <typename R>
int launch_frob_tiles(const R* T, int64_t ldt, int rows, int cols, int lower, double* partial, hipStream_t s) {
  const int tm = rows / TILE, tn = cols / TILE;
  if (tm <= 0 || tn <= 0) return 0;
  if (lower) hipLaunchKernelGGL(frob_tile_kernel<R>, dim3(tm * (tm + 1) / 2), dim3(256), 0, s, T, ldt, partial);
  else hipLaunchKernelGGL(frob_block_kernel<R>, dim3(tm * tn), dim3(256), 0, s, T, ldt, tn, partial);
  GP_HIP(hipGetLastError());
  return 0;
}

// dst (fp32) <- src (fp64) over a rows x cols block
__global__ void demote_block_kernel(const double* __restrict__ src, int64_t lds, float* __restrict__ dst, int64_t ldd,
                                    int cols) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < cols) dst[(int64_t)blockIdx.y * ldd + c] = (float)src[(int64_t)blockIdx.y * lds + c];
}

int launch_demote_block(const double* src, int64_t lds, float* dst, int64_t ldd, int rows, int cols, hipStream_t s) {
  if (rows <= 0 || cols <= 0) return 0;
  hipLaunchKernelGGL(demote_block_kernel, dim3((cols + 255) / 256, rows), dim3(256), 0, s, src, lds, dst, ldd, cols);
  GP_HIP(hipGetLastError());
  return 0;
}

template <typename R>
__device__ __forceinline__ void dot_body(const R* __restrict__ x, const R* __restrict__ y, int n, double* __restrict__ out,
                                         double* sh) {
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) v += (double)x[i] * (double)y[i];
  v = block_sum(v, sh);
  if (threadIdx.x == 0) out[0] = v;
}
template <typename R>
__global__ void dot_kernel(const R* __restrict__ x, const R* __restrict__ y, int n, double* __restrict__ out) {
  __shared__ double sh[17];
  dot_body(x, y, n, out, sh);
}
__global__ void dot_group_kernel(PerUnit<double*> x, PerUnit<double*> y, int n, PerUnit<double*> out) {
  __shared__ double sh[17];
  const int u = blockIdx.y;
  dot_body<double>(x[u], y[u], n, out[u], sh);
}
int launch_dot_group(int n_units, PerUnit<double*> x, PerUnit<double*> y, int n, PerUnit<double*> out, hipStream_t s) {
  hipLaunchKernelGGL(dot_group_kernel, dim3(1, n_units), dim3(1024), 0, s, x, y, n, out);
  GP_HIP(hipGetLastError());
  return 0;
}

template <typename R>
int launch_dot(const R* x, const R* y, int n, double* out, hipStream_t s) {
  hipLaunchKernelGGL(dot_kernel<R>, dim3(1), dim3(1024), 0, s, x, y, n, out);
  GP_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ moments / rate / likelihood
// One thread per observation over n / 256 workgroups; the three sums go through per-workgroup partials that the last
// workgroup to finish (a ticket) adds up in workgroup order -- deterministic, and one launch.  (A single workgroup
// walking all n observations, two strided diagonal reads and an acos / exp each, took 25 us at N = 4096 and 51 us at
// N = 8192.)
template <typename R>
__global__ __launch_bounds__(256) void moments_kernel(const R* __restrict__ Kvec, const R* __restrict__ q,
                                                      const R* __restrict__ Cos, int64_t ldc, const R* __restrict__ V,
                                                      int64_t ldv, const R* __restrict__ m, const R* __restrict__ r, int n,
                                                      double A, double lambda0, R* __restrict__ lam_m,
                                                      R* __restrict__ lam_var, R* __restrict__ f, R* __restrict__ wl,
                                                      double* __restrict__ scal, double* __restrict__ part,
                                                      int* __restrict__ ticket) {
  __shared__ double sh[17];
  __shared__ bool last;
  double s_rm = 0.0, s_r = 0.0, s_f = 0.0;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const double c = (double)Cos[(int64_t)i * ldc + i];
    const double delta = acos(c);
    const double J = (sqrt(1.0 - c * c) + PI32 * c - delta * c) / PI32;
    const double qi = (double)q[i];
    const double kii = qi * qi * J;                         // K~_ii as the Gram kernel wrote it
    const double lv = (double)Kvec[i] - kii + (double)V[(int64_t)i * ldv + i];  // utils.py:1101, a = B, full rank
    const double lm = (double)m[i];                         // utils.py:1090
    const double fi = exp(A * lm + 0.5 * A * A * lv + lambda0);  // utils.py:1138
    const double g = 1.0 - J - (PI32 - delta) * (1.0 - c) / PI32;
    lam_m[i] = (R)lm;
    lam_var[i] = (R)lv;
    f[i] = (R)fi;
    wl[i] = (R)(-0.5 * A * A * fi * g);
    s_rm = (double)r[i] * lm;
    s_r = (double)r[i];
    s_f = fi;
  }
  s_rm = block_sum(s_rm, sh);
  s_r = block_sum(s_r, sh);
  s_f = block_sum(s_f, sh);
  if (threadIdx.x == 0) {
    part[blockIdx.x * 3 + 0] = s_rm;
    part[blockIdx.x * 3 + 1] = s_r;
    part[blockIdx.x * 3 + 2] = s_f;
    __threadfence();                                    // partials visible before the ticket
    last = (atomicAdd(ticket, 1) == (int)gridDim.x - 1);
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  if (threadIdx.x < 3) {
    double v = 0.0;
    for (int b = 0; b < (int)gridDim.x; ++b)
      v += __hip_atomic_load(&part[b * 3 + threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    scal[threadIdx.x] = v;
  }
  if (threadIdx.x == 0) *ticket = 0;
}

// part: >= 3 * ceil(n / 256) doubles of scratch; ticket: a device int that is 0 between calls
template <typename R>
int launch_moments(const R* Kvec, const R* q, const R* Cos, int64_t ldc, const R* V, int64_t ldv, const R* m,
                   const R* r, int n, double A, double lambda0, R* lam_m, R* lam_var, R* f, R* wl, double* scal,
                   double* part, int* ticket, hipStream_t s) {
  hipLaunchKernelGGL(moments_kernel<R>, dim3((n + 255) / 256), dim3(256), 0, s, Kvec, q, Cos, ldc, V, ldv, m, r, n, A,
                     lambda0, lam_m, lam_var, f, wl, scal, part, ticket);
  GP_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ adjoint pass (64 x 64 tiles)
// Aout receives Lambda = tril(A_w, -1) + 1/2 diag(A_w) (A_w = Lambda + Lambda^T): every lower tile once, the
// diagonal tiles with half the diagonal and zeros above it (the product that consumes Lambda reads whole diagonal
// tiles); the tiles above the diagonal are not touched.
template <typename R>
__global__ __launch_bounds__(256) void adjoint_kernel(const R* __restrict__ W, const R* __restrict__ Cos, int64_t ld,
                                                      const R* __restrict__ b, const R* __restrict__ q, int n,
                                                      int np, R* __restrict__ Aout, double* __restrict__ upart,
                                                      double* __restrict__ vpart, double* __restrict__ sumA_part) {
  __shared__ double colsum[4][64];
  __shared__ double sh[17];
  int ti, tj;
  {
    const int t = blockIdx.x;
    int i = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    while (i * (i + 1) / 2 > t) --i;
    ti = i;
    tj = t - i * (i + 1) / 2;
  }
  const bool diag = (ti == tj);
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // ty = wave
  const int j = tj * 64 + tx;
  const double qj = (double)q[j], bj = (double)b[j];
  double csum = 0.0, asum = 0.0;
  for (int rr = ty; rr < 64; rr += 4) {
    const int i = ti * 64 + rr;
    double aw = 0.0, bm = 0.0;
    if (i < n && j < n) {
      // canonical storage is the lower triangle: in a diagonal tile read (j,i) when i < j
      const int64_t o = (diag && i < j) ? ((int64_t)j * ld + i) : ((int64_t)i * ld + j);
      const double w = (double)W[o] - 0.5 * (double)b[i] * bj;
      const double c = (double)Cos[o];
      aw = w * (PI32 - acos(c)) / PI32;
      bm = w * sqrt(1.0 - c * c) / PI32;
    }
    Aout[(int64_t)i * ld + j] = (R)((diag && i <= j) ? (i == j ? 0.5 * aw : 0.0) : aw);
    asum += aw;
    // row sum over the 64 columns of this tile (one wave holds a whole row)
    const double rs = wave_sum(bm * qj);
    if (tx == 0) upart[(int64_t)tj * np + i] = rs;
    csum += bm * (double)q[i];
  }
  colsum[ty][tx] = csum;
  __syncthreads();
  if (!diag && ty == 0) vpart[(int64_t)ti * np + j] = colsum[0][tx] + colsum[1][tx] + colsum[2][tx] + colsum[3][tx];
  asum = block_sum(asum, sh);
  if (threadIdx.x == 0) sumA_part[blockIdx.x] = diag ? asum : 2.0 * asum;
}

// (block = 32 entries x 8 slices of the partial index, combined in a fixed order: the serial walk over N / 64
// partials took 21 us at N = 4096 and 48 us at N = 8192 on N / 256 workgroups)
template <typename R>
__global__ __launch_bounds__(256) void adjoint_u_kernel(const double* __restrict__ upart, const double* __restrict__ vpart,
                                                        int nt64, const R* __restrict__ q, const R* __restrict__ wl, int n,
                                                        int np, R* __restrict__ tvec, double* __restrict__ uq) {
  __shared__ double sl[8][33];
  const int li = threadIdx.x & 31, z = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + li;
  double u = 0.0;
  if (i < n) {
    const int T = i >> 6;
#pragma unroll 4
    for (int t = z; t < nt64; t += 8) u += (t <= T ? upart : vpart)[(int64_t)t * np + i];
  }
  sl[z][li] = u;
  __syncthreads();
  if (z != 0 || i >= np) return;
  if (i >= n) {
    tvec[i] = (R)0;
    uq[i] = 0.0;
    return;
  }
  u = sl[0][li];
#pragma unroll
  for (int k = 1; k < 8; ++k) u += sl[k][li];
  const double v = u / (double)q[i];
  uq[i] = v;
  tvec[i] = (R)(v - (double)wl[i]);
}

// the three sums behind the adjoint pass in one launch (block 0: uq, block 1: wl, block 2: the tile sums)
template <typename R>
__global__ void adjoint_sums_kernel(const double* __restrict__ uq, const R* __restrict__ wl, int n,
                                    const double* __restrict__ sumA_part, int ntile_tri, double* __restrict__ out) {
  __shared__ double sh[17];
  const int b = blockIdx.x;
  double v = 0.0;
  if (b == 0) for (int i = threadIdx.x; i < n; i += blockDim.x) v += uq[i];
  else if (b == 1) for (int i = threadIdx.x; i < n; i += blockDim.x) v += (double)wl[i];
  else for (int i = threadIdx.x; i < ntile_tri; i += blockDim.x) v += sumA_part[i];
  v = block_sum(v, sh);
  if (threadIdx.x == 0) out[b] = v;
}

// Rectangular adjoint (x1 != x2, utils.py:996-1021 contracted with W[n1][n2]): per 64 x 64 tile
//   Aout = W o (pi - delta)/pi ,  B_m = W o sqrt(1 - c^2)/pi ,
//   upart[tj][i] = sum_{j in tile} B_m[i][j] q2[j] ,  vpart[ti][j] = sum_{i in tile} B_m[i][j] q1[i] ,
//   tile_sum[ti][tj] = sum Aout.   Padding rows / columns of Aout are written as zero.
__global__ __launch_bounds__(256) void adjoint_rect_kernel(const double* __restrict__ W, int64_t ldw,
                                                           const double* __restrict__ Cos, int64_t ldc,
                                                           const double* __restrict__ q1,
                                                           const double* __restrict__ q2, int n1, int n2, int np1,
                                                           int np2, double* __restrict__ Aout, int64_t lda,
                                                           double* __restrict__ upart, double* __restrict__ vpart,
                                                           double* __restrict__ tile_sum) {
  __shared__ double colsum[4][64];
  __shared__ double sh[17];
  const int tj = blockIdx.x, ti = blockIdx.y;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int j = tj * 64 + tx;
  const double qj = (j < n2) ? q2[j] : 0.0;
  double csum = 0.0, asum = 0.0;
  for (int rr = ty; rr < 64; rr += 4) {
    const int i = ti * 64 + rr;
    double aw = 0.0, bm = 0.0;
    if (i < n1 && j < n2) {
      const double w = W[(int64_t)i * ldw + j];
      const double c = Cos[(int64_t)i * ldc + j];
      aw = w * (PI32 - acos(c)) / PI32;
      bm = w * sqrt(1.0 - c * c) / PI32;
    }
    Aout[(int64_t)i * lda + j] = aw;
    asum += aw;
    const double rs = wave_sum(bm * qj);
    if (tx == 0) upart[(int64_t)tj * np1 + i] = rs;
    csum += (i < n1) ? bm * q1[i] : 0.0;
  }
  colsum[ty][tx] = csum;
  __syncthreads();
  if (ty == 0) vpart[(int64_t)ti * np2 + j] = colsum[0][tx] + colsum[1][tx] + colsum[2][tx] + colsum[3][tx];
  asum = block_sum(asum, sh);
  if (threadIdx.x == 0) tile_sum[ti * gridDim.x + tj] = asum;
}

// u[i] = sum_t part[t][i];  tvec = u / (2 q) (+ extra);  uq = u / q   (zero on padding).
// Block = 32 entries x 8 slices of the partial index (fixed order): with one thread walking all nt = N / 64 partials
// the pass over n_t = 8192 tile rows took 44 us on 8 workgroups.
__global__ __launch_bounds__(256) void adjoint_rect_reduce_kernel(const double* __restrict__ part, int nt,
                                                                  const double* __restrict__ q,
                                                                  const double* __restrict__ extra, int n, int np,
                                                                  double* __restrict__ tvec, double* __restrict__ uq) {
  __shared__ double sl[8][33];
  const int li = threadIdx.x & 31, z = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + li;
  double u = 0.0;
  if (i < n) {
#pragma unroll 4
    for (int t = z; t < nt; t += 8) u += part[(int64_t)t * np + i];
  }
  sl[z][li] = u;
  __syncthreads();
  if (z != 0 || i >= np) return;
  if (i >= n) {
    tvec[i] = 0.0;
    uq[i] = 0.0;
    return;
  }
  u = sl[0][li];
#pragma unroll
  for (int k = 1; k < 8; ++k) u += sl[k][li];
  const double v = u / q[i];
  uq[i] = v;
  tvec[i] = 0.5 * v + (extra ? extra[i] : 0.0);
}

// up to four independent sums in one launch (block b: out[b] = scale[b] * sum of x[b][0 .. n[b]))
struct SumList {
  const double* x[4];
  int n[4];
  double scale[4];
  double* out[4];
};
__global__ void sum_list_kernel(SumList l) {
  __shared__ double sh[17];
  const int b = blockIdx.x;
  double v = 0.0;
  for (int i = threadIdx.x; i < l.n[b]; i += blockDim.x) v += l.x[b][i];
  v = block_sum(v, sh);
  if (threadIdx.x == 0) l.out[b][0] = l.scale[b] * v;
}

int launch_adjoint_rect(const double* W, int64_t ldw, const double* Cos, int64_t ldc, const double* q1,
                        const double* q2, int n1, int n2, int np1, int np2, double* Aout, int64_t lda, double* upart,
                        double* vpart, double* tile_sum, const double* extra1, double* t1, double* t2, double* uq1,
                        double* uq2, double* scal3, hipStream_t s) {
  const int g1 = np1 / 64, g2 = np2 / 64;
  hipLaunchKernelGGL(adjoint_rect_kernel, dim3(g2, g1), dim3(256), 0, s, W, ldw, Cos, ldc, q1, q2, n1, n2, np1, np2,
                     Aout, lda, upart, vpart, tile_sum);
  hipLaunchKernelGGL(adjoint_rect_reduce_kernel, dim3((np1 + 31) / 32), dim3(256), 0, s, upart, g2, q1, extra1, n1,
                     np1, t1, uq1);
  hipLaunchKernelGGL(adjoint_rect_reduce_kernel, dim3((np2 + 31) / 32), dim3(256), 0, s, vpart, g1, q2,
                     (const double*)nullptr, n2, np2, t2, uq2);
  SumList l{};
  l.x[0] = tile_sum; l.n[0] = g1 * g2; l.scale[0] = 1.0; l.out[0] = scal3 + 0;
  l.x[1] = uq1; l.n[1] = n1; l.scale[1] = 1.0; l.out[1] = scal3 + 1;
  l.x[2] = uq2; l.n[2] = n2; l.scale[2] = 1.0; l.out[2] = scal3 + 2;
  hipLaunchKernelGGL(sum_list_kernel, dim3(3), dim3(1024), 0, s, l);
  GP_HIP(hipGetLastError());
  return 0;
}

template <typename R>
int launch_adjoint(const R* W, const R* Cos, int64_t ld, const R* b, const R* q, int n, int np, R* Aout,
                   double* upart, double* vpart, double* sumA_part, hipStream_t s) {
  const int t = np / 64, nt = t * (t + 1) / 2;
  hipLaunchKernelGGL(adjoint_kernel<R>, dim3(nt), dim3(256), 0, s, W, Cos, ld, b, q, n, np, Aout, upart, vpart,
                     sumA_part);
  GP_HIP(hipGetLastError());
  return 0;
}

template <typename R>
int launch_adjoint_reduce(const double* upart, const double* vpart, const double* sumA_part, int ntile,
                          int ntile_tri, const R* q, const R* wl, int n, int np, R* tvec, double* uq,
                          double* scal_out, hipStream_t s) {
  hipLaunchKernelGGL(adjoint_u_kernel<R>, dim3((np + 31) / 32), dim3(256), 0, s, upart, vpart, ntile, q, wl, n,
                     np, tvec, uq);
  hipLaunchKernelGGL(adjoint_sums_kernel<R>, dim3(3), dim3(1024), 0, s, uq, wl, n, sumA_part, ntile_tri, scal_out);
  GP_HIP(hipGetLastError());
  return 0;
}

template <typename R>
__global__ void rowscale_add_kernel(R* __restrict__ Y, int64_t ldy, const R* __restrict__ Xm, int64_t ldm,
                                    const R* __restrict__ t, int dp, R scale) {
  const int i = blockIdx.y;
  const R ti = scale * t[i];
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < dp; k += gridDim.x * blockDim.x)
    Y[(int64_t)i * ldy + k] += ti * Xm[(int64_t)i * ldm + k];
}

template <typename R>
int launch_rowscale_add(R* Y, int64_t ldy, const R* Xm, int64_t ldm, const R* t, int np, int dp, hipStream_t s, double scale) {
  hipLaunchKernelGGL(rowscale_add_kernel<R>, dim3((dp + 255) / 256, np), dim3(256), 0, s, Y, ldy, Xm, ldm, t, dp, (R)scale);
  GP_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ metric contraction
// grad5[p] = sum_kl dC_p[k][l] M[k][l], dC_p rebuilt from C and the pixel coordinates
// (utils.py:902-909), order Amp, -2log2beta, -log2rho2, eps_0x, eps_0y.
// METRIC_BLOCKS workgroups take the rows of the d x d matrices cyclically; each leaves its five partial
// sums in part[block][5] and the last one to arrive (ticket counter, reset for the next call) adds the
// partials in block order, so the result does not depend on the arrival order.  (The single-workgroup
// version of round 1 took 105 us at d = 256, at the end of every evaluation's critical path.)
constexpr int METRIC_BLOCKS = 32;
template <typename R>
__global__ __launch_bounds__(256) void metric_contract_kernel(Theta th, const int* __restrict__ pix, int d, int n_rows,
                                                              int n_cols, const R* __restrict__ C, int64_t ldc,
                                                              const R* __restrict__ M, int64_t ldm,
                                                              double* __restrict__ grad5, double* __restrict__ part,
                                                              int* __restrict__ ticket) {
  __shared__ double sh[17];
  __shared__ int last;
  double g[5] = {0, 0, 0, 0, 0};
  for (int i = blockIdx.x; i < d; i += gridDim.x) {
    const int pi = pix[i];
    const double xi = lin_pm1(pi % n_cols, n_cols), yi = lin_pm1(pi / n_cols, n_rows);
    const double dxi = xi - th.eps0x, dyi = yi - th.eps0y;
    const double lai = -th.eb * (dxi * dxi + dyi * dyi);
    for (int j = threadIdx.x; j < d; j += blockDim.x) {
      const int pj = pix[j];
      const double xj = lin_pm1(pj % n_cols, n_cols), yj = lin_pm1(pj / n_cols, n_rows);
      const double dxj = xj - th.eps0x, dyj = yj - th.eps0y;
      const double laj = -th.eb * (dxj * dxj + dyj * dyj);
      const double ex = xj - xi, ey = yj - yi;
      const double ls = -th.er * (ex * ex + ey * ey);
      const double c = (double)C[(int64_t)i * ldc + j];
      const double mm = (double)M[(int64_t)i * ldm + j];
      g[0] += (c / th.amp) * mm;
      g[1] += (c * (lai + laj)) * mm;
      g[2] += (c * ls) * mm;
      g[3] += (2.0 * th.eb * c * (xi + xj - 2.0 * th.eps0x)) * mm;
      g[4] += (2.0 * th.eb * c * (yi + yj - 2.0 * th.eps0y)) * mm;
    }
  }
#pragma unroll
  for (int p = 0; p < 5; ++p) {
    const double v = block_sum(g[p], sh);
    if (threadIdx.x == 0) part[blockIdx.x * 5 + p] = v;
  }
  if (threadIdx.x == 0) {
    __threadfence();                                    // partials visible before the ticket
    last = (atomicAdd(ticket, 1) == (int)gridDim.x - 1);
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  if (threadIdx.x < 5) {
    double v = 0.0;
    for (int b = 0; b < (int)gridDim.x; ++b) v += __hip_atomic_load(&part[b * 5 + threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    grad5[threadIdx.x] = v;
  }
  if (threadIdx.x == 0) *ticket = 0;
}

// part: >= 5 * METRIC_BLOCKS doubles of scratch; ticket: a device int that is 0 between calls
template <typename R>
int launch_metric_contract(const Theta& th, const int* pix, int d, int n_rows, int n_cols, const R* C, int64_t ldc,
                           const R* M, int64_t ldm, double* grad5, double* part, int* ticket, hipStream_t s) {
  hipLaunchKernelGGL(metric_contract_kernel<R>, dim3(METRIC_BLOCKS), dim3(256), 0, s, th, pix, d, n_rows, n_cols, C,
                     ldc, M, ldm, grad5, part, ticket);
  GP_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ generic API helpers
// dst[dp][ldd] <- src[d][lds] zero padded
__device__ __forceinline__ void pad_copy_body(const double* __restrict__ src, int64_t lds, int rows, int cols,
                                              double* __restrict__ dst, int64_t ldd, int prow, int pcol) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j >= pcol || i >= prow) return;
  dst[(int64_t)i * ldd + j] = (i < rows && j < cols) ? src[(int64_t)i * lds + j] : 0.0;
}
__global__ void pad_copy_kernel(const double* __restrict__ src, int64_t lds, int rows, int cols,
                                double* __restrict__ dst, int64_t ldd, int prow, int pcol) {
  pad_copy_body(src, lds, rows, cols, dst, ldd, prow, pcol);
}
__global__ void pad_copy_group_kernel(PerUnit<const double*> src, PerUnit<int64_t> lds, PerUnit<int> rows, PerUnit<int> cols,
                                      PerUnit<double*> dst, int64_t ldd, int prow, int pcol) {
  const int u = blockIdx.z;
  pad_copy_body(src[u], lds[u], rows[u], cols[u], dst[u], ldd, prow, pcol);
}
int launch_pad_copy_group(int n_units, PerUnit<const double*> src, PerUnit<int64_t> lds, PerUnit<int> rows, PerUnit<int> cols,
                          PerUnit<double*> dst, int64_t ldd, int prow, int pcol, hipStream_t s) {
  hipLaunchKernelGGL(pad_copy_group_kernel, dim3((pcol + 255) / 256, prow, n_units), dim3(256), 0, s, src, lds, rows, cols,
                     dst, ldd, prow, pcol);
  GP_HIP(hipGetLastError());
  return 0;
}
int launch_pad_copy_group(int n_units, PerUnit<const double*> src, PerUnit<int64_t> lds, int rows, PerUnit<int> cols,
                          PerUnit<double*> dst, int64_t ldd, int prow, int pcol, hipStream_t s) {
  PerUnit<int> r{};
  for (int u = 0; u < n_units; ++u) r.v[u] = rows;
  return launch_pad_copy_group(n_units, src, lds, r, cols, dst, ldd, prow, pcol, s);
}

int launch_pad_copy(const double* src, int64_t lds, int rows, int cols, double* dst, int64_t ldd, int prow,
                    int pcol, hipStream_t s) {
  hipLaunchKernelGGL(pad_copy_kernel, dim3((pcol + 255) / 256, prow), dim3(256), 0, s, src, lds, rows, cols, dst,
                     ldd, prow, pcol);
  GP_HIP(hipGetLastError());
  return 0;
}

// K <- (K + K^T)/2 for a square n x n matrix (reference utils.py:1024-1025 when n1 == n2 but x1 != x2)
__device__ __forceinline__ void symmetrize_avg_body(double* __restrict__ A, int64_t lda, int n) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (i >= n || j >= i) return;
  const double a = A[(int64_t)i * lda + j], b = A[(int64_t)j * lda + i];
  const double v = (a + b) / 2.0;
  A[(int64_t)i * lda + j] = v;
  A[(int64_t)j * lda + i] = v;
}
__global__ void symmetrize_avg_kernel(double* __restrict__ A, int64_t lda, int n) { symmetrize_avg_body(A, lda, n); }
// (the grid covers the largest n of the group: a unit's blocks beyond its own n return at once, as the single form's do)
__global__ void symmetrize_avg_group_kernel(PerUnit<double*> A, int64_t lda, PerUnit<int> n) {
  const int u = blockIdx.z;
  symmetrize_avg_body(A[u], lda, n[u]);
}
int launch_symmetrize_avg_group(int n_units, PerUnit<double*> A, int64_t lda, PerUnit<int> n, hipStream_t s) {
  int nmax = 0;
  for (int u = 0; u < n_units; ++u) nmax = std::max(nmax, n.v[u]);
  if (nmax <= 0) return 0;
  hipLaunchKernelGGL(symmetrize_avg_group_kernel, dim3((nmax + 255) / 256, nmax, n_units), dim3(256), 0, s, A, lda, n);
  GP_HIP(hipGetLastError());
  return 0;
}

int launch_symmetrize_avg(double* A, int64_t lda, int n, hipStream_t s) {
  hipLaunchKernelGGL(symmetrize_avg_kernel, dim3((n + 255) / 256, n), dim3(256), 0, s, A, lda, n);
  GP_HIP(hipGetLastError());
  return 0;
}

// dK/dsigma_0 (utils.py:996-1004): pure element-wise from q1, q2 and cos(delta)
__global__ void dk_sigma0_kernel(const double* __restrict__ Cos, int64_t ldc, const double* __restrict__ q1,
                                 const double* __restrict__ q2, int n1, int n2, double s0,
                                 double* __restrict__ dK, int64_t ldk) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (i >= n1 || j >= n2) return;
  const double c = Cos[(int64_t)i * ldc + j];
  const double a = q1[i], b = q2[j], qq = a * b;
  const double delta = acos(c);
  const double J = (sqrt(1.0 - c * c) + PI32 * c - delta * c) / PI32;
  const double dqq = s0 * s0 * (b / a + a / b);        // :996
  const double dcos = (2.0 * s0 * s0 - c * dqq) / qq;  // :998
  const double dJ = -(delta - PI32) * dcos / PI32;     // :1000
  dK[(int64_t)i * ldk + j] = (qq * dJ + dqq * J) / s0; // :1004
}

int launch_dk_sigma0(const double* Cos, int64_t ldc, const double* q1, const double* q2, int n1, int n2,
                     double s0, double* dK, int64_t ldk, hipStream_t s) {
  hipLaunchKernelGGL(dk_sigma0_kernel, dim3((n2 + 255) / 256, n1), dim3(256), 0, s, Cos, ldc, q1, q2, n1, n2, s0,
                     dK, ldk);
  GP_HIP(hipGetLastError());
  return 0;
}

// dq[i] = 0.5 * sum_k Xt[k][i] * XDt[k][i] / q[i]   (utils.py:1012-1013);  h = the plain sum (:1042)
__global__ void dq_kernel(const double* __restrict__ Xt, const double* __restrict__ XDt, int64_t ld, int dp,
                          int n, const double* __restrict__ q, double* __restrict__ dq, double* __restrict__ h) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double v = 0.0;
  for (int k = 0; k < dp; ++k) v += Xt[(int64_t)k * ld + i] * XDt[(int64_t)k * ld + i];
  if (h) h[i] = v;
  if (dq) dq[i] = 0.5 * v / q[i];
}

int launch_dq(const double* Xt, const double* XDt, int64_t ld, int dp, int n, const double* q, double* dq,
              double* h, hipStream_t s) {
  hipLaunchKernelGGL(dq_kernel, dim3((n + 255) / 256), dim3(256), 0, s, Xt, XDt, ld, dp, n, q, dq, h);
  GP_HIP(hipGetLastError());
  return 0;
}

// dK_p = qq dJ + dqq J from H = x1 dC_p x2^T (utils.py:1015-1021); H is overwritten in place
__global__ void dk_metric_kernel(double* __restrict__ H, int64_t ldh, const double* __restrict__ Cos, int64_t ldc,
                                 const double* __restrict__ q1, const double* __restrict__ q2,
                                 const double* __restrict__ dq1, const double* __restrict__ dq2, int n1, int n2) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (i >= n1 || j >= n2) return;
  const double c = Cos[(int64_t)i * ldc + j];
  const double a = q1[i], b = q2[j], qq = a * b;
  const double delta = acos(c);
  const double J = (sqrt(1.0 - c * c) + PI32 * c - delta * c) / PI32;
  const double dqq = dq1[i] * b + a * dq2[j];                       // :1015
  const double dcos = (H[(int64_t)i * ldh + j] - c * dqq) / qq;      // :1017
  const double dJ = -(delta - PI32) * dcos / PI32;                   // :1019
  H[(int64_t)i * ldh + j] = qq * dJ + dqq * J;                       // :1021
}

int launch_dk_metric(double* H, int64_t ldh, const double* Cos, int64_t ldc, const double* q1, const double* q2,
                     const double* dq1, const double* dq2, int n1, int n2, hipStream_t s) {
  hipLaunchKernelGGL(dk_metric_kernel, dim3((n2 + 255) / 256, n1), dim3(256), 0, s, H, ldh, Cos, ldc, q1, q2, dq1,
                     dq2, n1, n2);
  GP_HIP(hipGetLastError());
  return 0;
}

template <typename R>
__global__ void add_diag_kernel(R* __restrict__ A, int64_t lda, int n, double v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) A[(int64_t)i * lda + i] += (R)v;
}

template <typename R>
int launch_add_diag(R* A, int64_t lda, int n, double v, hipStream_t s) {
  hipLaunchKernelGGL(add_diag_kernel<R>, dim3((n + 255) / 256), dim3(256), 0, s, A, lda, n, v);
  GP_HIP(hipGetLastError());
  return 0;
}
__global__ void add_diag_group_kernel(PerUnit<double*> A, int64_t lda, int n, double v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) A[blockIdx.y][(int64_t)i * lda + i] += v;
}
int launch_add_diag_group(int n_units, PerUnit<double*> A, int64_t lda, int n, double v, hipStream_t s) {
  hipLaunchKernelGGL(add_diag_group_kernel, dim3((n + 255) / 256, n_units), dim3(256), 0, s, A, lda, n, v);
  GP_HIP(hipGetLastError());
  return 0;
}

// dst[i] = alpha * src[i]
template <typename R>
__global__ void scale_copy_kernel(R* __restrict__ dst, const R* __restrict__ src, int n, R alpha) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = alpha * src[i];
}

template <typename R>
int launch_scale_copy(R* dst, const R* src, int n, double alpha, hipStream_t s) {
  hipLaunchKernelGGL(scale_copy_kernel<R>, dim3((n + 255) / 256), dim3(256), 0, s, dst, src, n, (R)alpha);
  GP_HIP(hipGetLastError());
  return 0;
}

// dst[r][c] = a * dst[r][c] + b * src[r][c] over a rows x cols block (cols even, 16-byte rows)
template <typename R>
__global__ void axpby_block_kernel(R* __restrict__ dst, int64_t ldd, const R* __restrict__ src, int64_t lds, int rows,
                                   int cols, R a, R b) {
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * 2;
  const int r = blockIdx.y;
  if (c >= cols || r >= rows) return;
  R* d = dst + (int64_t)r * ldd + c;
  const R* q = src + (int64_t)r * lds + c;
  d[0] = a * d[0] + b * q[0];
  d[1] = a * d[1] + b * q[1];
}

template <typename R>
int launch_axpby_block(R* dst, int64_t ldd, const R* src, int64_t lds, int rows, int cols, double a, double b,
                       hipStream_t s) {
  hipLaunchKernelGGL(axpby_block_kernel<R>, dim3((cols / 2 + 255) / 256, rows), dim3(256), 0, s, dst, ldd, src, lds,
                     rows, cols, (R)a, (R)b);
  GP_HIP(hipGetLastError());
  return 0;
}

__global__ void fill_kernel(double* __restrict__ x, int64_t n, double v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] = v;
}

int launch_fill(double* x, int64_t n, double v, hipStream_t s) {
  hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, v);
  GP_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ E-step helpers
// s_i = A sqrt(f_i) ; rhs_i = A^2 f_i m_i + A (r_i - f_i)   (utils.py:1421-1422, 1431 with a = I)
// (the body is shared by the by-value kernel and the chain's, which forms A on the device: equal A, equal bits)
__device__ __forceinline__ void estep_prep_body(const double* __restrict__ f, const double* __restrict__ r,
                                                const double* __restrict__ m, int n, int np, double A,
                                                double* __restrict__ sv, double* __restrict__ rhs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  if (i >= n) {
    sv[i] = 0.0;
    rhs[i] = 0.0;
    return;
  }
  sv[i] = A * sqrt(f[i]);
  rhs[i] = A * A * f[i] * m[i] + A * (r[i] - f[i]);
}
__global__ void estep_prep_kernel(const double* __restrict__ f, const double* __restrict__ r,
                                  const double* __restrict__ m, int n, int np, double A, double* __restrict__ sv,
                                  double* __restrict__ rhs) {
  estep_prep_body(f, r, m, n, np, A, sv, rhs);
}
// A step of gpfit_estep_chain_full / _batch (unit u = blockIdx.y): A = exp(logA) of the unit's chain block, recorded for
// the caller while the chain runs; the context's four info words are zeroed here, by the first kernel of the step (as
// estep_proj_rows_chain_group_kernel does)
__global__ void estep_prep_chain_group_kernel(PerUnit<double*> f, PerUnit<const double*> r, PerUnit<double*> m, int n, int np,
                                              PerUnit<ChainBlock*> blks, int step, PerUnit<int*> infos, PerUnit<double*> sv,
                                              PerUnit<double*> rhs) {
  const int u = blockIdx.y;
  ChainBlock* __restrict__ blk = blks[u];
  const double A = exp(blk->logA);
  if (blockIdx.x == 0 && threadIdx.x == 0 && blk->stop == 0) blk->rec[step][CR_A] = A;
  if (blockIdx.x == 0 && threadIdx.x < 4) infos[u][threadIdx.x] = 0;
  estep_prep_body(f[u], r[u], m[u], n, np, A, sv[u], rhs[u]);
}

int launch_estep_prep(const double* f, const double* r, const double* m, int n, int np, double A, double* sv,
                      double* rhs, hipStream_t s) {
  hipLaunchKernelGGL(estep_prep_kernel, dim3((np + 255) / 256), dim3(256), 0, s, f, r, m, n, np, A, sv, rhs);
  GP_HIP(hipGetLastError());
  return 0;
}
int launch_estep_prep_chain_group(const ChainGroupT& g, int step, hipStream_t s) {
  hipLaunchKernelGGL(estep_prep_chain_group_kernel, dim3((g.npc + 255) / 256, g.n_units), dim3(256), 0, s, g.f, g.r, g.m, g.n,
                     g.npc, g.blk, step, g.info, g.sv, g.u);
  GP_HIP(hipGetLastError());
  return 0;
}

// M = I + diag(s) K diag(s) (lower 128-tiles, identity padding), SK = diag(s) K (full, zero padded),
// Kl = K (lower 128-tiles, zero padded) -- one pass over K
// (the body is shared by the single kernel and the unit-batched one: every element by the same expression, whatever
// the grid)
__device__ __forceinline__ void estep_build_body(const double* __restrict__ K, int64_t ldk, int n,
                                                 const double* __restrict__ sv, double* __restrict__ Mb,
                                                 double* __restrict__ SK, double* __restrict__ Kl, int64_t ld) {
  const int tj = blockIdx.x, ti = blockIdx.y;
  const int r0 = ti * TILE, c0 = tj * TILE;
  for (int e = threadIdx.x; e < TILE * TILE; e += blockDim.x) {
    const int i = r0 + (e >> 7), j = c0 + (e & 127);
    const bool in = (i < n && j < n);
    const double k = in ? K[(int64_t)i * ldk + j] : 0.0;
    const double si = sv[i];
    SK[(int64_t)i * ld + j] = si * k;
    if (tj <= ti) {
      Mb[(int64_t)i * ld + j] = si * k * sv[j] + ((i == j) ? 1.0 : 0.0);
      Kl[(int64_t)i * ld + j] = k;
    }
  }
}
__global__ void estep_build_kernel(const double* __restrict__ K, int64_t ldk, int n, const double* __restrict__ sv,
                                   double* __restrict__ Mb, double* __restrict__ SK, double* __restrict__ Kl,
                                   int64_t ld) {
  estep_build_body(K, ldk, n, sv, Mb, SK, Kl, ld);
}
// the same pass for every unit of a group (unit u = blockIdx.z, its own K and ldk)
__global__ void estep_build_group_kernel(PerUnit<const double*> K, PerUnit<int64_t> ldk, int n, PerUnit<double*> sv,
                                         PerUnit<double*> Mb, PerUnit<double*> SK, PerUnit<double*> Kl, int64_t ld) {
  const int u = blockIdx.z;
  estep_build_body(K[u], ldk[u], n, sv[u], Mb[u], SK[u], Kl[u], ld);
}

int launch_estep_build(const double* K, int64_t ldk, int n, int np, const double* sv, double* Mb, double* SK,
                       double* Kl, int64_t ld, hipStream_t s) {
  hipLaunchKernelGGL(estep_build_kernel, dim3(np / TILE, np / TILE), dim3(256), 0, s, K, ldk, n, sv, Mb, SK, Kl, ld);
  GP_HIP(hipGetLastError());
  return 0;
}
int launch_estep_build_group(const ChainGroupT& g, hipStream_t s) {
  hipLaunchKernelGGL(estep_build_group_kernel, dim3(g.npc / TILE, g.npc / TILE, g.n_units), dim3(256), 0, s, g.K, g.ldk, g.n,
                     g.sv, g.W, g.SK, g.Vw, g.ld);
  GP_HIP(hipGetLastError());
  return 0;
}

// y = A x for a symmetric matrix stored in its lower triangle (row-major): one wave per row
// gathers the row part (j <= i) and the column part (j > i) of row i.
__device__ __forceinline__ void symv_lower_body(const double* __restrict__ A, int64_t lda, int n,
                                                const double* __restrict__ x, double* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (i >= n) return;
  double v = 0.0;
  for (int j = lane; j <= i; j += 64) v += A[(int64_t)i * lda + j] * x[j];
  for (int j = i + 1 + lane; j < n; j += 64) v += A[(int64_t)j * lda + i] * x[j];
  v = wave_sum(v);
  if (lane == 0) y[i] = v;
}
__global__ void symv_lower_kernel(const double* __restrict__ A, int64_t lda, int n, const double* __restrict__ x,
                                  double* __restrict__ y) {
  symv_lower_body(A, lda, n, x, y);
}
__global__ void symv_lower_group_kernel(PerUnit<double*> A, int64_t lda, int n, PerUnit<double*> x, PerUnit<double*> y) {
  const int u = blockIdx.y;
  symv_lower_body(A[u], lda, n, x[u], y[u]);
}
int launch_symv_lower_group(int n_units, PerUnit<double*> A, int64_t lda, int n, PerUnit<double*> x, PerUnit<double*> y,
                            hipStream_t s) {
  hipLaunchKernelGGL(symv_lower_group_kernel, dim3((n + 3) / 4, n_units), dim3(256), 0, s, A, lda, n, x, y);
  GP_HIP(hipGetLastError());
  return 0;
}

int launch_symv_lower(const double* A, int64_t lda, int n, const double* x, double* y, hipStream_t s) {
  hipLaunchKernelGGL(symv_lower_kernel, dim3((n + 3) / 4), dim3(256), 0, s, A, lda, n, x, y);
  GP_HIP(hipGetLastError());
  return 0;
}

// dst[n][ldd] (full symmetric) <- lower triangle of src[np][lds]
__global__ void unpack_sym_kernel(const double* __restrict__ src, int64_t lds, int n, double* __restrict__ dst,
                                  int64_t ldd) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (i >= n || j >= n) return;
  dst[(int64_t)i * ldd + j] = (j <= i) ? src[(int64_t)i * lds + j] : src[(int64_t)j * lds + i];
}

int launch_unpack_sym(const double* src, int64_t lds, int n, double* dst, int64_t ldd, hipStream_t s) {
  hipLaunchKernelGGL(unpack_sym_kernel, dim3((n + 255) / 256, n), dim3(256), 0, s, src, lds, n, dst, ldd);
  GP_HIP(hipGetLastError());
  return 0;
}

// dst[np][ldd] <- the lower triangle of src[n][lds]: zero above the diagonal (whatever src holds there), identity on the
// padding; every element of the np x np block is written
__device__ __forceinline__ void pack_tri_body(const double* __restrict__ src, int64_t lds, int n, double* __restrict__ dst,
                                              int64_t ldd, int np) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (i >= np || j >= np) return;
  double v = (i == j) ? 1.0 : 0.0;
  if (i < n && j < n) v = (j <= i) ? src[(int64_t)i * lds + j] : 0.0;
  dst[(int64_t)i * ldd + j] = v;
}
__global__ void pack_tri_kernel(const double* __restrict__ src, int64_t lds, int n, double* __restrict__ dst, int64_t ldd,
                                int np) {
  pack_tri_body(src, lds, n, dst, ldd, np);
}
// the same for every unit of a group: unit = blockIdx.z
__global__ void pack_tri_group_kernel(PerUnit<const double*> src, PerUnit<int64_t> lds, PerUnit<int> n, PerUnit<double*> dst,
                                      int64_t ldd, int np) {
  const int u = blockIdx.z;
  pack_tri_body(src[u], lds[u], n[u], dst[u], ldd, np);
}

int launch_pack_tri(const double* src, int64_t lds, int n, double* dst, int64_t ldd, int np, hipStream_t s) {
  hipLaunchKernelGGL(pack_tri_kernel, dim3((np + 255) / 256, np), dim3(256), 0, s, src, lds, n, dst, ldd, np);
  GP_HIP(hipGetLastError());
  return 0;
}
int launch_pack_tri_group(int n_units, PerUnit<const double*> src, PerUnit<int64_t> lds, PerUnit<int> n, PerUnit<double*> dst,
                          int64_t ldd, int np, hipStream_t s) {
  hipLaunchKernelGGL(pack_tri_group_kernel, dim3((np + 255) / 256, np, n_units), dim3(256), 0, s, src, lds, n, dst, ldd, np);
  GP_HIP(hipGetLastError());
  return 0;
}

// ---- the small kernels of a chained E-step (kernels.h: ChainBlock, ChainGate, ChainGroupT)
// the full-rank moments behind a committed update (gpfit_estep_chain_full / _batch; a = B = I; unit u = blockIdx.y behind
// its own gate): lam_m = m_new and lam_var = (Kvec - diag K~) + diag V, the diagonal read from the lower-tile work
// matrix the update left
__global__ void estep_full_moments_chain_group_kernel(PerUnit<ChainBlock*> blk, PerUnit<int*> info, PerUnit<double*> m_new,
                                                      PerUnit<double*> Vw, int64_t ld, PerUnit<const double*> kv0, int n,
                                                      PerUnit<double*> lam_m, PerUnit<double*> lam_var) {
  const int u = blockIdx.y;
  const ChainGate g{&blk[u]->stop, info[u]};
  if (!g.open()) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  lam_m[u][i] = m_new[u][i];
  lam_var[u][i] = kv0[u][i] + Vw[u][(int64_t)i * ld + i];
}
int launch_estep_full_moments_chain_group(const ChainGroupT& g, hipStream_t s) {
  hipLaunchKernelGGL(estep_full_moments_chain_group_kernel, dim3((g.n + 255) / 256, g.n_units), dim3(256), 0, s, g.blk, g.info,
                     g.mo, g.Vw, g.ld, g.kv0, g.n, g.lam_m, g.lam_var);
  GP_HIP(hipGetLastError());
  return 0;
}

// the bookkeeping and the gated commits of a step for a group of chains (the single call is the group of one): unit u =
// the free grid dimension, its own block and info word behind every gate
__global__ __launch_bounds__(256) void chain_init_group_kernel(PerUnit<ChainBlock*> blk, PerUnit<double> logA0,
                                                               PerUnit<double> lambda0, int n_rec) {
  const int u = blockIdx.x;
  ChainBlock* b = blk[u];
  double* rec = &b->rec[0][0];
  for (int i = threadIdx.x; i < n_rec; i += 256) rec[i] = 0.0;
  if (threadIdx.x == 0) {
    b->logA = logA0[u];
    b->lambda0 = lambda0[u];
    b->stop = 0;
  }
}
int launch_chain_init_group(const ChainGroupT& g, int n_steps, hipStream_t s) {
  hipLaunchKernelGGL(chain_init_group_kernel, dim3(g.n_units), dim3(256), 0, s, g.blk, g.logA0, g.lambda0, n_steps * CHAIN_REC);
  GP_HIP(hipGetLastError());
  return 0;
}
__global__ void chain_info_group_kernel(PerUnit<ChainBlock*> blk, PerUnit<int*> info, int step) {
  ChainBlock* b = blk[blockIdx.x];
  if (b->stop != 0) return;   // a skipped step: its factorisation ran on workspace only, its record stays zero
  const int v = info[blockIdx.x][0];
  b->rec[step][CR_INFO] = v;
  if (v != 0) b->stop = 1;
}
int launch_chain_info_group(const ChainGroupT& g, int step, hipStream_t s) {
  hipLaunchKernelGGL(chain_info_group_kernel, dim3(g.n_units), dim3(1), 0, s, g.blk, g.info, step);
  GP_HIP(hipGetLastError());
  return 0;
}
__global__ void chain_copy_group_kernel(PerUnit<ChainBlock*> blk, PerUnit<int*> info, PerUnit<double*> src, PerUnit<int> n,
                                        PerUnit<double*> dst) {
  const int u = blockIdx.y;
  const ChainGate g{&blk[u]->stop, info[u]};
  if (!g.open()) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n[u]) dst[u][i] = src[u][i];
}
int launch_chain_copy_group(const ChainGroupT& g, hipStream_t s) {
  hipLaunchKernelGGL(chain_copy_group_kernel, dim3((g.kmax + 255) / 256, g.n_units), dim3(256), 0, s, g.blk, g.info, g.mo, g.nb,
                     g.m);
  GP_HIP(hipGetLastError());
  return 0;
}
__global__ void unpack_sym_chain_group_kernel(PerUnit<ChainBlock*> blk, PerUnit<int*> info, PerUnit<double*> srcs, int64_t lds,
                                              PerUnit<int> ns, PerUnit<double*> dsts, PerUnit<int64_t> ldds) {
  const int u = blockIdx.z;
  const ChainGate g{&blk[u]->stop, info[u]};
  if (!g.open()) return;
  const int n = ns[u];
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (i >= n || j >= n) return;
  const double* __restrict__ src = srcs[u];
  dsts[u][(int64_t)i * ldds[u] + j] = (j <= i) ? src[(int64_t)i * lds + j] : src[(int64_t)j * lds + i];
}
int launch_unpack_sym_chain_group(const ChainGroupT& g, hipStream_t s) {
  hipLaunchKernelGGL(unpack_sym_chain_group_kernel, dim3((g.kmax + 255) / 256, g.kmax, g.n_units), dim3(256), 0, s, g.blk, g.info,
                     g.Vw, g.ld, g.nb, g.V, g.ldv);
  GP_HIP(hipGetLastError());
  return 0;
}
__global__ __launch_bounds__(256) void chain_collect_group_kernel(PerUnit<ChainBlock*> blk, PerUnit<double*> rec_host, int n_rec) {
  const double* rec = &blk[blockIdx.x]->rec[0][0];
  double* out = rec_host[blockIdx.x];
  for (int i = threadIdx.x; i < n_rec; i += 256) out[i] = rec[i];
  __threadfence_system();
}
int launch_chain_collect_group(const ChainGroupT& g, int n_steps, hipStream_t s) {
  hipLaunchKernelGGL(chain_collect_group_kernel, dim3(g.n_units), dim3(256), 0, s, g.blk, g.rec_host, n_steps * CHAIN_REC);
  GP_HIP(hipGetLastError());
  return 0;
}

// ---- the damped step of a chain (gpfit_estep_chain_damped / _batch; kernels.h): unit = blockIdx.y.  The fallback test
// is block-uniform: every thread reads the unit's one word of the V chain
__global__ __launch_bounds__(256) void chain_keep2_group_kernel(PerUnit<double*> src, PerUnit<double*> d0, PerUnit<double*> d1,
                                                                int64_t count) {
  const int u = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const double v = src[u][i];
  d0[u][i] = v;
  d1[u][i] = v;
}
int launch_chain_keep2_group(int n_units, PerUnit<double*> src, PerUnit<double*> d0, PerUnit<double*> d1, int64_t count,
                             hipStream_t s) {
  hipLaunchKernelGGL(chain_keep2_group_kernel, dim3((unsigned)((count + 255) / 256), n_units), dim3(256), 0, s, src, d0, d1, count);
  GP_HIP(hipGetLastError());
  return 0;
}
// (the expression of axpby_block_kernel: the damped mean of gpfit_estep_projected_damped, bit for bit)
__global__ __launch_bounds__(256) void chain_damped_mean_group_kernel(PerUnit<const int*> info_v, PerUnit<double*> mo,
                                                                      PerUnit<double*> m, PerUnit<int> nb, double a, double b) {
  const int u = blockIdx.y;
  if (*info_v[u] != 0) return;   // V is not positive definite: the full step's mean stays
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nb[u]) return;
  double* d = mo[u] + j;
  const double* q = m[u] + j;
  d[0] = a * d[0] + b * q[0];
}
int launch_chain_damped_mean_group(const ChainGroupT& g, PerUnit<const int*> info_v, double alpha, hipStream_t s) {
  hipLaunchKernelGGL(chain_damped_mean_group_kernel, dim3((g.kmax + 255) / 256, g.n_units), dim3(256), 0, s, info_v, g.mo, g.m,
                     g.nb, alpha, 1.0 - alpha);
  GP_HIP(hipGetLastError());
  return 0;
}
__global__ __launch_bounds__(256) void chain_damped_restore_group_kernel(PerUnit<const int*> info_v, PerUnit<double*> W1c,
                                                                         PerUnit<double*> Wa, int64_t count) {
  const int u = blockIdx.y;
  if (*info_v[u] == 0) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) Wa[u][i] = W1c[u][i];
}
int launch_chain_damped_restore_group(int n_units, PerUnit<const int*> info_v, PerUnit<double*> W1c, PerUnit<double*> Wa,
                                      int64_t count, hipStream_t s) {
  hipLaunchKernelGGL(chain_damped_restore_group_kernel, dim3((unsigned)((count + 255) / 256), n_units), dim3(256), 0, s, info_v,
                     W1c, Wa, count);
  GP_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ tracked loss (gpfit_elbo, gpfit_elbo_batch)
// unit = blockIdx.y; workgroup w owns rows w ELBO_QUAD_ROWS .. of Kinv, wave v rows 2 v and 2 v + 1 of those.  A lane
// takes the column pairs (2 lane, 2 lane + 1) + 128 k: explicit fmas in one fixed order, so that the 16-byte loads of
// an aligned row and the 8-byte loads of any other row feed the same arithmetic.
__global__ __launch_bounds__(256) void elbo_quad_group_kernel(PerUnit<const double*> Kinv, PerUnit<int64_t> ldki,
                                                              PerUnit<const double*> V, PerUnit<int64_t> ldv,
                                                              PerUnit<const double*> m, PerUnit<int> nb, PerUnit<double*> part) {
  __shared__ double sh[2][4];
  const int u = blockIdx.y, n = nb[u];
  const int r0 = blockIdx.x * ELBO_QUAD_ROWS;
  if (r0 >= n) return;   // (the whole workgroup: the grid covers the largest unit)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double* __restrict__ mu = m[u];
  double tr = 0.0, quad = 0.0;
  for (int k = 0; k < ELBO_QUAD_ROWS / 4; ++k) {
    const int i = r0 + (ELBO_QUAD_ROWS / 4) * wave + k;   // wave-uniform
    if (i >= n) break;
    const double* __restrict__ kr = Kinv[u] + (int64_t)i * ldki[u];
    const double* __restrict__ vr = V[u] + (int64_t)i * ldv[u];
    const bool aligned = (((uintptr_t)kr | (uintptr_t)vr) & 15) == 0;
    double a = 0.0, b = 0.0;
#pragma unroll 4
    for (int j = 2 * lane; j < n; j += 128) {
      double k0, k1 = 0.0, v0, v1 = 0.0, m1 = 0.0;
      if (j + 1 < n) {
        if (aligned) {
          const double2 kk = *reinterpret_cast<const double2*>(kr + j), vv = *reinterpret_cast<const double2*>(vr + j);
          k0 = kk.x; k1 = kk.y; v0 = vv.x; v1 = vv.y;
        } else {
          k0 = kr[j]; k1 = kr[j + 1]; v0 = vr[j]; v1 = vr[j + 1];
        }
        m1 = mu[j + 1];
      } else {
        k0 = kr[j]; v0 = vr[j];
      }
      a = fma(k0, v0, a); a = fma(k1, v1, a);
      b = fma(k0, mu[j], b); b = fma(k1, m1, b);
    }
    a = wave_sum(a);
    b = wave_sum(b);
    tr += a;
    quad = fma(mu[i], b, quad);
  }
  if (lane == 0) { sh[0][wave] = tr; sh[1][wave] = quad; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const double* p = sh[threadIdx.x];
    part[u][2 * blockIdx.x + threadIdx.x] = ((p[0] + p[1]) + p[2]) + p[3];
  }
}
int launch_elbo_quad_group(int n_units, PerUnit<const double*> Kinv, PerUnit<int64_t> ldki, PerUnit<const double*> V,
                           PerUnit<int64_t> ldv, PerUnit<const double*> m, PerUnit<int> nb, PerUnit<double*> part,
                           hipStream_t s) {
  int nmax = 0;
  for (int u = 0; u < n_units; ++u) nmax = std::max(nmax, nb[u]);
  hipLaunchKernelGGL(elbo_quad_group_kernel, dim3((nmax + ELBO_QUAD_ROWS - 1) / ELBO_QUAD_ROWS, n_units), dim3(256), 0, s, Kinv,
                     ldki, V, ldv, m, nb, part);
  GP_HIP(hipGetLastError());
  return 0;
}
// unit = blockIdx.y; workgroup b sums the b-th stretch of ceil(n / ELBO_ROWS_WG) training points
__global__ __launch_bounds__(256) void elbo_rows_group_kernel(PerUnit<const double*> r, PerUnit<const double*> f,
                                                              PerUnit<const double*> lam_m, int n, PerUnit<double*> part,
                                                              PerUnit<int*> info) {
  __shared__ double sh[17];
  const int u = blockIdx.y, b = blockIdx.x;
  if (b == 0 && threadIdx.x < 4) info[u][threadIdx.x] = 0;
  const int chunk = (n + ELBO_ROWS_WG - 1) / ELBO_ROWS_WG;
  const int64_t lo = (int64_t)b * chunk, hi = lo + chunk < n ? lo + chunk : n;
  const double* __restrict__ ru = r[u];
  const double* __restrict__ fu = f[u];
  const double* __restrict__ lu = lam_m[u];
  double rl = 0.0, sr = 0.0, sf = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    const double ri = ru[i];
    rl = fma(ri, lu[i], rl);
    sr += ri;
    sf += fu[i];
  }
  rl = block_sum(rl, sh);
  sr = block_sum(sr, sh);
  sf = block_sum(sf, sh);
  if (threadIdx.x == 0) { part[u][3 * b] = rl; part[u][3 * b + 1] = sr; part[u][3 * b + 2] = sf; }
}
int launch_elbo_rows_group(int n_units, PerUnit<const double*> r, PerUnit<const double*> f, PerUnit<const double*> lam_m, int n,
                           PerUnit<double*> part, PerUnit<int*> info, hipStream_t s) {
  hipLaunchKernelGGL(elbo_rows_group_kernel, dim3(ELBO_ROWS_WG, n_units), dim3(256), 0, s, r, f, lam_m, n, part, info);
  GP_HIP(hipGetLastError());
  return 0;
}
// unit = blockIdx.x; threads 0 .. 4 add one list of partials each in index order, thread 0 forms the results
__global__ __launch_bounds__(64) void elbo_finish_group_kernel(ElboFinishT g) {
  __shared__ double sums[5];
  const int u = blockIdx.x, t = threadIdx.x;
  if (t < 2) {
    const int nwg = (g.nb[u] + ELBO_QUAD_ROWS - 1) / ELBO_QUAD_ROWS;
    const double* p = g.quad_part[u];
    double acc = 0.0;
    for (int w = 0; w < nwg; ++w) acc += p[2 * w + t];
    sums[t] = acc;
  } else if (t < 5) {
    const double* p = g.rows_part[u];
    double acc = 0.0;
    for (int b = 0; b < ELBO_ROWS_WG; ++b) acc += p[3 * b + (t - 2)];
    sums[t] = acc;
  }
  __syncthreads();
  if (t != 0) return;
  const int info_V = *g.info_V[u], info_K = g.known[u] ? 0 : *g.info_K[u];
  const double tr = sums[0], mkm = sums[1], rlam = sums[2], sum_r = sums[3], sum_f = sums[4];
  const double logdet_V = *g.logdet_V[u], logdet_K = g.known[u] ? g.given[u] : *g.logdet_K[u];
  const double loglik = g.A[u] * rlam + g.lambda0[u] * sum_r - sum_f;                     // utils.py:1243
  const double KL = -0.5 * logdet_V + 0.5 * logdet_K + 0.5 * mkm + 0.5 * tr;               // utils.py:1326
  double o[ELBO_OUT] = {loglik, KL, loglik - KL, logdet_V, logdet_K, mkm, tr, rlam, sum_r, sum_f};
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (info_V != 0) o[1] = o[2] = o[3] = o[4] = nan;
  if (info_K != 0) o[1] = o[2] = o[4] = nan;
  double* out = g.out_host[u];
  for (int i = 0; i < ELBO_OUT; ++i) out[i] = o[i];
  *g.info_V_host[u] = info_V;
  *g.info_K_host[u] = info_K;
  __threadfence_system();
}
int launch_elbo_finish_group(const ElboFinishT& g, hipStream_t s) {
  hipLaunchKernelGGL(elbo_finish_group_kernel, dim3(g.n_units), dim3(64), 0, s, g);
  GP_HIP(hipGetLastError());
  return 0;
}

// dst[n][ldd] <- lower triangle of src, strict upper zeroed (triangular factor for the caller)
__global__ void unpack_tri_kernel(const double* __restrict__ src, int64_t lds, int n, double* __restrict__ dst,
                                  int64_t ldd) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (i >= n || j >= n) return;
  dst[(int64_t)i * ldd + j] = (j <= i) ? src[(int64_t)i * lds + j] : 0.0;
}

int launch_unpack_tri(const double* src, int64_t lds, int n, double* dst, int64_t ldd, hipStream_t s) {
  hipLaunchKernelGGL(unpack_tri_kernel, dim3((n + 255) / 256, n), dim3(256), 0, s, src, lds, n, dst, ldd);
  GP_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ firing-rate parameters
// One pass over the N training points for the inner logA optimiser (utils.py:1897-1934):
//   e_i = exp(A lam_m_i + A^2/2 lam_var_i)
//   lambda0 = closed form log(sum r) - log(sum e)            (utils.py:1215-1229) or the given one
//   f_i = e_i exp(lambda0)                                   (utils.py:1138)
//   loglik = A r.lam_m + lambda0 sum r - sum f               (utils.py:1243)
//   dloglik/dlogA = A (r.lam_m - sum (lam_m + A lam_var) f)  (utils.py:1253)
// The pass is shared by fparam_kernel (one evaluation) and fparam_lbfgs_kernel (the whole optimiser): at equal A
// both give the same bits.

// the totals that depend on A: sum e and sum (lam_m + A lam_var) e (valid in every thread)
__device__ __forceinline__ void fparam_sums_A(const double* __restrict__ lam_m, const double* __restrict__ lam_var,
                                              int n, double A, double* sh, double& se, double& sg) {
  double e_sum = 0.0, g_sum = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const double e = exp(A * lam_m[i] + 0.5 * A * A * lam_var[i]);
    e_sum += e;
    g_sum += (lam_m[i] + A * lam_var[i]) * e;
  }
  se = block_sum(e_sum, sh);
  sg = block_sum(g_sum, sh);
}

// the totals that do not: sum r and r.lam_m (valid in every thread)
__device__ __forceinline__ void fparam_sums_r(const double* __restrict__ lam_m, const double* __restrict__ r, int n,
                                              double* sh, double& sr, double& srm) {
  double r_sum = 0.0, rm_sum = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    r_sum += r[i];
    rm_sum += r[i] * lam_m[i];
  }
  sr = block_sum(r_sum, sh);
  srm = block_sum(rm_sum, sh);
}

// the rate f_i at (A, lambda0)
__device__ __forceinline__ void fparam_rate(const double* __restrict__ lam_m, const double* __restrict__ lam_var, int n,
                                            double A, double lambda0, double* __restrict__ f) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) f[i] = exp(A * lam_m[i] + 0.5 * A * A * lam_var[i] + lambda0);
}

// the scalars of one evaluation from the four totals
struct FparamScalars {
  double lambda0, loglik, dloglik, sum_f, lambda0_closed;
};
__device__ __forceinline__ FparamScalars fparam_scalars(double A, double se, double sg, double sr, double srm,
                                                        int closed_form, double lambda0_in) {
  FparamScalars v;
  v.lambda0 = closed_form ? (log(sr) - log(se)) : lambda0_in;
  const double el0 = exp(v.lambda0);
  v.sum_f = se * el0;
  v.loglik = A * srm + v.lambda0 * sr - v.sum_f;
  v.dloglik = A * (srm - sg * el0);
  v.lambda0_closed = log(sr) - log(se);  // closed-form lambda0 for this logA, whatever was used above
  return v;
}

// out[0] lambda0 used, out[1] loglik, out[2] dloglik/dlogA, out[3] sum f, out[4] sum r, out[5] r.lam_m,
// out[6] closed-form lambda0
__global__ void fparam_kernel(const double* __restrict__ lam_m, const double* __restrict__ lam_var,
                              const double* __restrict__ r, int n, double A, int closed_form, double lambda0_in,
                              double* __restrict__ f, double* __restrict__ out) {
  __shared__ double sh[17];
  double se, sg, sr, srm;
  fparam_sums_A(lam_m, lam_var, n, A, sh, se, sg);
  fparam_sums_r(lam_m, r, n, sh, sr, srm);
  const FparamScalars v = fparam_scalars(A, se, sg, sr, srm, closed_form, lambda0_in);
  if (f) fparam_rate(lam_m, lam_var, n, A, v.lambda0, f);
  if (threadIdx.x == 0) {
    out[0] = v.lambda0;
    out[1] = v.loglik;
    out[2] = v.dloglik;
    out[3] = v.sum_f;
    out[4] = sr;
    out[5] = srm;
    out[6] = v.lambda0_closed;
  }
}

int launch_fparam(const double* lam_m, const double* lam_var, const double* r, int n, double A, int closed_form,
                  double lambda0_in, double* f, double* out, hipStream_t s) {
  hipLaunchKernelGGL(fparam_kernel, dim3(1), dim3(1024), 0, s, lam_m, lam_var, r, n, A, closed_form, lambda0_in, f,
                     out);
  GP_HIP(hipGetLastError());
  return 0;
}

// The pass of the optimiser's closure at A = exp(logA).  The totals of the last pass are kept: the final rate is
// usually asked at the A that was evaluated last.
struct FparamDevicePass {
  const double* lam_m;
  const double* lam_var;
  int n;
  double* sh;
  double sr, srm;
  double A, se, sg;
  __device__ void pass(double logA) {
    const double A_new = exp(logA);
    if (!(A_new == A)) {
      fparam_sums_A(lam_m, lam_var, n, A_new, sh, se, sg);
      A = A_new;
    }
  }
  __device__ double lambda0_closed() const { return log(sr) - log(se); }
  __device__ FparamValues values(double lambda0_used) const {
    const FparamScalars v = fparam_scalars(A, se, sg, sr, srm, 0, lambda0_used);
    return FparamValues{v.loglik, v.dloglik, v.sum_f};
  }
};

// history slots in LDS: thread 0 writes, a barrier publishes (every thread computes the same values)
struct Lbfgs1dLdsSlots {
  __device__ static void put(double* p, int i, double v) {
    if (threadIdx.x == 0) p[i] = v;
  }
  __device__ static void publish() { __syncthreads(); }
};

// The whole rate-parameter optimiser of an E-step (utils.py:1892-1934) in one workgroup: every thread runs the scalar
// L-BFGS of lbfgs1d.h on the block totals, so the control flow is uniform.  Dynamic LDS: 4 * history_size doubles.
// The optimiser's state does not fit the 128 VGPRs a 1024-thread workgroup leaves each lane: the resource report
// shows 112 bytes per lane of register spills (the history itself is in LDS); the kernel averages 22 us per E-step.
// out[0] final logA, [1] closed-form lambda0 there, [2] first loss, [3] last loss, [4] closure calls, [5] iterations,
// [6] status (0 or the failing call), [7] logA and [8] lambda0 left by a failing call.  f: the rate at out[0..1].
// (fparam_lbfgs_run is the optimiser itself, fparam_lbfgs_store its nine results: shared with the chain's kernel)
struct FparamLbfgsRun {
  Lbfgs1dResult res;
  double lambda0, fail_x, fail_lambda0;
};
__device__ __forceinline__ FparamLbfgsRun fparam_lbfgs_run(const double* __restrict__ lam_m,
                                                           const double* __restrict__ lam_var,
                                                           const double* __restrict__ r, int n, double logA0,
                                                           int lambda0_mode, double lambda0_fixed,
                                                           const Lbfgs1dConfig& cfg, double* __restrict__ f, double* sh,
                                                           double* hist) {
  const int hs = cfg.history_size;
  FparamClosure<FparamDevicePass> obj;
  obj.ev.lam_m = lam_m;
  obj.ev.lam_var = lam_var;
  obj.ev.n = n;
  obj.ev.sh = sh;
  obj.ev.A = __builtin_nan("");
  obj.ev.se = obj.ev.sg = 0.0;
  fparam_sums_r(lam_m, r, n, sh, obj.ev.sr, obj.ev.srm);
  obj.fixed = lambda0_mode;
  obj.lambda0_fixed = lambda0_fixed;
  obj.lambda0 = 0.0;
  obj.calls = 0;
  obj.fail_x = obj.fail_lambda0 = 0.0;
  FparamLbfgsRun o;
  o.res = lbfgs1d_step<Lbfgs1dLdsSlots>(obj, logA0, cfg, Lbfgs1dStorage{hist, hist + hs, hist + 2 * hs, hist + 3 * hs});
  o.lambda0 = __builtin_nan("");
  if (o.res.status == 0) {
    // lambda0_and_rate() (utils.py:1934): the closed form at the final logA and the rate there
    obj.ev.pass(o.res.x);
    o.lambda0 = obj.ev.lambda0_closed();
    if (f) fparam_rate(lam_m, lam_var, n, obj.ev.A, o.lambda0, f);
  }
  o.fail_x = obj.fail_x;
  o.fail_lambda0 = obj.fail_lambda0;
  return o;
}
__device__ __forceinline__ void fparam_lbfgs_store(const FparamLbfgsRun& o, double* __restrict__ out) {
  out[0] = o.res.x;
  out[1] = o.lambda0;
  out[2] = o.res.first_loss;
  out[3] = o.res.last_loss;
  out[4] = o.res.n_evals;
  out[5] = o.res.n_iter;
  out[6] = o.res.status;
  out[7] = o.res.status ? o.fail_x : 0.0;
  out[8] = o.res.status ? o.fail_lambda0 : 0.0;
}
__global__ __launch_bounds__(1024) void fparam_lbfgs_kernel(const double* __restrict__ lam_m,
                                                            const double* __restrict__ lam_var,
                                                            const double* __restrict__ r, int n, double logA0,
                                                            int lambda0_mode, double lambda0_fixed, Lbfgs1dConfig cfg,
                                                            double* __restrict__ f, double* __restrict__ out) {
  __shared__ double sh[17];
  extern __shared__ double hist[];
  const FparamLbfgsRun o = fparam_lbfgs_run(lam_m, lam_var, r, n, logA0, lambda0_mode, lambda0_fixed, cfg, f, sh, hist);
  if (threadIdx.x == 0) fparam_lbfgs_store(o, out);
}
// The optimiser of a chained step: behind the gate, from the logA the block holds.  rec[0..8]: the
// nine results, rec[CR_RAN] = 1.  Status 0 leaves (logA, lambda0) in the block for the next step (and the rate in f);
// a failing closure call sets the stop word instead.
__device__ __forceinline__ void fparam_lbfgs_chain_body(ChainGate g, const double* __restrict__ lam_m,
                                                        const double* __restrict__ lam_var, const double* __restrict__ r,
                                                        int n, int lambda0_mode, double lambda0_fixed,
                                                        const Lbfgs1dConfig& cfg, double* __restrict__ f, ChainBlock* blk,
                                                        double* __restrict__ rec, double* sh, double* hist,
                                                        const int* full_step = nullptr) {
  if (!g.open()) return;   // the same two words in every thread: uniform
  const double logA0 = blk->logA;
  const FparamLbfgsRun o = fparam_lbfgs_run(lam_m, lam_var, r, n, logA0, lambda0_mode, lambda0_fixed, cfg, f, sh, hist);
  __syncthreads();         // every thread has read the gate and the block before thread 0 writes them
  if (threadIdx.x == 0) {
    fparam_lbfgs_store(o, rec + CR_LBFGS);
    rec[CR_RAN] = (full_step && *full_step != 0) ? 2.0 : 1.0;   // 2: the damped chain committed the full step
    if (o.res.status == 0) {
      blk->logA = o.res.x;
      blk->lambda0 = o.lambda0;
    } else {
      blk->stop = 1;
    }
  }
}
// one workgroup per unit of a group: each behind its own gate, from its own block
__global__ __launch_bounds__(1024) void fparam_lbfgs_chain_group_kernel(PerUnit<ChainBlock*> blks, PerUnit<int*> info,
                                                                        PerUnit<double*> lam_m, PerUnit<double*> lam_var,
                                                                        PerUnit<const double*> r, int n, int lambda0_mode,
                                                                        PerUnit<double> lambda0_fixed, Lbfgs1dConfig cfg,
                                                                        PerUnit<double*> f, int step,
                                                                        PerUnit<const int*> full_step) {
  __shared__ double sh[17];
  extern __shared__ double hist[];
  const int u = blockIdx.x;
  ChainBlock* blk = blks[u];
  fparam_lbfgs_chain_body(ChainGate{&blk->stop, info[u]}, lam_m[u], lam_var[u], r[u], n, lambda0_mode, lambda0_fixed[u], cfg,
                          f[u], blk, &blk->rec[step][0], sh, hist, full_step[u]);
}

int launch_fparam_lbfgs(const double* lam_m, const double* lam_var, const double* r, int n, double logA0,
                        int lambda0_mode, double lambda0_fixed, const Lbfgs1dConfig& cfg, double* f, double* out,
                        hipStream_t s) {
  const size_t lds = 4 * (size_t)cfg.history_size * sizeof(double);
  hipLaunchKernelGGL(fparam_lbfgs_kernel, dim3(1), dim3(1024), lds, s, lam_m, lam_var, r, n, logA0, lambda0_mode,
                     lambda0_fixed, cfg, f, out);
  GP_HIP(hipGetLastError());
  return 0;
}
int launch_fparam_lbfgs_chain_group(const ChainGroupT& g, int step, int lambda0_mode, const Lbfgs1dConfig& cfg, hipStream_t s,
                                    PerUnit<const int*> full_step) {
  const size_t lds = 4 * (size_t)cfg.history_size * sizeof(double);
  hipLaunchKernelGGL(fparam_lbfgs_chain_group_kernel, dim3(g.n_units), dim3(1024), lds, s, g.blk, g.info, g.lam_m, g.lam_var,
                     g.r, g.n, lambda0_mode, g.lambda0, cfg, g.f, step, full_step);
  GP_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ explicit instantiations
#define GP_INST(R)                                                                                                  \
  template int launch_localker<R>(const Theta&, const int*, int, int, int, int, R*, int64_t, R*, hipStream_t);      \
  template int launch_gather<R>(const R*, int64_t, int, const int*, int, int, int, R*, int64_t, R*, int64_t,        \
                                hipStream_t);                                                                       \
  template int launch_qvec<R>(const R*, const R*, int64_t, int, int, int, double, R*, R*, hipStream_t);             \
  template int launch_pack_lower<R>(const R*, int64_t, int, R*, int64_t, int, hipStream_t);                         \
  template int launch_symmetrize<R>(R*, int64_t, int, hipStream_t);                                                 \
  template int launch_logdet<R>(const R*, int64_t, int, double*, hipStream_t);                                      \
  template int launch_logdet_pair<R>(const R*, double*, const R*, double*, int64_t, int, hipStream_t);              \
  template int launch_frob_lower<R>(const R*, int64_t, int, double*, double*, hipStream_t);                         \
  template int launch_trmv_lower<R>(const R*, int64_t, int, const R*, R*, hipStream_t);                             \
  template int launch_trmv_lower_t<R>(const R*, int64_t, int, const R*, R*, double*, hipStream_t);                  \
  template int launch_gemv_sub<R>(const R*, int64_t, int, int, const R*, const R*, R*, hipStream_t);                \
  template int launch_gemv_t_sub<R>(const R*, int64_t, int, int, const R*, const R*, R*, double*, hipStream_t);     \
  template int launch_frob_tiles<R>(const R*, int64_t, int, int, int, double*, hipStream_t);                        \
  template int launch_group_prepare<R>(const GroupPrepT<R>&, hipStream_t);                                          \
  template int launch_dot<R>(const R*, const R*, int, double*, hipStream_t);                                        \
  template int launch_moments<R>(const R*, const R*, const R*, int64_t, const R*, int64_t, const R*, const R*, int, \
                                 double, double, R*, R*, R*, R*, double*, double*, int*, hipStream_t);              \
  template int launch_adjoint<R>(const R*, const R*, int64_t, const R*, const R*, int, int, R*, double*, double*,   \
                                 double*, hipStream_t);                                                             \
  template int launch_adjoint_reduce<R>(const double*, const double*, const double*, int, int, const R*, const R*,  \
                                        int, int, R*, double*, double*, hipStream_t);                               \
  template int launch_rowscale_add<R>(R*, int64_t, const R*, int64_t, const R*, int, int, hipStream_t, double);     \
  template int launch_reduce_slabs<R>(const R*, int64_t, int, int, R*, int, int, hipStream_t);                      \
  template int launch_reduce_slices_sym<R>(const R*, int64_t, int, R*, int, hipStream_t);                           \
  template int launch_reduce_slices<R, R>(const R*, int64_t, int, R*, int64_t, hipStream_t);                        \
  template int launch_metric_contract<R>(const Theta&, const int*, int, int, int, const R*, int64_t, const R*,      \
                                         int64_t, double*, double*, int*, hipStream_t);                             \
  template int launch_add_diag<R>(R*, int64_t, int, double, hipStream_t);                                           \
  template int launch_axpby_block<R>(R*, int64_t, const R*, int64_t, int, int, double, double, hipStream_t);          \
  template int launch_scale_copy<R>(R*, const R*, int, double, hipStream_t);
GP_INST(double)
GP_INST(float)
#undef GP_INST
template int launch_reduce_slices<double, float>(const double*, int64_t, int, float*, int64_t, hipStream_t);

}  // namespace gpfit
