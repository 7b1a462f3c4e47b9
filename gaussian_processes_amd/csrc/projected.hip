// Element-wise pieces of the fused truncated-rank and sparse M-step closures (gpfit_fit_eval_projected,
// gpfit_fit_eval_sparse and its _batch form; fit.hip: projected_adjoints): moments / rate / likelihood over the N x n
// projected matrices, the adjoint assembly, and the small n x n combinations.  fp64 only (the reference's
// precision; utils.py:31-33).
#include "kernels.h"

namespace gpfit {

// One wave per training point i (utils.py:1090, 1101, 1138; Bp: the matrix a of the moments, B or K_b K~_b^-1):
//   lam_m = a_i . m_b,  lam_var = Kvec_i - a_i . Kb_i + aV_i . a_i,  f = exp(A lam_m + A^2/2 lam_var + lambda0)
//   g_m = A (r - f),  g_v = -A^2 f / 2;   block partial sums of r lam_m, r, f -> part[3][gridDim.x]
// (each body below is written for one unit; its kernel puts the unit on a grid dimension the body leaves free, so a unit's
// sums run in the same order whatever else is in the launch: the same bits alone and in any group)
__device__ __forceinline__ void proj_moments_body(const double* __restrict__ Bp, const double* __restrict__ Kb,
                                                  const double* __restrict__ aV, int64_t ld, int nb,
                                                  const double* __restrict__ mb, const double* __restrict__ Kvec,
                                                  const double* __restrict__ r, int n, double A, double lambda0,
                                                  double* __restrict__ lam_m, double* __restrict__ lam_var,
                                                  double* __restrict__ f, double* __restrict__ gm,
                                                  double* __restrict__ gv, double* __restrict__ part, double (*red)[4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + w;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  if (i < n) {
    const double* b = Bp + (int64_t)i * ld;
    const double* k = Kb + (int64_t)i * ld;
    const double* a = aV + (int64_t)i * ld;
    for (int j = lane; j < nb; j += 64) {
      const double bj = b[j];
      s0 += bj * mb[j];
      s1 += bj * k[j];
      s2 += a[j] * bj;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    s0 += __shfl_down(s0, o);
    s1 += __shfl_down(s1, o);
    s2 += __shfl_down(s2, o);
  }
  if (lane == 0) {
    double c0 = 0.0, c1 = 0.0, c2 = 0.0;
    if (i < n) {
      const double lm = s0, lv = Kvec[i] - s1 + s2;
      const double fi = exp(A * lm + 0.5 * A * A * lv + lambda0);
      lam_m[i] = lm; lam_var[i] = lv; f[i] = fi;
      gm[i] = A * (r[i] - fi);
      gv[i] = -0.5 * A * A * fi;
      c0 = r[i] * lm; c1 = r[i]; c2 = fi;
    }
    red[0][w] = c0; red[1][w] = c1; red[2][w] = c2;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int q = threadIdx.x;
    part[(int64_t)q * gridDim.x + blockIdx.x] = red[q][0] + red[q][1] + red[q][2] + red[q][3];
  }
}

// out[q] = sum of part[q][0..nblk) in index order (deterministic), q = 0..2
__device__ __forceinline__ void proj_sum3_body(const double* __restrict__ part, int nblk, double* __restrict__ out, double* red) {
  for (int q = 0; q < 3; ++q) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) s += part[(int64_t)q * nblk + i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[q] = red[0];
    __syncthreads();
  }
}

// G_a = g_m m_b^T - diag(g_v) K_b + 2 diag(g_v) aV   (N x nb, rows >= n left zero)
__device__ __forceinline__ void proj_ga_body(const double* __restrict__ Kb, const double* __restrict__ aV, int64_t ld, int nb,
                                             int n, const double* __restrict__ gm, const double* __restrict__ gv,
                                             const double* __restrict__ mb, double* __restrict__ Ga) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= nb) return;
  const int64_t o = (int64_t)i * ld + j;
  Ga[o] = (i < n) ? gm[i] * mb[j] - gv[i] * Kb[o] + 2.0 * gv[i] * aV[o] : 0.0;
}

// G_Kb = diag(g_v) B - G_a K~_b^-1, in place on the product (rows >= n left zero)
__device__ __forceinline__ void proj_gkb_body(const double* __restrict__ Bp, int64_t ld, int nb, int n,
                                              const double* __restrict__ gv, double* __restrict__ GaKi) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= nb) return;
  const int64_t o = (int64_t)i * ld + j;
  GaKi[o] = (i < n) ? gv[i] * Bp[o] - GaKi[o] : 0.0;
}

// G_K~b = 1/2 K~_b^-1 - 1/2 b b^T - 1/2 (K~_b^-1 V_b K~_b^-1) + B^T G_a K~_b^-1     (nb x nb)
__device__ __forceinline__ void proj_gktb_body(const double* __restrict__ Ki, const double* __restrict__ P1,
                                               const double* __restrict__ P2, int64_t ld, int nb,
                                               const double* __restrict__ b, double* __restrict__ G) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= nb) return;
  const int64_t o = (int64_t)i * ld + j;
  G[o] = 0.5 * Ki[o] - 0.5 * b[i] * b[j] - 0.5 * P1[o] + P2[o];
}

// out[0] = sum_i A[i][i], i < n
__device__ __forceinline__ void proj_trace_body(const double* __restrict__ A, int64_t lda, int n, double* __restrict__ out,
                                                double* red) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += A[(int64_t)i * lda + i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}

// ---- the kernels (kernels.h: ProjGroupT; a single closure is the group of one): unit = the free grid dimension
__global__ __launch_bounds__(256) void proj_moments_group_kernel(PerUnit<double*> am, PerUnit<double*> Kb, PerUnit<double*> aV,
                                                                  int64_t ld, int nb, PerUnit<double*> mb, PerUnit<double*> Kvec,
                                                                  PerUnit<const double*> r, int n, PerUnit<double> A,
                                                                  PerUnit<double> lambda0, PerUnit<double*> lam_m,
                                                                  PerUnit<double*> lam_var, PerUnit<double*> f,
                                                                  PerUnit<double*> gm, PerUnit<double*> gv, PerUnit<double*> part) {
  __shared__ double red[3][4];
  const int u = blockIdx.y;
  proj_moments_body(am[u], Kb[u], aV[u], ld, nb, mb[u], Kvec[u], r[u], n, A[u], lambda0[u], lam_m[u], lam_var[u], f[u], gm[u],
                    gv[u], part[u], red);
}
__global__ __launch_bounds__(256) void proj_sum3_group_kernel(PerUnit<double*> part, int nblk, PerUnit<double*> out) {
  __shared__ double red[256];
  const int u = blockIdx.y;
  proj_sum3_body(part[u], nblk, out[u], red);
}
__global__ __launch_bounds__(256) void proj_ga_group_kernel(PerUnit<double*> Kb, PerUnit<double*> aV, int64_t ld, int nb, int n,
                                                             PerUnit<double*> gm, PerUnit<double*> gv, PerUnit<double*> mb,
                                                             PerUnit<double*> Ga) {
  const int u = blockIdx.z;
  proj_ga_body(Kb[u], aV[u], ld, nb, n, gm[u], gv[u], mb[u], Ga[u]);
}
__global__ __launch_bounds__(256) void proj_gkb_group_kernel(PerUnit<double*> am, int64_t ld, int nb, int n, PerUnit<double*> gv,
                                                              PerUnit<double*> GaKi) {
  const int u = blockIdx.z;
  proj_gkb_body(am[u], ld, nb, n, gv[u], GaKi[u]);
}
__global__ __launch_bounds__(256) void proj_gktb_group_kernel(PerUnit<double*> Ki, PerUnit<double*> P1, PerUnit<double*> P2,
                                                               int64_t ld, int nb, PerUnit<double*> b, PerUnit<double*> G) {
  const int u = blockIdx.z;
  proj_gktb_body(Ki[u], P1[u], P2[u], ld, nb, b[u], G[u]);
}
__global__ __launch_bounds__(256) void proj_trace_group_kernel(PerUnit<double*> A, int64_t lda, PerUnit<int> n, PerUnit<double*> out) {
  __shared__ double red[256];
  const int u = blockIdx.y;
  proj_trace_body(A[u], lda, n[u], out[u], red);
}
int launch_proj_moments_group(const ProjGroupT& g, hipStream_t s) {
  const int nblk = (g.n + 3) / 4;
  hipLaunchKernelGGL(proj_moments_group_kernel, dim3(nblk, g.n_units), dim3(256), 0, s, g.am, g.Kb, g.aV, g.ld, g.nb, g.mb,
                     g.Kvec, g.r, g.n, g.A, g.lambda0, g.lam_m, g.lam_var, g.f, g.gm, g.gv, g.part);
  hipLaunchKernelGGL(proj_sum3_group_kernel, dim3(1, g.n_units), dim3(256), 0, s, g.part, nblk, g.out3);
  GP_HIP(hipGetLastError());
  return 0;
}
int launch_proj_ga_group(const ProjGroupT& g, hipStream_t s) {
  hipLaunchKernelGGL(proj_ga_group_kernel, dim3((g.nb + 255) / 256, g.np, g.n_units), dim3(256), 0, s, g.Kb, g.aV, g.ld, g.nb,
                     g.n, g.gm, g.gv, g.mb, g.Ga);
  GP_HIP(hipGetLastError());
  return 0;
}
int launch_proj_gkb_group(const ProjGroupT& g, hipStream_t s) {
  hipLaunchKernelGGL(proj_gkb_group_kernel, dim3((g.nb + 255) / 256, g.np, g.n_units), dim3(256), 0, s, g.am, g.ld, g.nb, g.n,
                     g.gv, g.GaKi);
  GP_HIP(hipGetLastError());
  return 0;
}
int launch_proj_gktb_group(const ProjGroupT& g, hipStream_t s) {
  hipLaunchKernelGGL(proj_gktb_group_kernel, dim3((g.nb + 255) / 256, g.nb, g.n_units), dim3(256), 0, s, g.Ki, g.P1, g.P2, g.ld,
                     g.nb, g.bvec, g.G);
  GP_HIP(hipGetLastError());
  return 0;
}
int launch_proj_trace_group(int n_units, PerUnit<double*> A, int64_t lda, PerUnit<int> n, PerUnit<double*> out, hipStream_t s) {
  hipLaunchKernelGGL(proj_trace_group_kernel, dim3(1, n_units), dim3(256), 0, s, A, lda, n, out);
  GP_HIP(hipGetLastError());
  return 0;
}

// ---- fused E-step in the projected basis (gpfit_estep_projected, api_solve.hip)
// One wave per training point i: lam = a_i . m_b, s_i = A sqrt(f_i), u_i = A^2 f_i lam + A (r_i - f_i)
// (the right-hand side G m + g of utils.py:1431 before its projection a^T); zero on the padding rows.
// (the body is shared by the by-value kernel and the chain's, which forms A on the device: equal A, equal bits)
__device__ __forceinline__ void estep_proj_rows_body(const double* __restrict__ a, int64_t lda, int nb,
                                                     const double* __restrict__ mb, const double* __restrict__ f,
                                                     const double* __restrict__ r, int n, int nrows, double A,
                                                     double* __restrict__ sv, double* __restrict__ u) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nrows) return;
  double s0 = 0.0;
  if (i < n) {
    const double* row = a + (int64_t)i * lda;
    for (int j = lane; j < nb; j += 64) s0 += row[j] * mb[j];
  }
  for (int o = 32; o > 0; o >>= 1) s0 += __shfl_down(s0, o);
  if (lane == 0) {
    if (i < n) {
      const double fi = f[i];
      sv[i] = A * sqrt(fi);
      u[i] = A * A * fi * s0 + A * (r[i] - fi);
    } else {
      sv[i] = 0.0;
      u[i] = 0.0;
    }
  }
}
__global__ __launch_bounds__(256) void estep_proj_rows_kernel(const double* __restrict__ a, int64_t lda, int nb,
                                                               const double* __restrict__ mb, const double* __restrict__ f,
                                                               const double* __restrict__ r, int n, int nrows, double A,
                                                               double* __restrict__ sv, double* __restrict__ u) {
  estep_proj_rows_body(a, lda, nb, mb, f, r, n, nrows, A, sv, u);
}
// A step of the chained E-steps (the single call is the group of one), for every unit of the group: unit = blockIdx.y;
// A = exp(logA) of the unit's chain block, recorded for the caller while the chain runs; the unit's four info words are
// zeroed here, by the first kernel of the step
__global__ __launch_bounds__(256) void estep_proj_rows_chain_group_kernel(PerUnit<const double*> a, PerUnit<int64_t> lda,
                                                                           PerUnit<int> nb, PerUnit<double*> mb,
                                                                           PerUnit<double*> f, PerUnit<const double*> r,
                                                                           int n, int nrows, PerUnit<ChainBlock*> blks,
                                                                           PerUnit<int*> info, int step, PerUnit<double*> sv,
                                                                           PerUnit<double*> uv) {
  const int u = blockIdx.y;
  ChainBlock* blk = blks[u];
  const double A = exp(blk->logA);
  if (blockIdx.x == 0 && threadIdx.x == 0 && blk->stop == 0) blk->rec[step][CR_A] = A;
  if (blockIdx.x == 0 && threadIdx.x < 4) info[u][threadIdx.x] = 0;
  estep_proj_rows_body(a[u], lda[u], nb[u], mb[u], f[u], r[u], n, nrows, A, sv[u], uv[u]);
}

// Y[i][j] = s_i aL[i][j], zero padded to [nrows][ld] (and, if asked for, the zero-padded copy aLp of aL itself);
// part[slice][j] = sum over the 32 rows of the slice of aL[i][j] u_i (added up slice by slice afterwards: deterministic)
__device__ __forceinline__ void estep_proj_scale_body(const double* __restrict__ aL, int64_t ldal, int nb, int n,
                                                      const double* __restrict__ sv, const double* __restrict__ u,
                                                      double* __restrict__ Y, double* __restrict__ aLp, int64_t ld, int npc,
                                                      double* __restrict__ part) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= npc) return;
  const int i0 = blockIdx.y * 32;
  double acc = 0.0;
#pragma unroll 8
  for (int q = 0; q < 32; ++q) {
    const int i = i0 + q;
    const double v = (i < n && j < nb) ? aL[(int64_t)i * ldal + j] : 0.0;
    Y[(int64_t)i * ld + j] = sv[i] * v;
    if (aLp) aLp[(int64_t)i * ld + j] = v;
    acc += v * u[i];
  }
  part[(int64_t)blockIdx.y * npc + j] = acc;
}
__global__ __launch_bounds__(256) void estep_proj_scale_kernel(const double* __restrict__ aL, int64_t ldal, int nb, int n,
                                                                const double* __restrict__ sv, const double* __restrict__ u,
                                                                double* __restrict__ Y, double* __restrict__ aLp,
                                                                int64_t ld, int npc, double* __restrict__ part) {
  estep_proj_scale_body(aL, ldal, nb, n, sv, u, Y, aLp, ld, npc, part);
}
__global__ __launch_bounds__(256) void estep_proj_scale_group_kernel(PerUnit<const double*> aL, PerUnit<int64_t> ldal,
                                                                      PerUnit<int> nb, int n, PerUnit<double*> sv,
                                                                      PerUnit<double*> uv, PerUnit<double*> Y,
                                                                      PerUnit<double*> aLp, int64_t ld, int npc,
                                                                      PerUnit<double*> part) {
  const int u = blockIdx.z;
  estep_proj_scale_body(aL[u], ldal[u], nb[u], n, sv[u], uv[u], Y[u], aLp[u], ld, npc, part[u]);
}

int launch_estep_proj_rows(const double* a, int64_t lda, int nb, const double* mb, const double* f, const double* r,
                           int n, int nrows, double A, double* sv, double* u, hipStream_t s) {
  hipLaunchKernelGGL(estep_proj_rows_kernel, dim3((nrows + 3) / 4), dim3(256), 0, s, a, lda, nb, mb, f, r, n, nrows, A,
                     sv, u);
  GP_HIP(hipGetLastError());
  return 0;
}
int launch_estep_proj_scale(const double* aL, int64_t ldal, int nb, int n, int nrows, const double* sv, const double* u,
                            double* Y, double* aLp, int64_t ld, int npc, double* part, hipStream_t s) {
  hipLaunchKernelGGL(estep_proj_scale_kernel, dim3((npc + 255) / 256, nrows / 32), dim3(256), 0, s, aL, ldal, nb, n, sv,
                     u, Y, aLp, ld, npc, part);
  GP_HIP(hipGetLastError());
  return 0;
}

// The moments of lambda behind the update, from Z = aL L_W^-T (one wave per training point):
//   lam_m_i = a_i . m_new = Z_i . z1 (z1 = L_W^-1 aL^T u),  lam_var_i = kv0_i + a_i V_new a_i^T = kv0_i + |Z_i|^2
__device__ __forceinline__ void estep_proj_moments_body(const double* __restrict__ Z, int64_t ld, int nb,
                                                       const double* __restrict__ z1, const double* __restrict__ kv0,
                                                       int n, double* __restrict__ lam_m, double* __restrict__ lam_var) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const double* row = Z + (int64_t)i * ld;
  double s0 = 0.0, s1 = 0.0;
  for (int j = lane; j < nb; j += 64) {
    const double v = row[j];
    s0 += v * z1[j];
    s1 += v * v;
  }
  for (int o = 32; o > 0; o >>= 1) {
    s0 += __shfl_down(s0, o);
    s1 += __shfl_down(s1, o);
  }
  if (lane == 0) {
    lam_m[i] = s0;
    lam_var[i] = kv0[i] + s1;
  }
}
__global__ __launch_bounds__(256) void estep_proj_moments_kernel(const double* __restrict__ Z, int64_t ld, int nb,
                                                                  const double* __restrict__ z1,
                                                                  const double* __restrict__ kv0, int n,
                                                                  double* __restrict__ lam_m, double* __restrict__ lam_var) {
  estep_proj_moments_body(Z, ld, nb, z1, kv0, n, lam_m, lam_var);
}
int launch_estep_proj_moments(const double* Z, int64_t ld, int nb, const double* z1, const double* kv0, int n,
                              double* lam_m, double* lam_var, hipStream_t s) {
  hipLaunchKernelGGL(estep_proj_moments_kernel, dim3((n + 3) / 4), dim3(256), 0, s, Z, ld, nb, z1, kv0, n, lam_m, lam_var);
  GP_HIP(hipGetLastError());
  return 0;
}

// ---- the chained E-steps (gpfit_estep_chain, gpfit_estep_chain_batch)
int launch_estep_proj_rows_chain_group(const ChainGroupT& g, int step, hipStream_t s) {
  hipLaunchKernelGGL(estep_proj_rows_chain_group_kernel, dim3((g.nrows + 3) / 4, g.n_units), dim3(256), 0, s, g.a, g.lda, g.nb,
                     g.m, g.f, g.r, g.n, g.nrows, g.blk, g.info, step, g.sv, g.u);
  GP_HIP(hipGetLastError());
  return 0;
}
int launch_estep_proj_scale_group(const ChainGroupT& g, hipStream_t s) {
  hipLaunchKernelGGL(estep_proj_scale_group_kernel, dim3((g.npc + 255) / 256, g.nrows / 32, g.n_units), dim3(256), 0, s, g.aL,
                     g.ldal, g.nb, g.n, g.sv, g.u, g.Y, g.aLp, g.ld, g.npc, g.part);
  GP_HIP(hipGetLastError());
  return 0;
}
// estep_proj_moments_body behind each unit's gate
__global__ __launch_bounds__(256) void estep_proj_moments_chain_group_kernel(PerUnit<ChainBlock*> blk, PerUnit<int*> info,
                                                                              PerUnit<double*> Z, int64_t ld, PerUnit<int> nb,
                                                                              PerUnit<double*> z1, PerUnit<const double*> kv0,
                                                                              int n, PerUnit<double*> lam_m,
                                                                              PerUnit<double*> lam_var) {
  const int u = blockIdx.y;
  const ChainGate g{&blk[u]->stop, info[u]};
  if (!g.open()) return;
  estep_proj_moments_body(Z[u], ld, nb[u], z1[u], kv0[u], n, lam_m[u], lam_var[u]);
}
int launch_estep_proj_moments_chain_group(const ChainGroupT& g, hipStream_t s) {
  hipLaunchKernelGGL(estep_proj_moments_chain_group_kernel, dim3((g.n + 3) / 4, g.n_units), dim3(256), 0, s, g.blk, g.info, g.Zm,
                     g.ld, g.nb, g.z1, g.kv0, g.n, g.lam_m, g.lam_var);
  GP_HIP(hipGetLastError());
  return 0;
}
// The moments behind a damped update (gpfit_estep_chain_damped / _batch), behind each unit's gate, one wave per training
// point: lam_m_i = a_i . m with the committed mean -- a blend, so the full step's Z_i . z1 does not give it -- and
// lam_var_i = kv0_i + |Z_i|^2 with Z = aL L_Wa^-T.  Lane l adds columns l, l + 64, .. and the wave folds in a fixed
// order: the same bits alone and in any group.
__global__ __launch_bounds__(256) void estep_damped_moments_chain_group_kernel(PerUnit<ChainBlock*> blk, PerUnit<int*> info,
                                                                                PerUnit<double*> Z, int64_t ld, PerUnit<int> nb,
                                                                                PerUnit<const double*> a, PerUnit<int64_t> lda,
                                                                                PerUnit<double*> m, PerUnit<const double*> kv0,
                                                                                int n, PerUnit<double*> lam_m,
                                                                                PerUnit<double*> lam_var) {
  const int u = blockIdx.y;
  const ChainGate g{&blk[u]->stop, info[u]};
  if (!g.open()) return;
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const double* __restrict__ zrow = Z[u] + (int64_t)i * ld;
  const double* __restrict__ arow = a[u] + (int64_t)i * lda[u];
  const double* __restrict__ mu = m[u];
  const int k = nb[u];
  double s0 = 0.0, s1 = 0.0;
  for (int j = lane; j < k; j += 64) {
    const double v = zrow[j];
    s0 += arow[j] * mu[j];
    s1 += v * v;
  }
  for (int o = 32; o > 0; o >>= 1) {
    s0 += __shfl_down(s0, o);
    s1 += __shfl_down(s1, o);
  }
  if (lane == 0) {
    lam_m[u][i] = s0;
    lam_var[u][i] = kv0[u][i] + s1;
  }
}
int launch_estep_damped_moments_chain_group(const ChainGroupT& g, hipStream_t s) {
  hipLaunchKernelGGL(estep_damped_moments_chain_group_kernel, dim3((g.n + 3) / 4, g.n_units), dim3(256), 0, s, g.blk, g.info,
                     g.Zm, g.ld, g.nb, g.a, g.lda, g.m, g.kv0, g.n, g.lam_m, g.lam_var);
  GP_HIP(hipGetLastError());
  return 0;
}

}  // namespace gpfit
