// The active-learning utility of ONE candidate, evaluated by one workgroup of UT_THREADS threads: the device code that
// nd_utility_kernel (utility.hip) and the conditioning step of gpfit_select_batch (select.hip) share, so that both give
// the same bits for the same (sigma2, mu).  Internal header; device only.
#pragma once
#include "common.h"

namespace gpfit {

// principal branch, real z >= 0: logarithmic start + Fritsch's quartic iteration on w = ln(z/w)
__device__ __forceinline__ double lambert_w0(double z) {
  if (!(z > 0.0)) return 0.0;
  double w = (z < 2.0) ? z / (1.0 + z) : log(z) - log(log(z));
#pragma unroll 1
  for (int it = 0; it < 6; ++it) {
    const double zn = log(z / w) - w;
    const double q = 2.0 * (1.0 + w) * (1.0 + w + (2.0 / 3.0) * zn);
    const double eps = zn / (1.0 + w) * (q - zn) / (q - 2.0 * zn);
    w = w * (1.0 + eps);
    if (fabs(eps) < 1e-17) break;
  }
  return w;
}

constexpr int UT_THREADS = 128;

// U = H(r|x,D) - <H(r|f,x)> at (s2, m); the threads stride over the response counts r_k and the sums over k are reduced
// in a fixed order.  Every thread of the workgroup calls it (it holds barriers); the value is valid in thread 0 only.
__device__ __forceinline__ double nd_utility_block(double s2, double m, const double* __restrict__ r, int nr,
                                                   double (*red)[UT_THREADS]) {
  double s_plogp = 0.0, s_plrf = 0.0;
  for (int k = threadIdx.x; k < nr; k += UT_THREADS) {
    double rk = r[k];
    double rs = rk * s2;
    double z = exp(rs + m) * s2;                       // utils.py:447
    double lrf = lgamma(rk + 1.0);                     // utils.py:481
    if (z == INFINITY) {                               // utils.py:450-453, 489-490: overflowing terms
      z = 0.0; rs = 0.0; rk = 0.0; lrf = 0.0;
    }
    const double lam = rs + m - lambert_w0(z);         // utils.py:466
    const double e = exp(lam);
    const double dl = lam - m;
    const double logp = lam * rk - e - dl * dl / (2.0 * s2) - 0.5 * log(e * s2 + 1.0) - lrf;  // utils.py:494
    const double p = exp(logp);
    s_plogp += p * logp;
    s_plrf += p * lrf;
  }
  red[0][threadIdx.x] = s_plogp;
  red[1][threadIdx.x] = s_plrf;
  __syncthreads();
  for (int s = UT_THREADS / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  const double H_r = -red[0][0];                                               // utils.py:516
  const double H_mean = -exp(m + 0.5 * s2) * (m + s2 - 1.0) + red[1][0];       // utils.py:428
  return H_r - H_mean;                                                         // utils.py:519
}

}  // namespace gpfit
