// Active-learning utility U = H(r|x,D) - <H(r|f,x)> for a batch of candidate stimuli
// (reference: nd_utility and its helpers, utils.py:413-525; the Lambert W the reference takes
// from scipy on the host, utils.py:464-466, is evaluated on the device).
// One workgroup per candidate; the threads stride over the response counts r_k; the three sums
// over k are reduced in a fixed order (bit-reproducible): utility_dev.h, shared with select.hip.
#include "common.h"
#include "kernels.h"
#include "utility_dev.h"

namespace gpfit {

// unit u = blockIdx.y of a group scores its own moments into its own output (the single call is the group of one)
__global__ __launch_bounds__(UT_THREADS) void nd_utility_kernel(PerUnit<const double*> sigma2_u, PerUnit<const double*> mu_u,
                                                                const double* __restrict__ r, int nr,
                                                                PerUnit<double*> U_u) {
  const double* __restrict__ sigma2 = sigma2_u[blockIdx.y];
  const double* __restrict__ mu = mu_u[blockIdx.y];
  double* __restrict__ U = U_u[blockIdx.y];
  __shared__ double red[2][UT_THREADS];
  const int i = blockIdx.x;
  const double u = nd_utility_block(sigma2[i], mu[i], r, nr, red);
  if (threadIdx.x == 0) U[i] = u;
}

int launch_nd_utility_group(int n_units, PerUnit<const double*> sigma2, PerUnit<const double*> mu, int64_t nstar,
                            const double* r, int nr, PerUnit<double*> U, hipStream_t s) {
  if (nstar <= 0) return 0;
  hipLaunchKernelGGL(nd_utility_kernel, dim3((unsigned)nstar, n_units), dim3(UT_THREADS), 0, s, sigma2, mu, r, nr, U);
  GP_HIP(hipGetLastError());
  return 0;
}

int launch_nd_utility(const double* sigma2, const double* mu, int64_t nstar, const double* r, int nr, double* U,
                      hipStream_t s) {
  PerUnit<const double*> s2{}, m{};
  PerUnit<double*> out{};
  s2.v[0] = sigma2; m.v[0] = mu; out.v[0] = U;
  return launch_nd_utility_group(1, s2, m, nstar, r, nr, out, s);
}

// ---- the utility of a population: out[i] = sum_u weight[u] U[u][i], the rows in ascending order from the first
// product, one rounding per multiply and per add (the bits of the host loop acc = w[0] U[0]; acc = acc + w[u] U[u]).
// One thread per candidate walks the rows: consecutive threads read consecutive doubles of a row.
__global__ __launch_bounds__(256) void utility_sum_kernel(const double* __restrict__ U, int64_t ldu, int n_rows,
                                                          const double* __restrict__ weight, int64_t P,
                                                          double* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  double acc = weight ? weight[0] * U[i] : U[i];
  for (int u = 1; u < n_rows; ++u) {
    const double v = U[(int64_t)u * ldu + i];
    const double t = weight ? weight[u] * v : v;
    acc = acc + t;
  }
  out[i] = acc;
}

}  // namespace gpfit

using namespace gpfit;

extern "C" int gpfit_nd_utility(void* stream, const double* sigma2, const double* mu, int64_t nstar, const double* r,
                                int nr, double* U) {
  if (!sigma2 || !mu || !r || !U || nstar < 0 || nr <= 0 || nstar > 0x7fffffff) {
    set_error("gpfit_nd_utility: bad argument");
    return -3;
  }
  return launch_nd_utility(sigma2, mu, nstar, r, nr, U, (hipStream_t)stream);
}

extern "C" int gpfit_utility_sum(void* stream, const double* U, int64_t ldu, int n_rows, const double* weight, int64_t P,
                                 double* out) {
  if (!U || !out || n_rows < 1 || P < 0 || ldu < P || (P + 255) / 256 > 0x7fffffff) {
    set_error("gpfit_utility_sum: bad argument");
    return -3;
  }
  if (P == 0) return 0;
  hipLaunchKernelGGL(utility_sum_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, U, ldu, n_rows,
                     weight, P, out);
  GP_HIP(hipGetLastError());
  return 0;
}
