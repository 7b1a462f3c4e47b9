// Picking the images of a round one by one, each conditioned on those already chosen (gpfit_select_batch).
// One more presentation of image i adds A^2 f_i a_i a_i^T to the posterior precision (the E-step's Newton term) and, at
// the expected response, leaves the mean where it is: "showing" i is a rank-1 Gaussian conditioning of the latents with
// pseudo-noise tau_i = 1 / (A^2 f_i).  With G the factor rows of the picks so far (a pivoted Cholesky of
// Sigma + diag(tau) restricted to the picks), step t does, per unit,
//   c_j = Sigma[j][i] - sum_{q<t} G[q][j] G[q][i],   G[t][j] = c_j / sqrt(s_i + tau_i),   s_j -= G[t][j]^2.
// A host-enqueued chain of two launches per pick, ordered by the stream alone -- no cooperative launch, no barrier
// between workgroups, no spin-wait, no atomic:
//   select_step_kernel   one workgroup per (candidate, unit): condition s_j on the previous pick, then the utility at the
//                        new s_j (the device code of nd_utility_kernel), left in row t of the unit's work matrix
//   select_pick_kernel   one workgroup: T[j] = sum_u weight[u] U_u[j], the lowest index among the rows of largest finite
//                        T not yet chosen; then sqrt(s_i + tau_i) of every unit into EVERY slot of row t, so that
//                        workgroup j of the next step reads its scalar from the slot that only it overwrites (with
//                        G[t][j]) and nothing is read that another workgroup of the same launch writes
// and one more step launch (no utility) conditions on the last pick: 2 n_select + 1 launches, no host synchronisation.
// An exhausted or non-finite pool is decided on the device: the pick is -1, every later launch returns at once.
#include "kernels.h"
#include "utility_dev.h"
#include "gpfit_mi355x.h"

#include <string>

namespace gpfit {
namespace {

struct SelectArgs {
  PerUnit<const double*> Sigma;   // [M][ldsig]
  PerUnit<int64_t> ldsig;
  PerUnit<const double*> mu;      // [M]
  PerUnit<double*> work;          // [n_select][M]: rows < t hold G, row t the utilities, then the step's scalar
  PerUnit<double*> s2c;           // [M] conditional variances
  PerUnit<double> A, A2, lambda0, weight;
  const double* r;
  int* picked;                    // [n_select]
  double* utility;                // [n_select]
  int nr, n_units, M, has_weight;
};

// step t: condition on pick t - 1 (t > 0), then (with_utility) the utility of step t
__global__ __launch_bounds__(UT_THREADS) void select_step_kernel(SelectArgs p, int t, int with_utility) {
  __shared__ double red[2][UT_THREADS];
  const int j = blockIdx.x, u = blockIdx.y, tid = threadIdx.x;
  const int64_t M = p.M;
  double* __restrict__ work = p.work[u];
  double* __restrict__ s2c = p.s2c[u];
  const double* __restrict__ Sigma = p.Sigma[u];
  const int64_t ld = p.ldsig[u];
  double s;
  if (t == 0) {
    s = Sigma[(int64_t)j * ld + j];
    if (tid == 0) s2c[j] = s;
  } else {
    const int i = p.picked[t - 1];
    if (i < 0) return;   // nothing left to pick: the whole workgroup, before any barrier
    // the dot product over the earlier picks: each thread its q in ascending order, the threads in a fixed tree
    double acc = 0.0;
    for (int q = tid; q < t - 1; q += UT_THREADS) acc += work[q * M + j] * work[q * M + i];
    red[0][tid] = acc;
    __syncthreads();
    for (int h = UT_THREADS / 2; h > 0; h >>= 1) {
      if (tid < h) red[0][tid] += red[0][tid + h];
      __syncthreads();
    }
    if (tid == 0) {
#pragma clang fp contract(off)
      const double sv = work[(t - 1) * M + j];   // sqrt(s_i + tau_i), this workgroup's own copy (select_pick_kernel)
      const double c = Sigma[(int64_t)j * ld + i] - red[0][0];
      const double g = c / sv;
      const double gg = g * g;
      work[(t - 1) * M + j] = g;
      const double sn = s2c[j] - gg;
      s2c[j] = sn;
      red[1][0] = sn;
    }
    __syncthreads();
    s = red[1][0];
    __syncthreads();   // red is reused below
  }
  if (!with_utility) return;
  double s2s, ms;
  {
    // one rounding per operation, as pool_finish_kernel scales the arguments of the utility
#pragma clang fp contract(off)
    const double am = p.A[u] * p.mu[u][j];
    s2s = p.A2[u] * s;
    ms = am + p.lambda0[u];
  }
  const double U = nd_utility_block(s2s, ms, p.r, p.nr, red);
  if (tid == 0) work[t * M + j] = U;
}

constexpr int PICK_THREADS = 256;

__global__ __launch_bounds__(PICK_THREADS) void select_pick_kernel(SelectArgs p, int t) {
  __shared__ double bval[PICK_THREADS];
  __shared__ int bidx[PICK_THREADS];
  __shared__ int chosen[GPFIT_SELECT_MAX];
  __shared__ double sv[CHAIN_MAXU];
  const int tid = threadIdx.x, M = p.M, nu = p.n_units;
  if (t > 0 && p.picked[t - 1] < 0) {   // exhausted at an earlier step
    if (tid == 0) {
      p.picked[t] = -1;
      p.utility[t] = __longlong_as_double(0x7ff8000000000000ll);
    }
    return;
  }
  if (tid < t) chosen[tid] = p.picked[tid];   // t <= GPFIT_SELECT_MAX - 1 < PICK_THREADS
  __syncthreads();
  const int64_t row = (int64_t)t * M;
  double best = 0.0;
  int at = -1;
  for (int j = tid; j < M; j += PICK_THREADS) {
    double acc;
    {
      // the order and the rounding of utility_sum_kernel
#pragma clang fp contract(off)
      const double u0 = p.work[0][row + j];
      acc = p.has_weight ? p.weight[0] * u0 : u0;
      for (int u = 1; u < nu; ++u) {
        const double v = p.work[u][row + j];
        const double w = p.has_weight ? p.weight[u] * v : v;
        acc = acc + w;
      }
    }
    bool free_row = isfinite(acc);
    for (int q = 0; q < t && free_row; ++q) free_row = chosen[q] != j;
    if (free_row && (at < 0 || acc > best)) {   // ascending j: the lowest index of the thread's largest value stays
      best = acc;
      at = j;
    }
  }
  bval[tid] = best;
  bidx[tid] = at;
  __syncthreads();
  for (int h = PICK_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) {
      const double v2 = bval[tid + h];
      const int i2 = bidx[tid + h], i1 = bidx[tid];
      if (i2 >= 0 && (i1 < 0 || v2 > bval[tid] || (v2 == bval[tid] && i2 < i1))) {
        bval[tid] = v2;
        bidx[tid] = i2;
      }
    }
    __syncthreads();
  }
  const int i = bidx[0];
  if (tid == 0) {
    p.picked[t] = i;
    p.utility[t] = i >= 0 ? bval[0] : __longlong_as_double(0x7ff8000000000000ll);
  }
  if (i < 0) return;
  if (tid < nu) {
    const double A = p.A[tid], A2 = p.A2[tid];
    const double s_i = p.s2c[tid][i];
    const double tau = 1.0 / (A2 * exp(A * p.mu[tid][i] + 0.5 * A2 * s_i + p.lambda0[tid]));
    sv[tid] = sqrt(s_i + tau);
  }
  __syncthreads();
  for (int j = tid; j < M; j += PICK_THREADS)   // thread tid read exactly these slots above
    for (int u = 0; u < nu; ++u) p.work[u][row + j] = sv[u];
}

}  // namespace
}  // namespace gpfit

using namespace gpfit;

extern "C" int gpfit_select_batch(void* stream, int n_units, const double* const* Sigma, const int64_t* ldsig, int64_t M,
                                  const double* const* mu, const double* A, const double* lambda0, const double* weight,
                                  const double* r, int nr, int n_select, double* const* work, double* const* sigma2_cond,
                                  int* picked, double* utility) {
  auto refuse = [](const std::string& why) {
    set_error("gpfit_select_batch: " + why);
    return -3;
  };
  if (n_units < 1 || n_units > CHAIN_MAXU) return refuse("1 .. " + std::to_string(CHAIN_MAXU) + " units per call");
  if (n_select < 1 || n_select > GPFIT_SELECT_MAX)
    return refuse("n_select is 1 .. " + std::to_string(GPFIT_SELECT_MAX));
  if (!Sigma || !ldsig || !mu || !A || !lambda0 || !r || nr <= 0 || !work || !sigma2_cond || !picked || !utility || M < 1 ||
      M > 0x7fffffff / GPFIT_SELECT_MAX)
    return refuse("bad argument");
  SelectArgs p{};
  for (int u = 0; u < n_units; ++u) {
    if (!Sigma[u] || !mu[u] || !work[u] || !sigma2_cond[u] || ldsig[u] < M)
      return refuse((n_units > 1 ? "unit " + std::to_string(u) + ": " : std::string()) + "bad argument");
    p.Sigma.v[u] = Sigma[u]; p.ldsig.v[u] = ldsig[u]; p.mu.v[u] = mu[u]; p.work.v[u] = work[u]; p.s2c.v[u] = sigma2_cond[u];
    p.A.v[u] = A[u]; p.A2.v[u] = A[u] * A[u]; p.lambda0.v[u] = lambda0[u]; p.weight.v[u] = weight ? weight[u] : 1.0;
  }
  p.r = r; p.nr = nr; p.picked = picked; p.utility = utility; p.n_units = n_units; p.M = (int)M; p.has_weight = weight != nullptr;
  hipStream_t s = (hipStream_t)stream;
  for (int t = 0; t <= n_select; ++t) {
    const int with_utility = t < n_select;
    hipLaunchKernelGGL(select_step_kernel, dim3((unsigned)M, n_units), dim3(UT_THREADS), 0, s, p, t, with_utility);
    GP_HIP(hipGetLastError());
    if (!with_utility) break;
    hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(PICK_THREADS), 0, s, p, t);
    GP_HIP(hipGetLastError());
  }
  return 0;
}
