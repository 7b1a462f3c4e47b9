// The projector step of a basis rebuild as one device call (gpfit_sign_steps, gpfit_sign_steps_batch): what the in-place
// branch of eigtop._kept_subspace runs from the host through gpfit_potrf and gpfit_dgemm -- the Cayley transform of the
// k x k Rayleigh quotient matrix and a stretch of the scaled Newton-Schulz sign iteration -- enqueued in one go with one
// wait at the end.
// Written as a group call, like the sweeps (sweeps.hip): every product is one product(...) on the list of units, the
// factorisation of the head is one potrf_lockstep batch on the k-chain of each unit's own context, every small kernel is
// one launch with the unit on a free grid dimension.  The schedule (the scalings, the number of steps, the count the
// symmetrisations go by) is the call's, shared by its units: a pointer-batched product has one alpha.  A unit runs the
// same products in the same order whatever else is in the group, each of them the product gpfit_dgemm runs for the host
// loop (same shape, same flags, dense operands, leading dimension k), so its X and X2 have the bits of the host loop,
// alone and in any group.
// Nothing is decided on the device.  The only failure is the factorisation of S + tau I: its info word (INFO_K, zeroed
// before the first launch and never cleared after it) is read once, at the end.  No kernel waits on another: a unit that
// has failed still takes part in the later launches, which only touch its own work matrices and its own X, X2 and W.
// The norm of X^2 - I, which decides whether the iteration has settled, stays on the host: its summation order is part of
// a fit's bits.
#include "units.h"
#include "gpfit_mi355x.h"

#include <cmath>
#include <string>
#include <utility>

using namespace gpfit;

namespace {

__global__ void sign_init_kernel(PerUnit<int*> info) {
  if (threadIdx.x < 4) info[blockIdx.x][threadIdx.x] = 0;
}

// the lower tiles of dst [np][ldd] <- S + tau I of the n x n matrix S [n][n], identity on the padding: the host loop's
// S + tau * eye and gpfit_potrf's launch_pack_lower in one pass (pack_lower_body's indexing: eight blocks of sixteen rows
// per tile, unit u = blockIdx.z / 8).  The diagonal gets the one rounded add; off it s + 0 is s.
__global__ __launch_bounds__(256) void sign_shift_pack_kernel(PerUnit<const double*> S, int n, PerUnit<double> tau,
                                                              PerUnit<double*> dst, int64_t ldd) {
  const int tj = blockIdx.x, ti = blockIdx.y;
  if (tj > ti) return;
  const int u = blockIdx.z / (TILE / 16);
  const double* __restrict__ g = S[u];
  const double t = tau[u];
  const int r0 = ti * TILE + 16 * (int)(blockIdx.z % (TILE / 16)), c0 = tj * TILE;
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int e = threadIdx.x + 256 * it;
    const int i = r0 + (e >> 7), j = c0 + (e & 127);
    double v;
    if (i < n && j < n) v = g[(int64_t)i * n + j] + (i == j ? t : 0.0);
    else v = (i == j) ? 1.0 : 0.0;
    dst[u][(int64_t)i * ldd + j] = v;
  }
}

// dst [n][n] <- S - tau I (row i = blockIdx.y, unit u = blockIdx.z): the host loop's S - tau * eye
__global__ __launch_bounds__(256) void sign_shift_kernel(PerUnit<const double*> S, int n, PerUnit<double> tau, PerUnit<double*> dst) {
  const int u = blockIdx.z;
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (i >= n || j >= n) return;
  dst[u][(int64_t)i * n + j] = S[u][(int64_t)i * n + j] - (i == j ? tau[u] : 0.0);
}

// behind the factorisation: dst [n][ldd] <- the lower triangle of src, zeros above it (launch_unpack_tri for every unit)
__global__ __launch_bounds__(256) void sign_unpack_tri_kernel(PerUnit<const double*> src, int64_t lds, int n, PerUnit<double*> dst,
                                                              int64_t ldd) {
  const int u = blockIdx.z;
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (i >= n || j >= n) return;
  dst[u][(int64_t)i * ldd + j] = (j <= i) ? src[u][(int64_t)i * lds + j] : 0.0;
}

// dst <- src over count elements (unit u = blockIdx.y): the host loop's X.clone()
__global__ __launch_bounds__(256) void sign_copy_kernel(PerUnit<const double*> src, PerUnit<double*> dst, int64_t count) {
  const int u = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) dst[u][i] = src[u][i];
}

// the four info words of every unit into its context's pinned, device-visible copy
__global__ void sign_collect_kernel(PerUnit<int*> info, PerUnit<int*> info_host) {
  if (threadIdx.x < 4) info_host[blockIdx.x][threadIdx.x] = info[blockIdx.x][threadIdx.x];
  __threadfence_system();
}

int sign_impl(const char* name, gpfit_ctx* const* ctxs, int n_units, void* stream, const double* const* S, int64_t k,
              const double* tau, double* const* X, double* const* X2, double* const* W, int n_steps, const double* c, int its0,
              int flags, int* rec_host) {
  const Refuse refuse{name};
  if (n_units < 1 || n_units > CHAIN_MAXU) return refuse("1 .. " + std::to_string(CHAIN_MAXU) + " units per call");
  if (!ctxs || !X || !X2 || !W || !rec_host) return refuse("bad argument");
  if (flags & ~(GPFIT_SIGN_CAYLEY | GPFIT_SIGN_X2_READY)) return refuse("bad argument: unknown flag");
  const bool cayley = (flags & GPFIT_SIGN_CAYLEY) != 0, x2_ready = (flags & GPFIT_SIGN_X2_READY) != 0;
  if (cayley && x2_ready) return refuse("bad argument: the Cayley head forms X, so no X2 can be ready");
  if (cayley && (!S || !tau)) return refuse("bad argument: the Cayley head needs S and tau");
  if (k < 16 || k > INT32_MAX - TILE || (k & 15)) return refuse("bad size (k a multiple of 16, 16 <= k)");
  if (n_steps < 0 || n_steps > GPFIT_SIGN_MAX_STEPS)
    return refuse("n_steps = " + std::to_string(n_steps) + " is not within 0 .. " + std::to_string(GPFIT_SIGN_MAX_STEPS));
  if (n_steps > 0 && !c) return refuse("bad argument: no scalings");
  if (its0 < 0) return refuse("bad argument: its0 is negative");
  const int np = (int)round_up(k, TILE);
  for (int u = 0; u < n_units; ++u) {
    const std::string unit = unit_prefix(n_units, u);
    if (!ctxs[u] || !X[u] || !X2[u] || !W[u] || (cayley && !S[u])) return refuse(unit + "bad argument: null context or operand");
    if (const char* why = unit_context_refusal(ctxs, u)) return refuse(unit + why);
    if (np > ctxs[u]->np_cap) return refuse(unit + "block larger than the context capacity");
  }
  DeviceGuard device_guard(ctxs[0]->device);
  hipStream_t s = (hipStream_t)stream;
  const int kb = (int)k;
  const int64_t ld = np, count = k * k;
  const Lane lane = main_lane(ctxs[0], s);   // every launch on the caller's stream with the leader's workspace
  const dim3 flat((unsigned)((count + 255) / 256), n_units), rows((kb + 255) / 256, kb, n_units);
  const Units all = Units::all(ctxs, n_units);
  // where a unit's X stands and which of its two blocks is free: they change places with every step
  double* x[CHAIN_MAXU];
  double* spare[CHAIN_MAXU];
  for (int u = 0; u < n_units; ++u) {
    x[u] = X[u];
    spare[u] = W[u];
  }
  auto symmetrise = [&]() -> int { return launch_symmetrize_avg_group(n_units, all.from(x), k, all.same(kb), s); };
  auto square = [&]() -> int {   // X2 = X X                                  matmul(X, X)
    return product(lane, {kb, kb, kb}, 1.0, plain(all.mats(x, k)), plain(all.mats(x, k)), into(all.mats(X2, k)));
  };
  hipLaunchKernelGGL(sign_init_kernel, dim3(n_units), dim3(64), 0, s, all.of(&gpfit_ctx::info));
  GP_HIP(hipGetLastError());
  if (cayley) {
    // S + tau I = L L^T with L^-1 (gpfit_potrf's factorisation), Sinv = L^-T L^-1 in Abuf, the dense L^-1 in TmpV, both
    // k x k with leading dimension k as the host loop has them; X = (S - tau I) Sinv, X = (X + X^T) / 2
    const auto Sinv = &gpfit_ctx::Abuf, Lid = &gpfit_ctx::TmpV;
    const PerUnit<double> taus = all.from(tau);
    hipLaunchKernelGGL(sign_shift_pack_kernel, dim3(np / TILE, np / TILE, n_units * (TILE / 16)), dim3(256), 0, s, all.from(S), kb,
                       taus, all.of(&gpfit_ctx::Kbuf), ld);
    GP_HIP(hipGetLastError());
    CholBatchT<double> cb;
    for (int u = 0; u < n_units; ++u) add_k_chain(cb, ctxs[u]);
    cb.ld = ld;
    GP_TRY(potrf_lockstep(cb, 0, np, all.chains(), lane));
    hipLaunchKernelGGL(sign_unpack_tri_kernel, rows, dim3(256), 0, s, all.cof(&gpfit_ctx::Libuf), ld, kb, all.of(Lid), k);
    GP_HIP(hipGetLastError());
    GP_TRY(product(lane, {kb, kb, kb}, 1.0, trans(all.mats(Lid, k)), plain(all.mats(Lid, k)), into(all.mats(Sinv, k))));
    hipLaunchKernelGGL(sign_shift_kernel, rows, dim3(256), 0, s, all.from(S), kb, taus, all.from(spare));
    GP_HIP(hipGetLastError());
    GP_TRY(product(lane, {kb, kb, kb}, 1.0, plain(all.mats(spare, k)), plain(all.mats(Sinv, k)), into(all.mats(x, k))));
    GP_TRY(symmetrise());
  }
  volatile double three = 3.0;   // (the cube as the host loop's c ** 3 forms it: one call of pow, not two products)
  for (int j = 0; j < n_steps; ++j) {
    if (!(j == 0 && x2_ready)) GP_TRY(square());
    // Xn <- X, Xn = -0.5 c^3 X X2 + 1.5 c Xn as ONE product with a beta, X <- Xn
    PerUnit<const double*> from{};
    for (int u = 0; u < n_units; ++u) from.v[u] = x[u];
    hipLaunchKernelGGL(sign_copy_kernel, flat, dim3(256), 0, s, from, all.from(spare), count);
    GP_HIP(hipGetLastError());
    GP_TRY(product(lane, {kb, kb, kb}, -0.5 * std::pow(c[j], three), plain(all.mats(x, k)), plain(all.mats(X2, k)),
                   into(all.mats(spare, k), 1.5 * c[j])));
    for (int u = 0; u < n_units; ++u) std::swap(x[u], spare[u]);
    if (((its0 + j) & 7) == 7) GP_TRY(symmetrise());
  }
  GP_TRY(square());   // the product the convergence test reads; when it fails, the first product of the next step
  hipLaunchKernelGGL(sign_collect_kernel, dim3(n_units), dim3(64), 0, s, all.of(&gpfit_ctx::info), all.of(&gpfit_ctx::info_host));
  GP_HIP(hipGetLastError());
  GP_HIP(hipStreamSynchronize(s));
  for (int u = 0; u < n_units; ++u) {
    const int info = ctxs[u]->info_host[INFO_K];
    rec_host[2 * u] = info != 0 ? 0 : n_steps;
    rec_host[2 * u + 1] = info;
  }
  return 0;
}

}  // namespace

extern "C" {

int gpfit_sign_steps_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* const* S, int64_t k, const double* tau,
                           double* const* X, double* const* X2, double* const* W, int n_steps, const double* c, int its0, int flags,
                           int* rec_host) {
  return sign_impl("gpfit_sign_steps_batch", ctxs, n_units, stream, S, k, tau, X, X2, W, n_steps, c, its0, flags, rec_host);
}

int gpfit_sign_steps(gpfit_ctx* ctx, void* stream, const double* S, int64_t k, double tau, double* X, double* X2, double* W,
                     int n_steps, const double* c, int its0, int flags, int* rec_host) {
  // the group of one (sign_impl): a unit's numbers are the same alone and in any group
  return sign_impl("gpfit_sign_steps", &ctx, 1, stream, &S, k, &tau, &X, &X2, &W, n_steps, c, its0, flags, rec_host);
}

}  // extern "C"
