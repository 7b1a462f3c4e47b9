// The sweeps of a basis rebuild as one device call (gpfit_subspace_sweeps, gpfit_subspace_sweeps_batch): what the
// inner loop of eigtop.top_eigenpairs runs from the host through gpfit_dgemm and gpfit_potrf -- Y = K Q, Y -= sigma Q,
// CholeskyQR -- and the inputs of its Rayleigh-Ritz step, enqueued in one go with one wait at the end.
// Written as a group call: every product is one product(...) on the list of units that still have the step, the
// factorisations of a round are one potrf_lockstep batch on the work matrices of each unit's own context (as one_chain
// in api_solve.hip names them), every small kernel is one launch with the unit on a free grid dimension.  A unit runs
// the same products in the same order whatever else is in the group, each of them the product gpfit_dgemm runs for the
// host loop (same shape, same flags, dense operands), so its Q, Y and S have the bits of the host loop, alone and in
// any group.
// Failure is the only thing decided on the device: the factorisation's info word (INFO_K, never cleared inside a call,
// so it keeps the first failure) and a stop word next to it (INFO_V's slot, which nothing else uses during this call)
// that records the step.  No kernel waits on another: a unit that has failed still takes part in the later launches,
// which only touch its own work matrices and its own Y / W, and the copy that makes steps visible in Q tests the gate.
#include "units.h"
#include "gpfit_mi355x.h"

#include <algorithm>
#include <string>

using namespace gpfit;

static_assert(GPFIT_ESTEP_CHAIN_MAX_UNITS == CHAIN_MAXU, "the header states the units of a group call");

namespace {

constexpr int INFO_SWEEP_STOP = INFO_V;   // the stop word of a unit: 0, or the step (counted from 1) whose factorisation failed

__device__ __forceinline__ ChainGate sweep_gate(const int* info) { return ChainGate{info + INFO_SWEEP_STOP, info + INFO_K}; }

__global__ void sweep_init_kernel(PerUnit<int*> info) {
  if (threadIdx.x < 4) info[blockIdx.x][threadIdx.x] = 0;
}

// Y <- Y - sigma Q over count elements (unit u = blockIdx.y), rounded as the host loop's Y.sub_(Q, alpha=sigma): torch's
// kernel forms y + (-sigma) q as ONE fused multiply-add (measured on the device against both roundings;
// tests/test_gpu_sweep_chain.py pins it)
__global__ __launch_bounds__(256) void sweep_shift_kernel(PerUnit<int*> info, PerUnit<double*> Y, PerUnit<const double*> Q,
                                                          PerUnit<double> sigma, int64_t count) {
  const int u = blockIdx.y;
  if (!sweep_gate(info[u]).open()) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  Y[u][i] = fma(-sigma[u], Q[u][i], Y[u][i]);
}

// the lower tiles of dst [np][ldd] <- (G + G^T) / 2 of the n x n matrix G [n][n], identity on the padding: the host loop's
// symmetrisation and gpfit_potrf's launch_pack_lower in one pass (pack_lower_body's indexing: eight blocks of sixteen rows
// per tile, unit u = blockIdx.z / 8).  (a + b) / 2 is exact and does not depend on the order of a and b, and a diagonal
// entry is (a + a) / 2 = a, so the factorisation reads the bits it reads there.
__global__ __launch_bounds__(256) void sweep_sym_pack_kernel(PerUnit<const double*> G, int n, PerUnit<double*> dst, int64_t ldd) {
  const int tj = blockIdx.x, ti = blockIdx.y;
  if (tj > ti) return;
  const int u = blockIdx.z / (TILE / 16);
  const double* __restrict__ g = G[u];
  const int r0 = ti * TILE + 16 * (int)(blockIdx.z % (TILE / 16)), c0 = tj * TILE;
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int e = threadIdx.x + 256 * it;
    const int i = r0 + (e >> 7), j = c0 + (e & 127);
    double v;
    if (i < n && j < n) v = (g[(int64_t)i * n + j] + g[(int64_t)j * n + i]) / 2.0;
    else v = (i == j) ? 1.0 : 0.0;
    dst[u][(int64_t)i * ldd + j] = v;
  }
}

// behind a factorisation: dst [n][ldd] <- the lower triangle of src, zeros above it (launch_unpack_tri for every unit of
// the list); and one thread per unit lets the stop word take the step at which the info word first became non-zero
__global__ __launch_bounds__(256) void sweep_unpack_tri_kernel(PerUnit<int*> info, int step, PerUnit<const double*> src, int64_t lds,
                                                               int n, PerUnit<double*> dst, int64_t ldd) {
  const int u = blockIdx.z;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    int* w = info[u];
    if (w[INFO_SWEEP_STOP] == 0 && w[INFO_K] != 0) w[INFO_SWEEP_STOP] = step + 1;
  }
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (i >= n || j >= n) return;
  dst[u][(int64_t)i * ldd + j] = (j <= i) ? src[u][(int64_t)i * lds + j] : 0.0;
}

// Q <- the orthonormalised block, behind the gate: where a step becomes visible
__global__ __launch_bounds__(256) void sweep_commit_kernel(PerUnit<int*> info, PerUnit<const double*> src, PerUnit<double*> Q,
                                                           int64_t count) {
  const int u = blockIdx.y;
  if (!sweep_gate(info[u]).open()) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) Q[u][i] = src[u][i];
}

// the four info words of every unit into its context's pinned, device-visible copy
__global__ void sweep_collect_kernel(PerUnit<int*> info, PerUnit<int*> info_host) {
  if (threadIdx.x < 4) info_host[blockIdx.x][threadIdx.x] = info[blockIdx.x][threadIdx.x];
  __threadfence_system();
}

int sweeps_impl(const char* name, gpfit_ctx* const* ctxs, int n_units, void* stream, const double* const* K, int64_t ldk,
                int64_t N, int64_t k, double* const* Q, double* const* Y, double* const* W, double* const* S, const int* m,
                const double* const* sigma, int flags, int* rec_host) {
  const Refuse refuse{name};
  if (n_units < 1 || n_units > CHAIN_MAXU) return refuse("1 .. " + std::to_string(CHAIN_MAXU) + " units per call");
  if (!ctxs || !K || !Q || !Y || !W || !m || !sigma || !rec_host) return refuse("bad argument");
  if (flags & ~(GPFIT_SWEEPS_Y_READY | GPFIT_SWEEPS_WANT_RR)) return refuse("bad argument: unknown flag");
  const bool y_ready = (flags & GPFIT_SWEEPS_Y_READY) != 0, want_rr = (flags & GPFIT_SWEEPS_WANT_RR) != 0;
  if (want_rr && !S) return refuse("bad argument: the Rayleigh-Ritz tail needs S");
  if (N <= 0 || N > INT32_MAX || (N & 15) || k < 16 || k > N || (k & 15) || ldk < N)
    return refuse("bad size (N and k multiples of 16, 16 <= k <= N, ldk >= N)");
  const int np = (int)round_up(k, TILE);
  int mmax = 0;
  for (int u = 0; u < n_units; ++u) {
    const std::string unit = unit_prefix(n_units, u);
    if (!ctxs[u] || !K[u] || !Q[u] || !Y[u] || !W[u] || (want_rr && !S[u])) return refuse(unit + "bad argument: null context or operand");
    if (m[u] < 0 || m[u] > GPFIT_SUBSPACE_SWEEPS_MAX_STEPS)
      return refuse(unit + "m = " + std::to_string(m[u]) + " is not within 0 .. " + std::to_string(GPFIT_SUBSPACE_SWEEPS_MAX_STEPS));
    if (m[u] > 0 && !sigma[u]) return refuse(unit + "bad argument: no shifts");
    if (const char* why = unit_context_refusal(ctxs, u)) return refuse(why);
    if (np > ctxs[u]->np_cap) return refuse(unit + "block larger than the context capacity");
    mmax = std::max(mmax, m[u]);
  }
  DeviceGuard device_guard(ctxs[0]->device);
  hipStream_t s = (hipStream_t)stream;
  const int n = (int)N, kb = (int)k;
  const int64_t ld = np, count = N * k;
  const Lane lane = main_lane(ctxs[0], s);   // every launch on the caller's stream with the leader's workspace
  const dim3 flat((unsigned)((count + 255) / 256));
  const Units everyone = Units::all(ctxs, n_units);
  // Where a unit's block and its product stand is known to the host at every launch.  blk: the block the step starts
  // from, the caller's Q at first; y: K blk, shifted, then the input of a round; the round's output becomes the next y
  // or the next blk.  The caller's Q is only ever written by the gated copy.  With a third work block beside Y and W
  // (the context's Tbuf, where N k elements fit) the block moves from buffer to buffer and is copied into Q once, behind
  // the unit's last step; without it every step ends with that copy.  The copies are exact: the same bits either way.
  double* third[CHAIN_MAXU];
  const double* blk[CHAIN_MAXU];
  double* y[CHAIN_MAXU];
  for (int u = 0; u < n_units; ++u) {
    third[u] = (int64_t)ctxs[u]->np_cap * ctxs[u]->np_cap >= count ? ctxs[u]->Tbuf : nullptr;
    blk[u] = Q[u];
    y[u] = Y[u];
  }
  // a work block of the unit that holds neither a nor b (nullptr: none)
  auto pick = [&](int u, const double* a, const double* b) -> double* {
    double* const work[3] = {Y[u], W[u], third[u]};
    for (double* w : work)
      if (w && w != a && w != b) return w;
    return nullptr;
  };
  // y = K blk                                                           matmul(K, Q)
  auto apply_K = [&](const Units& l) -> int {
    for (int i = 0; i < l.cnt; ++i) y[l.at[i]] = pick(l.at[i], blk[l.at[i]], nullptr);
    return product(lane, {n, kb, n}, 1.0, plain(l.mats(K, ldk)), plain(l.mats(blk, k)), into(l.mats(y, k)));
  };
  // Q <- blk behind the gate, and the block is the caller's Q again
  auto commit = [&](const Units& l) -> int {
    if (!l.cnt) return 0;
    hipLaunchKernelGGL(sweep_commit_kernel, dim3(flat.x, l.cnt), dim3(256), 0, s, l.of(&gpfit_ctx::info), l.from(blk), l.from(Q),
                       count);
    GP_HIP(hipGetLastError());
    for (int i = 0; i < l.cnt; ++i) blk[l.at[i]] = Q[l.at[i]];
    return 0;
  };
  // one round of _cholqr on the units of the list: G = Y^T Y, (G + G^T) / 2, gpfit_potrf's factorisation with the
  // inverse, Y L^-T.  G in Abuf and the dense L^-1 in TmpV, both k x k with leading dimension k as the host loop has them
  auto round = [&](const Units& l, int step) -> int {
    const auto G = &gpfit_ctx::Abuf, Lid = &gpfit_ctx::TmpV;
    GP_TRY(product(lane, {kb, kb, n}, 1.0, trans(l.mats(y, k)), plain(l.mats(y, k)), into(l.mats(G, k))));
    hipLaunchKernelGGL(sweep_sym_pack_kernel, dim3(np / TILE, np / TILE, l.cnt * (TILE / 16)), dim3(256), 0, s, l.cof(G), kb,
                       l.of(&gpfit_ctx::Kbuf), ld);
    GP_HIP(hipGetLastError());
    CholBatchT<double> cb;
    for (int i = 0; i < l.cnt; ++i) add_k_chain(cb, l.ctx[i]);
    cb.ld = ld;
    GP_TRY(potrf_lockstep(cb, 0, np, l.chains(), lane));
    hipLaunchKernelGGL(sweep_unpack_tri_kernel, dim3((kb + 255) / 256, kb, l.cnt), dim3(256), 0, s, l.of(&gpfit_ctx::info), step,
                       l.cof(&gpfit_ctx::Libuf), ld, kb, l.of(Lid), k);
    GP_HIP(hipGetLastError());
    double* out[CHAIN_MAXU];
    for (int i = 0; i < l.cnt; ++i) out[l.at[i]] = pick(l.at[i], blk[l.at[i]], y[l.at[i]]);
    GP_TRY(product(lane, {n, kb, kb}, 1.0, plain(l.mats(y, k)), trans(l.mats(Lid, k)), into(l.mats(out, k))));
    for (int i = 0; i < l.cnt; ++i) y[l.at[i]] = out[l.at[i]];
    return 0;
  };
  hipLaunchKernelGGL(sweep_init_kernel, dim3(n_units), dim3(64), 0, s, everyone.of(&gpfit_ctx::info));
  GP_HIP(hipGetLastError());
  for (int j = 0; j < mmax; ++j) {
    // the units that have step j; those with a shift in it; those for which it is the last; those whose Q is due
    Units act, shifted, last, due;
    for (int u = 0; u < n_units; ++u) {
      if (m[u] <= j) continue;
      act.add(ctxs[u], u);
      if (sigma[u][j] != 0.0) shifted.add(ctxs[u], u);
      if (m[u] == j + 1) last.add(ctxs[u], u);
      if (m[u] == j + 1 || !third[u]) due.add(ctxs[u], u);
    }
    if (!(j == 0 && y_ready)) GP_TRY(apply_K(act));   // (ready: y is the caller's Y, as set above)
    if (shifted.cnt) {
      hipLaunchKernelGGL(sweep_shift_kernel, dim3(flat.x, shifted.cnt), dim3(256), 0, s, shifted.of(&gpfit_ctx::info),
                         shifted.from(y), shifted.from(blk), shifted.table<double>([&](int u) { return sigma[u][j]; }), count);
      GP_HIP(hipGetLastError());
    }
    GP_TRY(round(act, j));
    if (last.cnt) GP_TRY(round(last, j));
    for (int i = 0; i < act.cnt; ++i) blk[act.at[i]] = y[act.at[i]];
    GP_TRY(commit(due));
  }
  if (want_rr) {
    // Y = K Q, S = Q^T Y, S = (S + S^T) / 2: what the Rayleigh-Ritz step and the certificate read
    GP_TRY(product(lane, {n, kb, n}, 1.0, plain(everyone.mats(K, ldk)), plain(everyone.mats(Q, k)), into(everyone.mats(Y, k))));
    GP_TRY(product(lane, {kb, kb, n}, 1.0, trans(everyone.mats(Q, k)), plain(everyone.mats(Y, k)), into(everyone.mats(S, k))));
    GP_TRY(launch_symmetrize_avg_group(n_units, everyone.from(S), k, everyone.same(kb), s));
  }
  hipLaunchKernelGGL(sweep_collect_kernel, dim3(n_units), dim3(64), 0, s, everyone.of(&gpfit_ctx::info),
                     everyone.of(&gpfit_ctx::info_host));
  GP_HIP(hipGetLastError());
  GP_HIP(hipStreamSynchronize(s));
  for (int u = 0; u < n_units; ++u) {
    const int info = ctxs[u]->info_host[INFO_K], stop = ctxs[u]->info_host[INFO_SWEEP_STOP];
    rec_host[2 * u] = info != 0 ? stop : m[u];
    rec_host[2 * u + 1] = info;
  }
  return 0;
}

}  // namespace

extern "C" {

int gpfit_subspace_sweeps_batch(gpfit_ctx* const* ctxs, int n_units, void* stream, const double* const* K, int64_t ldk, int64_t N,
                                int64_t k, double* const* Q, double* const* Y, double* const* W, double* const* S, const int* m,
                                const double* const* sigma, int flags, int* rec_host) {
  return sweeps_impl("gpfit_subspace_sweeps_batch", ctxs, n_units, stream, K, ldk, N, k, Q, Y, W, S, m, sigma, flags, rec_host);
}

int gpfit_subspace_sweeps(gpfit_ctx* ctx, void* stream, const double* K, int64_t ldk, int64_t N, int64_t k, double* Q, double* Y,
                          double* W, double* S, int m, const double* sigma, int flags, int* rec_host) {
  // the group of one (sweeps_impl): a unit's numbers are the same alone and in any group
  return sweeps_impl("gpfit_subspace_sweeps", &ctx, 1, stream, &K, ldk, N, k, &Q, &Y, &W, &S, &m, &sigma, flags, rec_host);
}

}  // extern "C"
