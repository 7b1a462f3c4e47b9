// General MFMA GEMM for gfx950 (fp64 and fp32 instances) with per-tile triangular k ranges,
// lower-only output, batching and split-K.  See common.h for the argument contract.
#include "gemm_core.h"

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <set>
#include <utility>

namespace gpfit {

// NS = LDS stages of the main loop (gemm_core.h): 2 everywhere except the "deep" small-tile
// instances (4 at T = 64, 8 at T = 32) the launcher picks when a launch has at most two
// workgroups per CU, i.e. when nothing else hides the load latency.
// Tile selection, k range and main loop of one workgroup: on return acc holds op(A) op(B) of tile (ti, tj) at
// (row0, col0) and C points at this batch / split's output; false when the block has no tile (schedule padding).
template <typename R, bool A_KMAJOR, bool B_KMAJOR, bool EDGE, int T, int NS>
__device__ __forceinline__ bool gemm_tile_compute(const GemmArgsT<R>& p, int tiles_n, int ntiles, R* smem,
                                                  typename Real<R>::acc_t (&acc)[T / 32][T / 32], int& ti, int& tj,
                                                  int& row0, int& col0, R*& C) {
  constexpr int KT = Real<R>::KT;

  // heaviest tiles first: with triangular operands the k range depends on the tile position,
  // so the launcher asks for the walk that starts with the long ones (shorter tail):
  // bit 0 = walk backwards, bit 1 = column-major (gemm_walk_tile, gemm_core.h).
  int slab = 0, slab_tiles = 0;
  const bool slabbed = (T == SLAB_TILE) && p.k_slabs > 0;   // gemm_pick_tile: the route runs on 64-tiles only
  if (slabbed) {
    // triangular-operand route: block = (item, tile column), the item's (panel, slab) from the slab plan
    const SlabPlan sp = slab_plan(p.M, p.k_slabs);
    slab_item(sp, (int)blockIdx.x / tiles_n, ti, slab);
    tj = (int)blockIdx.x % tiles_n;
    slab_tiles = sp.ks;
  } else if (p.sched != nullptr) {
    // XCD-aware schedule: the table says which tile this block id computes (-1: padding entry)
    const int e = p.sched[blockIdx.x];
    if (e < 0) return false;
    ti = e >> 16;
    tj = e & 0xffff;
  } else {
    gemm_walk_tile((int)blockIdx.x, p.reverse, p.out_lower != 0, TILE / T, tiles_n, ntiles, ti, tj);
  }
  row0 = ti * T;
  col0 = tj * T;
  const int b = blockIdx.y, z = blockIdx.z;
  const R* A;
  const R* B;
  if (p.nptr > 0) {
    A = p.Ap[b];
    B = p.Bp[b];
    C = p.Cp[b];
  } else {
    A = p.A + (int64_t)b * p.sA;
    B = p.B + (int64_t)b * p.sB;
    C = p.C + (int64_t)b * p.sC;
  }

  if (p.b_split > 0 && col0 >= p.b_split && p.B2 != nullptr) B = p.B2;   // the triangular part of a split op(B)
  const KRange kr = gemm_tile_k_range(p.a_tri, p.b_tri, p.K, row0, col0, T, p.b_split);
  int kbeg = kr.beg, kend = kr.end;
  // tri bounds are multiples of T >= 32 = the largest K step, so they stay K-step aligned
  if (slabbed) {
    kbeg = max(kbeg, slab * slab_tiles * T);
    kend = min(kend, (slab + 1) * slab_tiles * T);
    C += (int64_t)slab * p.sC;
  } else if (p.split_k > 1) {
    const int steps = max(0, kend - kbeg) / KT;
    const int per = (steps + p.split_k - 1) / p.split_k;
    const int s0 = min(steps, z * per), s1 = min(steps, (z + 1) * per);
    kend = kbeg + s1 * KT;
    kbeg = kbeg + s0 * KT;
    C += (int64_t)z * p.sC;
  }

#pragma unroll
  for (int i = 0; i < T / 32; ++i)
#pragma unroll
    for (int j = 0; j < T / 32; ++j) acc[i][j] = acc_zero<R>();

  // walk bit 2: k downwards (EDGE instances ignore it)
  gemm_mainloop<R, A_KMAJOR, B_KMAJOR, EDGE, T, 0, NS>(A, p.lda, B, p.ldb, p.M, p.N, row0, col0, kbeg, kend, smem, acc,
                                                       (p.reverse & 4) != 0);
  return true;
}

// EPI: fused epilogue compiled into this instance (common.h GemmArgsT::epi; 0 = the plain alpha / beta store).
template <typename R, bool A_KMAJOR, bool B_KMAJOR, bool EDGE, int T, int NS, int EPI = 0>
__device__ __forceinline__ void gemm_tile_body(const GemmArgsT<R>& p, int tiles_n, int ntiles, R* smem) {
  typename Real<R>::acc_t acc[T / 32][T / 32];
  int ti, tj, row0, col0;
  R* C;
  if (!gemm_tile_compute<R, A_KMAJOR, B_KMAJOR, EDGE, T, NS>(p, tiles_n, ntiles, smem, acc, ti, tj, row0, col0, C)) return;

  const R alpha = (R)p.alpha, beta = (p.split_k > 1 || (T == SLAB_TILE && p.k_slabs > 0)) ? (R)0 : (R)p.beta;
  const int64_t ldc = p.ldc;
  const int M = p.M, N = p.N;
  if constexpr (EPI != 0) {
    // fused epilogues (common.h: 1 mirror, 2 tile norms, 4 dual update, 8 added matrix); the launcher has checked that the
    // launch is data-parallel on full tiles
    constexpr int epi = EPI;
    R* __restrict__ D = p.nptr > 0 ? p.auxp[blockIdx.y] : p.aux;
    double* __restrict__ sumsq = p.nptr > 0 ? p.sumsqp[blockIdx.y] : p.sumsq;
    double ss = 0.0;
    for_each_acc<R, T>(acc, row0, col0, [&](int row, int col, R v) {
      if (EDGE && !(row < M && col < N)) return;
      R o = alpha * v;
      R* c = C + (int64_t)row * ldc + col;
      if (epi & 4) {
        R* dd = D + (int64_t)row * ldc + col;
        const R d0 = *dd;
        o += d0;
        *dd = o + d0;
      } else if (epi & 8) {
        o += D[(int64_t)row * ldc + col];
      } else if (beta != (R)0) {
        o += beta * (*c);
      }
      if (epi & 1) {
        // the diagonal tile's strict upper part comes from the transposed store of its lower part
        if (row >= col) *c = o;
        if (row > col) C[(int64_t)col * ldc + row] = o;
      } else {
        *c = o;
      }
      if (epi & 2) ss += (double)o * (double)o;
    });
    if (epi & 2) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) ss += __shfl_down(ss, o);
      double* red = reinterpret_cast<double*>(smem);
      __syncthreads();  // every wave is done with the operand stages
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
      __syncthreads();
      if (threadIdx.x == 0)
        sumsq[p.out_lower ? (int64_t)ti * (ti + 1) / 2 + tj : (int64_t)ti * tiles_n + tj] = (red[0] + red[1]) + (red[2] + red[3]);
    }
    return;
  }
  if (beta == (R)0) {
    for_each_acc<R, T>(acc, row0, col0, [&](int row, int col, R v) {
      if (!EDGE || (row < M && col < N)) C[(int64_t)row * ldc + col] = alpha * v;
    });
  } else {
    for_each_acc<R, T>(acc, row0, col0, [&](int row, int col, R v) {
      if (!EDGE || (row < M && col < N)) {
        R* c = C + (int64_t)row * ldc + col;
        *c = alpha * v + beta * (*c);
      }
    });
  }
}

template <typename R, bool A_KMAJOR, bool B_KMAJOR, bool EDGE, int T, int NS = 2>
__global__ __launch_bounds__(GEMM_THREADS, (T == 128 || NS > 2 ? 2 : 4)) void gemm_mfma_kernel(GemmArgsT<R> p,
                                                                                               int tiles_n,
                                                                                               int ntiles) {
  __shared__ __attribute__((aligned(16))) R smem[2 * NS * Real<R>::KT * T];
  gemm_tile_body<R, A_KMAJOR, B_KMAJOR, EDGE, T, NS>(p, tiles_n, ntiles, smem);
}

// The same 128-tile body under its own name for launches that follow an XCD-aware schedule table
// (gemm_sched.hip): in the fit these are Q = I - T T^T (<R, false, false>) and, where a block of T = L^-1 L_V is
// large enough for a table (<R, false, true>: N = 16384 up, or a unit below the block-form threshold), that block;
// one launch each per evaluation, so a profiler's per-kernel row for this name IS that launch.
#ifdef GPFIT_CLOCK_STAMPS
// Diagnostic build only (scripts/scratch/dev_gemm_clock.sh): shader cycles (s_memtime) and 100 MHz ticks
// (s_memrealtime) each workgroup of the last scheduled launch spent, [B_KMAJOR][block][2]; read back with
// hipMemcpyFromSymbol by gpfit_dev_gemm_clock.  No output value depends on them.
__device__ long long g_gemm_clock[2][4096][2];
#endif

template <typename R, bool A_KMAJOR, bool B_KMAJOR>
__global__ __launch_bounds__(GEMM_THREADS, 2) void gemm_xcd_kernel(GemmArgsT<R> p, int tiles_n, int ntiles) {
  __shared__ __attribute__((aligned(16))) R smem[4 * Real<R>::KT * TILE];
#ifdef GPFIT_CLOCK_STAMPS
  const long long t0 = __builtin_amdgcn_s_memtime(), w0 = __builtin_amdgcn_s_memrealtime();
#endif
  gemm_tile_body<R, A_KMAJOR, B_KMAJOR, false, TILE, 2>(p, tiles_n, ntiles, smem);
#ifdef GPFIT_CLOCK_STAMPS
  if (threadIdx.x == 0 && blockIdx.x < 4096) {
    g_gemm_clock[B_KMAJOR ? 1 : 0][blockIdx.x][0] = (long long)__builtin_amdgcn_s_memtime() - t0;
    g_gemm_clock[B_KMAJOR ? 1 : 0][blockIdx.x][1] = (long long)__builtin_amdgcn_s_memrealtime() - w0;
  }
#endif
}

// The 128-tile body with a fused epilogue (common.h GemmArgsT::epi), with or without a schedule table.
template <typename R, bool A_KMAJOR, bool B_KMAJOR, int EPI>
__global__ __launch_bounds__(GEMM_THREADS, 2) void gemm_epi_kernel(GemmArgsT<R> p, int tiles_n, int ntiles) {
  __shared__ __attribute__((aligned(16))) R smem[4 * Real<R>::KT * TILE];
#ifdef GPFIT_CLOCK_STAMPS
  const long long t0 = __builtin_amdgcn_s_memtime(), w0 = __builtin_amdgcn_s_memrealtime();
#endif
  gemm_tile_body<R, A_KMAJOR, B_KMAJOR, false, TILE, 2, EPI>(p, tiles_n, ntiles, smem);
#ifdef GPFIT_CLOCK_STAMPS
  if (threadIdx.x == 0 && blockIdx.x < 4096 && EPI != 4) {
    g_gemm_clock[B_KMAJOR ? 1 : 0][blockIdx.x][0] = (long long)__builtin_amdgcn_s_memtime() - t0;
    g_gemm_clock[B_KMAJOR ? 1 : 0][blockIdx.x][1] = (long long)__builtin_amdgcn_s_memrealtime() - w0;
  }
#endif
}

// Tile size: 128 when that already gives the chip >= 1.5 waves of blocks, otherwise 64 / 32 so
// the small panels near the leaves of the recursion are not serialised on a handful of CUs.
template <typename R>
int gemm_pick_tile(const GemmArgsT<R>& a) {
  if (a.k_slabs > 0) return SLAB_TILE;   // the slab route's cut is in 64-tiles, whatever the size of the launch
  if (a.tile == 128 || a.tile == 64 || a.tile == 32) return a.tile;
  auto ntiles = [&](int T) {
    const long tm = (a.M + T - 1) / T, tn = (a.N + T - 1) / T;
    const long nb = (a.M + TILE - 1) / TILE;
    return (a.out_lower ? (long)lower_tile_count((int)nb, TILE / T) : tm * tn) * (a.nptr > 0 ? a.nptr : (a.batch > 0 ? a.batch : 1)) *
           (a.split_k > 1 ? a.split_k : 1);
  };
  static const long t128_min = getenv("GPFIT_T128_MIN") ? atol(getenv("GPFIT_T128_MIN")) : 384;
  // pointer batches with triangular operands: the tiles' k ranges differ by up to the matrix size and a batch has
  // no balanced (stream-K / table) schedule, so the 128-tile only pays once the launch runs for several rounds of
  // the chip (measured at 2048-sized blocks, executed TF/s: two problems 37-39 on 128-tiles against 54 on
  // 64-tiles launched one by one; four problems 55)
  static const long t128_tri_min = getenv("GPFIT_T128_TRI_MIN") ? atol(getenv("GPFIT_T128_TRI_MIN")) : 1024;
  const bool batch_tri = a.nptr > 0 && (a.a_tri || a.b_tri);
  if (ntiles(128) >= (batch_tri ? t128_tri_min : t128_min)) return 128;
  static const long t64_min = getenv("GPFIT_T64_MIN") ? atol(getenv("GPFIT_T64_MIN")) : 256;
  static const long t32_dim = getenv("GPFIT_T32_DIM") ? atol(getenv("GPFIT_T32_DIM")) : 1024;
  if (ntiles(64) >= t64_min) return 64;
  return (a.M <= t32_dim && a.N <= t32_dim) ? 32 : 64;
}

constexpr int HALF_OCC_LDS = 17 * 1024;
// a kernel whose static + dynamic LDS exceeds 64 KiB needs the limit raised once per (function, device)
static void allow_dynamic_lds(const void* fn) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  int device = 0;
  (void)hipGetDevice(&device);
  std::lock_guard<std::mutex> lock(mu);
  if (done.insert({fn, device}).second)
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, HALF_OCC_LDS);
}

// Stages of a launch of `blocks` workgroups on full T-tiles: the deep pipeline (4 at T = 64, 8 at T = 32) when the
// launch has at most two workgroups per CU, i.e. when nothing else hides the load latency.
static int gemm_stages(int T, bool edge, long blocks) {
  static const int deep_max = getenv("GPFIT_DEEP_MAX") ? atoi(getenv("GPFIT_DEEP_MAX")) : 512;  // tuning knob
  return (T == TILE || edge || blocks > deep_max) ? 2 : (T == 64 ? 4 : 8);
}

// Stream-K (gemm_streamk.hip) for one problem of `ntiles` whole 128-tiles; two uses:
//  * operands triangular on both sides (k range of a tile ~ distance from the diagonal): pure
//    stream-K over all tiles (+8 % on L^-1 L_V, T T^T, L^-T R);
//  * uniform k range whose tile count leaves a short last round (2080 = 4 x 512 + 32): the full
//    rounds stay data-parallel -- workgroups that start together walk k in lock step and share
//    operand panels in L2, which stream-K's staggered shares give up -- and only the tail tiles
//    are cut along k over the whole chip.
// Returns the number of leading tiles that stay data-parallel (tails of uniform launches); -1: not a stream-K launch.
template <typename R>
static int streamk_first_tile(const GemmArgsT<R>& a, long ntiles) {
  static const bool disabled = getenv("GPFIT_NO_STREAMK") != nullptr;
  if (disabled) return -1;
  static const int sk_min = getenv("GPFIT_SK_MIN_TILES") ? atoi(getenv("GPFIT_SK_MIN_TILES")) : 384;
  if (ntiles < sk_min || (long)a.K < 1024) return -1;  // small launches: latency-, not balance-bound
  // classes of launches that take the stream-K schedule (tuning knob, bit mask): 1 operands
  // triangular on both sides, 2 lower output with an upper-triangular op(A), 4 tails of uniform
  // launches.  Class 2 is off by default: since the LDS-DMA main loop its data-parallel launch
  // (heavy rows first) is the faster one (2.86 vs 3.04 ms at N = 8192).
  static const int sk_classes = getenv("GPFIT_SK_CLASSES") ? atoi(getenv("GPFIT_SK_CLASSES")) : 5;
  const bool cls1 = (a.a_tri != 0 && a.b_tri != 0), cls2 = (a.out_lower && a.a_tri == 2 && a.b_tri == 0);
  if ((cls1 && !(sk_classes & 1)) || (cls2 && !(sk_classes & 2))) return -1;
  if (cls1 || cls2) return 0;
  if (!(sk_classes & 4)) return -1;
  if (a.a_tri || a.b_tri) return -1;       // one-sided triangles: the heavy-first walk already balances
  const int tail = (int)(ntiles % SK_SLOTS);
  if (tail == 0 || tail >= 384 || ntiles < SK_SLOTS) return -1;
  return (int)ntiles - tail;
}

// The route of a launch (common.h): refusals, schedule, epilogue, grid and instance -- decided here and nowhere else.
template <typename R>
GemmRoute gemm_route(const GemmArgsT<R>& a) {
  GemmRoute r{};
  r.sk_first = -1;
  if (a.M <= 0 || a.N <= 0) return r;
  const int T = r.tile = gemm_pick_tile(a);
  auto refuse = [T](const char* why) {
    GemmRoute e{};
    e.rc = -3; e.error = why; e.tile = T; e.sk_first = -1;
    return e;
  };
  const bool strided = a.batch > 1 && a.nptr <= 0;
  r.tiles_n = (a.N + T - 1) / T;
  r.tiles = a.out_lower ? lower_tile_count((a.M + TILE - 1) / TILE, TILE / T) : ((a.M + T - 1) / T) * r.tiles_n;
  r.edge = (a.M % T) || (a.N % T) || (a.out_lower && (a.M % TILE));

  // The schedule.  One problem on whole 128-tiles may take a balanced one: the XCD-aware table when the walk asks
  // for it and there are several rounds of the 512 resident workgroups to balance (below that the stream-K /
  // heavy-first walks win: N = 4096, 528 tiles, 7.27 vs 7.5 ms per fit), else stream-K where it pays.
  if (T == TILE && !r.edge && a.nptr <= 0 && a.batch <= 1 && a.split_k <= 1 && !a.half_occ &&
      (a.tile == 0 || a.tile == TILE)) {
    static const long xcd_min = getenv("GPFIT_XCD_MIN_TILES") ? atol(getenv("GPFIT_XCD_MIN_TILES")) : 1536;
    const long tm = a.M / TILE, tn = a.N / TILE;
    long ntiles = a.out_lower ? tm * (tm + 1) / 2 : tm * tn;
    if (a.b_split > 0) {   // the table of a split op(B) holds the tiles with a k range only
      ntiles = 0;
      for (long ti = 0; ti < tm; ++ti)
        for (long tj = 0; tj < tn; ++tj) {
          const KRange kr = gemm_tile_k_range(a.a_tri, a.b_tri, a.K, (int)ti * TILE, (int)tj * TILE, TILE, a.b_split);
          ntiles += kr.end > kr.beg;
        }
    }
    if ((a.reverse & 8) && !(a.out_lower && a.M != a.N) && tm < 32768 && tn < 32768 && ntiles >= xcd_min) r.sched = GEMM_XCD;
    else if (a.b_split <= 0 && (r.sk_first = streamk_first_tile(a, ntiles)) >= 0) r.sched = GEMM_STREAMK;
  }
  if (a.b_split != 0 && (r.sched != GEMM_XCD || a.b_split < 0 || a.b_split >= a.N || (a.b_split % TILE) || a.b_tri != 1 || a.out_lower))
    return refuse("launch_gemm: a split op(B) needs a lower triangle from a 128-column on and the XCD-aware table (gemm_route says so beforehand)");

  // Fused epilogues: full tiles of one problem or a pointer batch, and the instances that exist (launch_T): 128-tile,
  // row-major A, and per mode the operand layout the fit uses -- the blocks of T = L^-1 L_V with tile norms (lower or
  // full output), Q = -T T^T mirrored, H = Q21 A + Z21 / H = -W22 L21 + Z21 with the dual update.
  // On the stream-K schedule: the tile norms (2) of a square lower output whose tiles ALL take it (T = L^-1 L_V of a
  // unit below the size where the XCD-aware tables take over).  The mirrored store (1) was built for this schedule
  // too and taken out again: the transposed stores of an accumulator tile are 32-byte fragments, which cost Q's
  // launch 50 us and its fix-up 16 at N = 4096 against 28 us for the separate symmetrisation pass (which transposes
  // through LDS).
  if (a.epi) {
    bool ok = a.split_k <= 1 && a.k_slabs <= 0 && !strided && T == TILE && !(a.M % T) && !(a.N % T) && !a.a_kmajor && !a.half_occ;
    if ((a.epi & 1) && (!a.out_lower || a.M != a.N)) ok = false;
    if ((a.epi & 12) && a.nptr <= 0 && a.aux == nullptr) ok = false;
    if (!((a.epi == 2 && a.b_kmajor) || (a.epi == 1 && !a.b_kmajor) || ((a.epi == 4 || a.epi == 8) && a.b_kmajor))) ok = false;
    if (r.sched == GEMM_STREAMK && !(r.sk_first == 0 && a.out_lower && a.M == a.N && a.epi == 2 && a.sumsq != nullptr)) ok = false;
    if (!ok) return refuse("launch_gemm: this launch cannot carry a fused epilogue (gemm_route says so beforehand)");
  }
  // odd M/N are fine for the stores; k-major operands are then read up to one 16-byte chunk past
  // M/N, which internal callers cover with zero padding (the public gpfit_dgemm insists on even).
  constexpr int EPC = 16 / (int)sizeof(R);
  if (a.K % ktile_of<R>() != 0 || (a.lda % EPC) || (a.ldb % EPC))
    return refuse("launch_gemm: K must be a multiple of the K step and lda, ldb multiples of 16 bytes");
  if (a.out_lower && a.M != a.N) return refuse("launch_gemm: out_lower needs a square output");
  if (a.nptr > 0 && (a.nptr > GEMM_MAXB || a.sched || a.split_k > 1))
    return refuse("launch_gemm: a pointer batch holds at most GEMM_MAXB plain problems");
  if (a.k_slabs > 0 &&
      (a.a_tri != 2 || a.b_tri || a.out_lower || a.M != a.K || (a.M % SLAB_TILE) || a.split_k > 1 || a.sched ||
       a.half_occ || strided || (a.tile != 0 && a.tile != SLAB_TILE)))
    return refuse("launch_gemm: k_slabs needs an upper triangular square op(A) on whole 64-tiles and a plain launch");

  r.epi = a.epi;
  if (a.epi & 2) r.sumsq_entries = (r.sched == GEMM_STREAMK ? 33 : 1) * r.tiles;
  // grid and instance of the data-parallel launch
  r.gx = r.sched == GEMM_XCD ? 0 : (r.sched == GEMM_STREAMK ? r.sk_first : r.tiles);
  if (a.k_slabs > 0) {
    const SlabPlan sp = slab_plan(a.M, a.k_slabs);
    r.gx = sp.items * r.tiles_n;
    r.slabs = sp.live;
  }
  r.gy = a.nptr > 0 ? a.nptr : std::max(a.batch, 1);
  r.gz = a.split_k > 1 ? a.split_k : 1;
  r.stages = gemm_stages(T, r.edge, (long)r.gx * r.gy * r.gz);
  // half-occupancy launches (T = 128 only): 64 KiB static + 17 KiB of unused dynamic LDS = 81 KiB > 160 / 2
  r.half = T == TILE && a.half_occ;
  return r;
}
template GemmRoute gemm_route<double>(const GemmArgsT<double>&);
template GemmRoute gemm_route<float>(const GemmArgsT<float>&);

template <typename R, int T>
static void launch_T(const GemmArgsT<R>& p, const GemmRoute& r, hipStream_t s) {
  const int tn = r.tiles_n, tiles = r.tiles;
  const bool edge = r.edge, deep = r.stages > 2, half = r.half;
  dim3 grid(r.gx, r.gy, r.gz);
  dim3 block(GEMM_THREADS);
  constexpr int DEEP = (T == 128) ? 2 : (T == 64 ? 4 : 8);
#define GP_LAUNCH(AK, BK, ED)                                                                          \
  do {                                                                                                 \
    if (deep) hipLaunchKernelGGL((gemm_mfma_kernel<R, AK, BK, ED, T, (ED ? 2 : DEEP)>), grid, block, 0, s, p, tn, tiles); \
    else if (half) {                                                                                   \
      allow_dynamic_lds(reinterpret_cast<const void*>(gemm_mfma_kernel<R, AK, BK, ED, T, 2>));          \
      hipLaunchKernelGGL((gemm_mfma_kernel<R, AK, BK, ED, T, 2>), grid, block, HALF_OCC_LDS, s, p, tn, tiles); \
    } else hipLaunchKernelGGL((gemm_mfma_kernel<R, AK, BK, ED, T, 2>), grid, block, 0, s, p, tn, tiles); \
  } while (0)
  if (r.epi) {
    // the instances gemm_route admits
    if constexpr (T == TILE) {
      const int key = r.epi * 4 + (p.a_kmajor ? 2 : 0) + (p.b_kmajor ? 1 : 0);
      if (key == 2 * 4 + 1) hipLaunchKernelGGL((gemm_epi_kernel<R, false, true, 2>), grid, block, 0, s, p, tn, tiles);
      else if (key == 1 * 4 + 0) hipLaunchKernelGGL((gemm_epi_kernel<R, false, false, 1>), grid, block, 0, s, p, tn, tiles);
      else if (key == 4 * 4 + 1) hipLaunchKernelGGL((gemm_epi_kernel<R, false, true, 4>), grid, block, 0, s, p, tn, tiles);
      else if (key == 8 * 4 + 1) hipLaunchKernelGGL((gemm_epi_kernel<R, false, true, 8>), grid, block, 0, s, p, tn, tiles);
    }
    return;
  }
  if (p.sched && T == TILE && !edge) {
    switch ((p.a_kmajor ? 2 : 0) | (p.b_kmajor ? 1 : 0)) {
      case 0: hipLaunchKernelGGL((gemm_xcd_kernel<R, false, false>), grid, block, 0, s, p, tn, tiles); break;
      case 1: hipLaunchKernelGGL((gemm_xcd_kernel<R, false, true>), grid, block, 0, s, p, tn, tiles); break;
      case 2: hipLaunchKernelGGL((gemm_xcd_kernel<R, true, false>), grid, block, 0, s, p, tn, tiles); break;
      default: hipLaunchKernelGGL((gemm_xcd_kernel<R, true, true>), grid, block, 0, s, p, tn, tiles); break;
    }
    return;
  }
  const int sel = (p.a_kmajor ? 4 : 0) | (p.b_kmajor ? 2 : 0) | (edge ? 1 : 0);
  switch (sel) {
    case 0: GP_LAUNCH(false, false, false); break;
    case 1: GP_LAUNCH(false, false, true); break;
    case 2: GP_LAUNCH(false, true, false); break;
    case 3: GP_LAUNCH(false, true, true); break;
    case 4: GP_LAUNCH(true, false, false); break;
    case 5: GP_LAUNCH(true, false, true); break;
    case 6: GP_LAUNCH(true, true, false); break;
    case 7: GP_LAUNCH(true, true, true); break;
  }
#undef GP_LAUNCH
}

template <typename R>
int launch_gemm(const GemmArgsT<R>& a, const GemmRoute& route, hipStream_t s) {
  if (route.rc != 0) {
    set_error(route.error);
    return route.rc;
  }
  if (route.tile == 0) return 0;
  if (route.sched == GEMM_XCD) return launch_gemm_xcd(a, route, s);        // XCD-aware data-parallel schedule (gemm_sched.hip)
  if (route.sched != GEMM_STREAMK) return launch_gemm_plain(a, route, s);
  const int rc = launch_gemm_streamk(a, route, s);                        // large launches: balanced schedules (gemm_streamk.hip)
  if (rc <= 0) return rc;
  GemmRoute r = route;                                                    // 1: the planner declined
  r.stay_data_parallel();
  return launch_gemm_plain(a, r, s);
}

template <typename R>
int launch_gemm_plain(const GemmArgsT<R>& a, const GemmRoute& r, hipStream_t s) {
  GemmArgsT<R> p = a;
  p.batch = r.gy;
  switch (r.tile) {
    case 128: launch_T<R, 128>(p, r, s); break;
    case 64: launch_T<R, 64>(p, r, s); break;
    default: launch_T<R, 32>(p, r, s); break;
  }
  GP_HIP(hipGetLastError());
  return 0;
}

// ---- two structurally different small-tile pointer batches in one launch (common.h: launch_gemm_pair)
template <typename R>
struct GemmPairT {
  GemmArgsT<R> g[2];
  int tiles[2], tiles_n[2];
};

template <typename R, int T, int NS>
__global__ __launch_bounds__(GEMM_THREADS, (NS > 2 ? 2 : 4)) void gemm_pair_kernel(GemmPairT<R> q) {
  __shared__ __attribute__((aligned(16))) R smem[2 * NS * Real<R>::KT * T];
  const int w = blockIdx.z;
  const GemmArgsT<R>& p = q.g[w];
  if ((int)blockIdx.x >= q.tiles[w] || (int)blockIdx.y >= p.batch) return;
  if (p.b_kmajor) gemm_tile_body<R, false, true, false, T, NS>(p, q.tiles_n[w], q.tiles[w], smem);
  else gemm_tile_body<R, false, false, false, T, NS>(p, q.tiles_n[w], q.tiles[w], smem);
}

// the route a member would take on its own, if that is a plain pointer batch on full 32- or 64-tiles (else tile 0)
template <typename R>
static GemmRoute pair_member_route(const GemmArgsT<R>& a) {
  const GemmRoute none{};
  if (a.nptr <= 0 || a.epi || a.k_slabs > 0 || a.half_occ || a.a_kmajor || (a.M % 64) || (a.N % 64)) return none;
  const GemmRoute r = gemm_route(a);
  return (r.rc == 0 && !r.edge && (r.tile == 32 || r.tile == 64)) ? r : none;
}

template <typename R>
GemmRoute gemm_pair_shape(const GemmArgsT<R>& a, const GemmArgsT<R>& b) {
  static const bool off = getenv("GPFIT_NO_PAIR") != nullptr;   // tuning knob: the two launches on their own
  static const bool no64 = getenv("GPFIT_NO_PAIR64") != nullptr;
  GemmRoute h{};
  h.sk_first = -1;
  const GemmRoute ra = pair_member_route(a), rb = pair_member_route(b);
  if (off || ra.tile == 0 || ra.tile != rb.tile || (no64 && ra.tile == 64)) {
    h.rc = -3;
    h.error = "launch_gemm_pair: the two problems cannot share a launch (gemm_pair_shape says so beforehand)";
    return h;
  }
  h.tile = ra.tile;
  h.tiles = ra.tiles * ra.gy + rb.tiles * rb.gy;
  h.stages = gemm_stages(h.tile, false, h.tiles);
  h.gx = std::max(ra.tiles, rb.tiles);
  h.gy = std::max(ra.gy, rb.gy);
  h.gz = 2;
  return h;
}
template GemmRoute gemm_pair_shape<double>(const GemmArgsT<double>&, const GemmArgsT<double>&);
template GemmRoute gemm_pair_shape<float>(const GemmArgsT<float>&, const GemmArgsT<float>&);

template <typename R>
int launch_gemm_pair(const GemmArgsT<R>& a, const GemmArgsT<R>& b, const GemmRoute& h, hipStream_t s) {
  if (h.rc != 0) {
    set_error(h.error);
    return h.rc;
  }
  static_assert(sizeof(GemmPairT<R>) <= 4096, "kernel arguments are limited to 4 KiB");
  const int T = h.tile;
  GemmPairT<R> q;
  for (int w = 0; w < 2; ++w) {
    q.g[w] = w == 0 ? a : b;
    GemmArgsT<R>& p = q.g[w];
    p.batch = p.nptr;
    q.tiles_n[w] = p.N / T;
    q.tiles[w] = p.out_lower ? lower_tile_count(p.M / TILE, TILE / T) : (p.M / T) * (p.N / T);
  }
  const dim3 grid(h.gx, h.gy, h.gz), block(GEMM_THREADS);
  const bool deep = h.stages > 2;
  if (T == 32 && deep) hipLaunchKernelGGL((gemm_pair_kernel<R, 32, 8>), grid, block, 0, s, q);
  else if (T == 32) hipLaunchKernelGGL((gemm_pair_kernel<R, 32, 2>), grid, block, 0, s, q);
  else if (deep) hipLaunchKernelGGL((gemm_pair_kernel<R, 64, 4>), grid, block, 0, s, q);
  else hipLaunchKernelGGL((gemm_pair_kernel<R, 64, 2>), grid, block, 0, s, q);
  GP_HIP(hipGetLastError());
  return 0;
}
template int launch_gemm_pair<double>(const GemmArgsT<double>&, const GemmArgsT<double>&, const GemmRoute&, hipStream_t);
template int launch_gemm_pair<float>(const GemmArgsT<float>&, const GemmArgsT<float>&, const GemmRoute&, hipStream_t);

template int launch_gemm<double>(const GemmArgsT<double>&, const GemmRoute&, hipStream_t);
template int launch_gemm<float>(const GemmArgsT<float>&, const GemmRoute&, hipStream_t);
template int launch_gemm_plain<double>(const GemmArgsT<double>&, const GemmRoute&, hipStream_t);
template int launch_gemm_plain<float>(const GemmArgsT<float>&, const GemmRoute&, hipStream_t);
template int gemm_pick_tile<double>(const GemmArgsT<double>&);
template int gemm_pick_tile<float>(const GemmArgsT<float>&);

}  // namespace gpfit

#ifdef GPFIT_CLOCK_STAMPS
extern "C" int gpfit_dev_gemm_clock(long long* host_out /* [2][4096][2] */) {
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(gpfit::g_gemm_clock), sizeof(long long) * 2 * 4096 * 2) == hipSuccess ? 0 : -1;
}
#endif
