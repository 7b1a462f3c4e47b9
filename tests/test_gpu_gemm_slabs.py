"""The launcher's k_slabs route (csrc/gemm.hip, slab_plan in csrc/common.h): the row of tests/test_gpu_gemm_schedules.py
for the product with an upper triangular op(A) that the gradient pull-back runs (Y = Lambda^T Xm).

The route: 64-tiles whatever the size of the launch, k cut into at most k_slabs fixed slabs of whole tiles, one
workgroup per (row panel, slab, tile column) whose k range is not empty, slab z of a panel written to C + z sC, the
slabs below a panel's own k range neither launched nor written.

 * plan (no GPU): for 1..80 tiles per side and 1..4 slabs the items cover every (panel, k tile) of the triangle exactly
   once, stay inside their slab, and come heavy first.
 * exact leg: integer operands (fp64 uniform in [-8, 8], fp32 {-1, 0, 1}), every slab of every panel equal to the host's
   product over that slab's k range; the never-written slabs, the guard band and the leading-dimension padding still
   NaN; the operand carries NaN in everything its flags say is never read (k < 64 * panel: the tiles of Lambda above
   the diagonal).
 * the route itself (tile, live slabs, workgroups, stages) is asserted before every launch.
 * one problem == the same problem inside a pointer batch, bit for bit, on standard-normal operands; the sum of the
   live slabs in slab order against the derived bound 2 gamma_K (|opA| |opB|) of test_gpu_gemm_schedules.py.
"""
import ctypes

import pytest
import torch

from gaussian_processes_amd import _lib
from gaussian_processes_amd.build import build_library

ST = 64                                # the route's tile
G = 8
NAN = float("nan")
DT = {0: torch.float64, 1: torch.float32}


@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _lib.load()


def query(rows, cols, slabs, **kw):
    M, N = rows, kw.pop("N", cols)
    a = _lib.DevGemmArgs(M=M, N=N, K=M, lda=M, ldb=N, ldc=N, sC=M * N, alpha=1.0, a_kmajor=1, b_kmajor=1, a_tri=2, batch=1,
                         split_k=1, k_slabs=slabs)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def plan_of(lib, a, f32=0):
    need = lib.gpfit_dev_gemm_plan(f32, ctypes.byref(a), 3, None, 0)
    assert need >= 4, need
    buf = (ctypes.c_int32 * need)()
    assert lib.gpfit_dev_gemm_plan(f32, ctypes.byref(a), 3, buf, need) == need
    items, live, kslab, tile = buf[0:4]
    assert need == 4 + 4 * items
    return live, kslab, tile, [tuple(buf[4 + 4 * e: 8 + 4 * e]) for e in range(items)]


def route_of(lib, a, f32=0):
    r = _lib.DevGemmRoute()
    assert lib.gpfit_dev_gemm_route(f32, ctypes.byref(a), None, ctypes.byref(r)) == 0
    return r


# ------------------------------------------------------------------------------------------------ the plan (CPU)
def test_slab_plan_covers_the_triangle_exactly_once(lib):
    for nt in range(1, 81):
        for slabs in (1, 2, 3, 4):
            a = query(ST * nt, 256, slabs)
            live, kslab, tile, items = plan_of(lib, a)
            ks = -(-nt // slabs)
            assert tile == ST and kslab == ks * ST and live == -(-nt // ks) and live <= slabs, (nt, slabs)
            seen = set()
            lens = []
            for ti, z, kb, ke in items:
                assert 0 <= ti < nt and 0 <= z < live, (nt, slabs, ti, z)
                assert kb < ke and kb % ST == 0 and ke % ST == 0, (nt, slabs, ti, z, kb, ke)
                assert kb == max(ti * ST, z * kslab) and ke == min((z + 1) * kslab, nt * ST), (nt, slabs, ti, z, kb, ke)
                for k in range(kb // ST, ke // ST):
                    assert (ti, k) not in seen, f"nt {nt} slabs {slabs}: k tile {k} of panel {ti} twice"
                    seen.add((ti, k))
                lens.append(ke - kb)
            assert seen == {(ti, k) for ti in range(nt) for k in range(ti, nt)}, (nt, slabs)
            # heavy first; when the last slab is a short one (nt not a multiple of ks) its full items may come before
            # longer partial ones, never by more than the slab's deficit
            slack = live * ks - nt
            assert all(lens[i] + slack * ST >= lens[i + 1] for i in range(len(lens) - 1)), (nt, slabs)
            if slack == 0:
                assert lens == sorted(lens, reverse=True), (nt, slabs)
            r = route_of(lib, a)
            assert (r.rc, r.tile, r.slabs, r.blocks, r.xcd, r.sk_first) == (0, ST, live, len(items) * 4, 0, -1), (nt, slabs)
    # the cut is a function of (M, k_slabs): the same plan for N = 32 .. 512, fp32, and a pointer batch
    ref = plan_of(lib, query(2048, 256, 4))
    for kw in ({"N": 32}, {"N": 512}):
        assert plan_of(lib, query(2048, 256, 4, **dict(kw))) == ref
    assert plan_of(lib, query(2048, 256, 4), f32=1) == ref


def test_slab_route_refusals_and_thresholds(lib):
    """What the route needs (an upper triangular square op(A) on whole 64-tiles, a plain launch) and that it stays on
    64-tiles where the automatic choice would be 128 (the headline: 8192 x 256 x 8192) or 32."""
    assert route_of(lib, query(8192, 256, 4)).tile == ST and route_of(lib, query(8192, 256, 0)).tile == 64
    assert route_of(lib, query(8192, 2048, 0)).tile == 128
    assert route_of(lib, query(8192, 2048, 4)).tile == ST
    assert route_of(lib, query(256, 64, 0)).tile == 32 and route_of(lib, query(256, 64, 1)).tile == ST
    r = route_of(lib, query(8192, 256, 4))
    assert (r.slabs, r.stages, r.edge) == (4, 2, 0)
    assert r.blocks == 4 * ((1 + 33 + 65 + 97) + 31 * 4)           # full items per slab + 31 partial steps in each
    assert route_of(lib, query(1024, 256, 2)).stages == 4         # (1 + 9 + 7 * 2) * 4 = 96 workgroups: the deep pipeline
    for bad in ({"a_tri": 0}, {"a_tri": 1}, {"b_tri": 1}, {"out_lower": 1, "N": 2048}, {"K": 1024},
                {"M": 2080, "K": 2080, "lda": 2080}, {"split_k": 2}, {"tile": 128}, {"batch": 2}, {"epi": 2}, {"walk": 16}):
        assert route_of(lib, query(2048, 256, 4, **dict(bad))).rc == -3, bad
    assert lib.gpfit_dev_gemm_plan(0, ctypes.byref(query(2048, 256, 0)), 3, None, 0) == -1


# ------------------------------------------------------------------------------------------------ GPU
def dev():
    return torch.device("cuda:0")


class Problem:
    def __init__(self, M, N, f32, kind, seed):
        g = torch.Generator().manual_seed(4000 + seed)
        if kind == "int":
            lo, hi = (-1, 2) if f32 else (-8, 9)
            a, b = torch.randint(lo, hi, (M, M), generator=g).double(), torch.randint(lo, hi, (M, N), generator=g).double()
        else:
            a, b = torch.randn(M, M, generator=g, dtype=torch.float64), torch.randn(M, N, generator=g, dtype=torch.float64)
            if f32:
                a, b = a.float().double(), b.float().double()
        self.M, self.N, self.f32 = M, N, f32
        self.opA, self.opB = torch.triu(a).to(dev()), b.to(dev())          # op(A)[m][k] = 0 for k < m
        # stored k-major: S[k][m] = op(A)[m][k] (Lambda, lower triangular); never read: k < 64 (m // 64), i.e. the
        # 64-tiles above the diagonal; the upper halves of the diagonal tiles are read and hold zeros
        m = torch.arange(M)[:, None] // ST
        k = torch.arange(M)[None, :]
        a = torch.triu(a)
        a[k < m * ST] = NAN
        lda = M + 8
        sa = torch.full((M, lda), NAN, dtype=DT[f32])
        sa[:, :M] = a.T
        sb = torch.full((M, N + 8), NAN, dtype=DT[f32])
        sb[:, :N] = b
        self.A, self.B = sa.to(dev())[:, :M], sb.to(dev())[:, :N]


def launch_slabs(lib, probs, slabs, want):
    """One launch for the problems of `probs` (a pointer batch when more than one); returns per problem the guard-banded
    buffer [slabs][M + 2G][N + 2G] and asserts the route."""
    p0 = probs[0]
    M, N, f32 = p0.M, p0.N, p0.f32
    ldc = N + 2 * G
    bufs = [torch.full((slabs, M + 2 * G, ldc), NAN, dtype=DT[f32], device=dev()) for _ in probs]
    views = [b[:, G:G + M, G:G + N] for b in bufs]
    a = _lib.DevGemmArgs(A=p0.A.data_ptr(), B=p0.B.data_ptr(), C=views[0].data_ptr(), lda=p0.A.stride(0), ldb=p0.B.stride(0),
                         ldc=ldc, sC=(M + 2 * G) * ldc, M=M, N=N, K=M, alpha=1.0, beta=0.0, a_kmajor=1, b_kmajor=1, a_tri=2,
                         batch=1, split_k=1, k_slabs=slabs)
    keep = []
    if len(probs) > 1:
        a.nptr = len(probs)
        for name, ts in (("Ap", [p.A for p in probs]), ("Bp", [p.B for p in probs]), ("Cp", views)):
            arr = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
            keep.append(arr)
            setattr(a, name, ctypes.cast(arr, ctypes.c_void_p))
    r = route_of(lib, a, f32)
    what = f"M {M} N {N} f32 {f32} slabs {slabs} problems {len(probs)}"
    live, kslab, _, items = plan_of(lib, a, f32)
    tn = -(-N // ST)
    got = {"rc": r.rc, "tile": r.tile, "slabs": r.slabs, "blocks": r.blocks, "edge": r.edge, "xcd": r.xcd, "sk_first": r.sk_first}
    exp = {"rc": 0, "tile": ST, "slabs": live, "blocks": len(items) * tn * len(probs), "edge": int(N % ST != 0), "xcd": 0, "sk_first": -1}
    exp.update(want)
    assert got == exp, what
    rc = lib.gpfit_dev_gemm(torch.cuda.current_stream().cuda_stream, f32, ctypes.byref(a), None)
    torch.cuda.synchronize()
    assert rc == 0, what + ": " + _lib.last_error()
    return bufs, live, kslab


def expected_slabs(p, slabs, live, kslab):
    """[slabs][M + 2G][N + 2G]: slab z of the rows whose panel starts below the slab's end holds op(A)[:, slab] op(B)[slab],
    everything else NaN."""
    M, N = p.M, p.N
    exp = torch.full((slabs, M + 2 * G, N + 2 * G), NAN, dtype=torch.float64, device=dev())
    for z in range(live):
        k0, k1 = z * kslab, min((z + 1) * kslab, M)
        rows = min(M, k1)                                             # panels ti with 64 ti < k1: k1 is a multiple of 64
        exp[z, G:G + rows, G:G + N] = p.opA[:rows, k0:k1] @ p.opB[k0:k1]
    return exp


def same(got, exp):
    return bool(((got.double() == exp) | (got.isnan() & exp.isnan())).all())


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,slabs", [(2048, 256, 4), (1024, 256, 2), (320, 96, 4), (128, 32, 1), (2048, 96, 3), (4096, 128, 4)])
def test_slabs_exact(lib, M, N, slabs):
    assert torch.cuda.is_available()
    for f32 in (0, 1):
        p = Problem(M, N, f32, "int", seed=M + N + f32)
        (buf,), live, kslab = launch_slabs(lib, [p], slabs, {})
        exp = expected_slabs(p, slabs, live, kslab)
        if not same(buf, exp):
            bad = (~((buf.double() == exp) | (buf.isnan() & exp.isnan()))).nonzero()
            z, i, j = (int(v) for v in bad[0])
            panels = sorted({(int(zz), (int(ii) - G) // ST) for zz, ii, _ in bad.tolist()[:100000]})
            raise AssertionError(f"M {M} N {N} f32 {f32} slabs {slabs}: {bad.shape[0]} elements differ; (slab, panel): {panels[:40]}; "
                                 f"first [{z}][{i - G}][{j - G}] got {float(buf[z, i, j])} expected {float(exp[z, i, j])}")
        # the sum of a row's live slabs is the whole product
        tot = torch.zeros(M, N, dtype=torch.float64, device=dev())
        for z in range(live):
            tot += torch.nan_to_num(buf[z, G:G + M, G:G + N].double())
        assert torch.equal(tot, p.opA @ p.opB)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,slabs,nptr", [(1024, 256, 2, 3), (2048, 128, 4, 2), (256, 64, 1, 16), (4096, 256, 4, 4)])
def test_single_problem_equals_pointer_batch(lib, M, N, slabs, nptr):
    """Standard-normal operands: a problem gets the same bits alone and in a batch (which may run another instance:
    the deep pipeline serves launches of at most 512 workgroups), and the slab sum meets the derived bound."""
    for f32 in (0, 1):
        probs = [Problem(M, N, f32, "normal", seed=10 * b + f32) for b in range(nptr)]
        batch, live, kslab = launch_slabs(lib, probs, slabs, {})
        for b in (0, nptr - 1):
            (alone,), _, _ = launch_slabs(lib, [probs[b]], slabs, {})
            assert same(alone, batch[b].double()), f"M {M} N {N} f32 {f32} slabs {slabs}: problem {b} of {nptr} differs from the single launch"
            p = probs[b]
            tot = torch.zeros(M, N, dtype=torch.float64, device=dev())
            first = torch.arange(M, device=dev()) // kslab                      # a row's first live slab
            for z in range(live):
                part = alone[z, G:G + M, G:G + N].double()
                rows = first <= z
                assert bool(part[rows].isfinite().all()) and bool(part[~rows].isnan().all())
                tot[rows] += part[rows]
            ref = p.opA @ p.opB
            absP = p.opA.abs() @ p.opB.abs()
            if f32:
                u, n = 2.0 ** -24, M + 1
                bound = n * u / (1 - n * u) * absP
            else:
                u, n = 2.0 ** -53, M
                bound = 2 * n * u / (1 - n * u) * absP + u * ref.abs()
            worst = float(((tot - ref).abs() / bound.clamp_min(1e-300)).max())
            print(f"M {M} N {N} f32 {f32} slabs {slabs}: worst |C - C_ref| / bound = {worst:.3e}")
            assert bool(((tot - ref).abs() <= bound).all()), worst
