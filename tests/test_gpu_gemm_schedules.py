"""The MFMA GEMM launcher against an exact reference, route by route.

Every product of the library goes through launch_gemm (csrc/gemm.hip, gemm_streamk.hip, gemm_sched.hip).  Each case
below is written for ONE route of it and asserts that route through gpfit_dev_gemm_route before it launches, so a
changed threshold fails loudly instead of quietly testing something else.  Method:

 * exact leg -- operands, C0 and aux are integer-valued (fp64: uniform in [-8, 8]; fp32 and every tile-norm case:
   {-1, 0, 1}), alpha in {1, -0.5, 2}, beta in {0, 1, -2}: every partial sum is an integer below 2^53 (fp32: 2^24),
   the product is exact in any summation order and the comparison with the host's fp64 product is equality.  A
   missing, repeated or misplaced tile or k-step cannot hide behind a tolerance; a failure names the tiles.
 * guard bands -- C is a view into a larger buffer filled with a sentinel (NaN for beta = 0, a large odd integer
   otherwise); padding, the 128-blocks above the diagonal of a lower launch and other problems' buffers must come back
   untouched.  Triangular operands carry NaN in the part their flag says is never read, leading dimensions are padded
   with NaN.
 * rounding leg, one per route, standard-normal operands: |C - C_ref| <= 2 gamma_K (|opA| |opB|) |alpha| + u |C_ref|,
   gamma_K = K u / (1 - K u), u = 2^-53 (the factor 2: the host reference carries the same bound); fp32: C_ref is the
   fp64 product of the fp32 values and the bound gamma_(K+1) (|opA| |opB|) |alpha| with u = 2^-24.  Derived, not tuned.
 * the bit-equality claims of the sources' comments.

ROUTES (shapes M x N x K; "lower" = out_lower):
  stream-K, all tiles     3584^3 lower a_tri 1 b_tri 1 (406 tiles); 2560^3 full output a_tri 1 b_tri 2
  stream-K tail, dense    2944 x 2944 x 1024 (529 tiles = 512 + 17)
  stream-K tail, lower    4096 x 4096 x 1024 lower (528 = 512 + 16); walks 2, 3 are the defect this module found
  XCD table               5120 x 5120 x 1024 (1600 tiles); 7168^2 x 1024 lower (1596); 7168^3 lower a_tri 1 b_tri 1
  data-parallel 128       2560 x 2560 x 512 (400 tiles), 2048 x 2560 x 512 forced; 2560^3 a_tri 2; walks 0..7, half-occupancy
  64 / 32 tiles           1024^3, 512^3, 512 x 256 x 2048 (deep pipelines), 2048 x 1280 x 256 (shallow 64); ragged
                          1000 x 616 x 528, 130 x 66 x 16 (edge instances); lower 320^2 x 64 with M % 128 != 0
  split-K                 512 x 512 x 8192 (32 slabs), 8192 x 512 x 8192 (3, uneven), 256 x 256 x 64 (8 slabs, 4 k-steps)
  strided / pointer batch 256^3, 512^3, nptr 1, 2, 7, 32; 2048-sized triangular blocks on both sides of the 128-tile threshold
  pair                    lower SYRK beta = 1 + L21 Li11 (b_tri 1), n 128, 256, 512, tile 32 / 64, shallow and deep
  epilogue 1 mirror       1024 lower, 7168 lower (XCD)
  epilogue 2 tile norms   1024 lower, 1024 x 768 full, 7168 lower (XCD), 3712 lower on stream-K, pointer batch
  epilogue 4 dual update  2048^3 b_tri 1, single and pointer batch
  fp32                    one case of every row
A new route of the launcher comes with a row here.
"""
import ctypes

import pytest
import torch

from gaussian_processes_amd import _lib

pytestmark = pytest.mark.gpu

T = 128
G = 8                                  # guard band around C (elements)
NAN = float("nan")
DT = {0: torch.float64, 1: torch.float32}
SENT = {0: float(2 ** 40 + 1), 1: float(2 ** 23 + 1)}
AB = ((1.0, 0.0), (-0.5, 1.0), (2.0, -2.0))
LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _lib.load()


def dev():
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ operands
class Ops:
    """op(A) [M x K] and op(B) [K x N] of one product: clean fp64 copies on the host for the reference, and per
    storage layout the device operands with NaN in everything the kernel must not read."""

    def __init__(self, M, N, K, at=0, bt=0, kind="int8", f32=0, seed=0, ref_on_device=False):
        g = torch.Generator().manual_seed(1000 + seed)

        def draw(r, c):
            if kind == "int8":
                return torch.randint(-8, 9, (r, c), generator=g).double()
            if kind == "int1":
                return torch.randint(-1, 2, (r, c), generator=g).double()
            x = torch.randn(r, c, generator=g, dtype=torch.float64)
            return x.float().double() if f32 else x

        self.M, self.N, self.K, self.at, self.bt, self.f32 = M, N, K, at, bt, f32
        a, b = draw(M, K), draw(K, N)
        if at == 1: a = torch.tril(a)
        if at == 2: a = torch.triu(a)
        if bt == 1: b = torch.tril(b)
        if bt == 2: b = torch.triu(b)
        self.opA, self.opB = a, b
        self.ref_on_device = ref_on_device
        self._P = self._absP = None
        self._store = {}

    def P(self):
        """opA @ opB in fp64, on the device."""
        if self._P is None:
            if self.ref_on_device:     # exact on integer operands too, and an independent implementation
                self._P = torch.matmul(self.opA.to(dev()), self.opB.to(dev()))
            else:
                self._P = (self.opA @ self.opB).to(dev())
        return self._P

    def absP(self):
        if self._absP is None:
            self._absP = (self.opA.abs() @ self.opB.abs()).to(dev())
        return self._absP

    def stored(self, ak, bk):
        if (ak, bk) not in self._store:
            a, b = self.opA.clone(), self.opB.clone()
            m = torch.arange(self.M)[:, None] // T
            k = torch.arange(self.K)[None, :]
            if self.at == 1: a[k >= (m + 1) * T] = NAN       # tile row m reads k < (m + 1) 128
            if self.at == 2: a[k < m * T] = NAN
            n = torch.arange(self.N)[None, :] // T
            k = torch.arange(self.K)[:, None]
            if self.bt == 1: b[k < n * T] = NAN               # tile column n reads k >= n 128
            if self.bt == 2: b[k >= (n + 1) * T] = NAN
            self._store[(ak, bk)] = (padded(a.T if ak else a, self.f32), padded(b if bk else b.T, self.f32))
        return self._store[(ak, bk)]


def padded(x, f32):
    """x on the device as a view into a buffer whose rows are at least 8 elements longer (the leading dimension a
    multiple of 16 bytes), the padding NaN."""
    r, c = x.shape
    buf = torch.full((r, (c + 8 + 3) // 4 * 4), NAN, dtype=DT[f32])
    buf[:, :c] = x
    return buf.to(dev())[:, :c]


def c_buffer(M, N, beta, f32, seed, kind="int8"):
    """(buffer, view): the guard-banded output.  beta = 0: everything NaN; otherwise integer C0 inside a sentinel frame."""
    if beta == 0:
        buf = torch.full((M + 2 * G, N + 2 * G), NAN, dtype=DT[f32], device=dev())
    else:
        buf = torch.full((M + 2 * G, N + 2 * G), SENT[f32], dtype=DT[f32], device=dev())
        g = torch.Generator().manual_seed(77 + seed)
        lo, hi = (-8, 9) if kind == "int8" else (-1, 2)
        buf[G:G + M, G:G + N] = torch.randint(lo, hi, (M, N), generator=g).to(DT[f32]).to(dev())
    return buf, buf[G:G + M, G:G + N]


def block_lower_mask(M, N):
    i = torch.arange(M, device=dev())[:, None] // T
    j = torch.arange(N, device=dev())[None, :] // T
    return i >= j


def expected(buf, P, alpha, beta, lower, f32):
    """The buffer the launch must leave: alpha P + beta C0 on the written region, everything else as it was."""
    exp = buf.clone()
    M, N = P.shape
    view = exp[G:G + M, G:G + N]
    R = alpha * P if beta == 0 else alpha * P + beta * view.double()
    R = R.to(DT[f32])
    if lower:
        R = torch.where(block_lower_mask(M, N), R, view)
    view.copy_(R)
    return exp


def assert_same(got, exp, what):
    """Equal values (NaN sentinels: still NaN).  A failure names the 128-tiles of the output that differ."""
    ok = (got == exp) | (got.isnan() & exp.isnan())
    if bool(ok.all()):
        return
    bad = (~ok).nonzero()
    inside = bad[((bad >= G) & (bad < torch.tensor(got.shape, device=bad.device) - G)).all(1)] - G
    tiles = sorted({(int(i) // T, int(j) // T) for i, j in inside.tolist()[:200000]})
    i, j = (int(v) for v in bad[0])
    raise AssertionError(f"{what}: {bad.shape[0]} elements differ, {bad.shape[0] - inside.shape[0]} of them in the guard band; "
                         f"{len(tiles)} output tiles (ti, tj) differ: {tiles[:40]}; first: [{i - G}, {j - G}] got {float(got[i, j])} "
                         f"expected {float(exp[i, j])}")


# ------------------------------------------------------------------------------------------------ launching
def gemm_args(A, B, C, M, N, K, alpha=1.0, beta=0.0, ak=0, bk=0, lower=0, at=0, bt=0, walk=0, tile=0, **kw):
    a = _lib.DevGemmArgs(A=A.data_ptr() if A is not None else None, B=B.data_ptr() if B is not None else None,
                         C=C.data_ptr() if C is not None else None, lda=A.stride(0) if A is not None else kw.pop("lda"),
                         ldb=B.stride(0) if B is not None else kw.pop("ldb"), ldc=C.stride(0) if C is not None else kw.pop("ldc"),
                         M=M, N=N, K=K, alpha=alpha, beta=beta, a_kmajor=ak, b_kmajor=bk, out_lower=lower, a_tri=at, b_tri=bt,
                         walk=walk, tile=tile, batch=1, split_k=1)
    keep = []
    for k, v in kw.items():
        if k in ("Ap", "Bp", "Cp", "auxp", "sumsqp"):        # lists of device tensors -> host arrays of device pointers
            arr = (ctypes.c_void_p * len(v))(*[t.data_ptr() for t in v])
            keep.append(arr)
            v = ctypes.cast(arr, ctypes.c_void_p)
        elif isinstance(v, torch.Tensor):
            v = v.data_ptr()
        setattr(a, k, v)
    a._keep = keep
    return a


def route(lib, f32, a, pair=None):
    r = _lib.DevGemmRoute()
    assert lib.gpfit_dev_gemm_route(f32, ctypes.byref(a), ctypes.byref(pair) if pair is not None else None, ctypes.byref(r)) == 0
    return r


def launch(lib, f32, a, pair=None):
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.gpfit_dev_gemm(st, f32, ctypes.byref(a), ctypes.byref(pair) if pair is not None else None)
    torch.cuda.synchronize()
    return rc


def check_route(r, want, what):
    for k, v in want.items():
        got = getattr(r, k)
        if k == "sk_first" and v == "tail":
            assert got > 0, f"{what}: route {k} = {got}, the case was written for a stream-K tail"
        else:
            assert got == v, f"{what}: route {k} = {got}, the case was written for {v}"


def exact_case(lib, ops, want, ak=0, bk=0, lower=0, walk=0, tile=0, ab=AB, seed=0, **kw):
    """One launch per (alpha, beta) of `ab` on integer operands, compared for equality, guard bands included."""
    f32 = ops.f32
    A, B = ops.stored(ak, bk)
    kind = "int8" if float(ops.opA.abs().max()) > 1 else "int1"
    for alpha, beta in ab:
        buf, C = c_buffer(ops.M, ops.N, beta, f32, seed, kind)
        a = gemm_args(A, B, C, ops.M, ops.N, ops.K, alpha, beta, ak, bk, lower, ops.at, ops.bt, walk, tile, **kw)
        what = f"M {ops.M} N {ops.N} K {ops.K} f32 {f32} ak {ak} bk {bk} lower {lower} tri {ops.at}{ops.bt} walk {walk} tile {tile} alpha {alpha} beta {beta}"
        check_route(route(lib, f32, a), {"rc": 0, **want}, what)
        exp = expected(buf, ops.P(), alpha, beta, lower, f32)
        assert launch(lib, f32, a) == 0, what + ": " + _lib.last_error()
        assert_same(buf, exp, what)


def rounding_case(lib, ops, want, ak=0, bk=1, lower=0, walk=0, tile=0, alpha=-0.5, **kw):
    """Standard-normal operands against the derived componentwise bound; returns the output view (for the bit-equality
    claims).  beta = 0: the buffer starts as NaN, so the written region must be complete and the rest untouched."""
    f32 = ops.f32
    A, B = ops.stored(ak, bk)
    buf, C = c_buffer(ops.M, ops.N, 0.0, f32, 0)
    a = gemm_args(A, B, C, ops.M, ops.N, ops.K, alpha, 0.0, ak, bk, lower, ops.at, ops.bt, walk, tile, **kw)
    what = f"rounding: M {ops.M} N {ops.N} K {ops.K} f32 {f32} ak {ak} bk {bk} lower {lower} tri {ops.at}{ops.bt} walk {walk} tile {tile}"
    check_route(route(lib, f32, a), {"rc": 0, **want}, what)
    assert launch(lib, f32, a) == 0, what + ": " + _lib.last_error()
    ref = alpha * ops.P()
    if f32:
        u, n = 2.0 ** -24, ops.K + 1
        bound = n * u / (1 - n * u) * ops.absP() * abs(alpha)
    else:
        u, n = 2.0 ** -53, ops.K
        bound = 2 * n * u / (1 - n * u) * ops.absP() * abs(alpha) + u * ref.abs()
    written = block_lower_mask(ops.M, ops.N) if lower else torch.ones(ops.M, ops.N, dtype=torch.bool, device=dev())
    err = (C.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300))[written].max())     # NaN (a tile left unwritten) compares false below
    print(f"{what}: worst |C - C_ref| / bound = {worst:.3e}")
    assert bool((err <= bound)[written].all()), f"{what}: worst error / bound {worst:.3e}"
    frame = torch.ones_like(buf, dtype=torch.bool)
    frame[G:G + ops.M, G:G + ops.N] = ~written
    assert bool(buf[frame].isnan().all()), what + ": wrote outside its region"
    return C.clone()


# ------------------------------------------------------------------------------------------------ stream-K
def test_streamk_all_tiles(lib):
    want = {"tile": 128, "sk_first": 0, "xcd": 0}
    for f32 in (0, 1):
        ops = Ops(3584, 3584, 3584, 1, 1, "int1" if f32 else "int8", f32, seed=1)     # T = L^-1 L_V: 406 lower tiles
        for n, (ak, bk) in enumerate(LAYOUTS if not f32 else ((0, 1),)):
            for walk in (0, 1, 2, 3):
                exact_case(lib, ops, want, ak, bk, 1, walk, ab=AB if (n, walk) == (1, 0) else (AB[(n + walk) % 3],), seed=walk)
        del ops
    ops = Ops(2560, 2560, 2560, 1, 2, seed=2)                                          # full output, 400 tiles
    for n, (ak, bk) in enumerate(LAYOUTS):
        for walk in (0, 1, 2, 3):
            exact_case(lib, ops, want, ak, bk, 0, walk, ab=(AB[(n + walk + 1) % 3],), seed=walk)
    # rounding (fp64; the fp32 bound is stated for K <= 1024, which no launch of this route has) and reproducibility
    ops = Ops(3584, 3584, 3584, 1, 1, "normal", seed=3)
    c1 = rounding_case(lib, ops, want, lower=1)
    c2 = rounding_case(lib, ops, want, lower=1)
    assert torch.equal(torch.nan_to_num(c1), torch.nan_to_num(c2)), "two runs of a stream-K launch differ"


def test_streamk_tail_dense(lib):
    want = {"tile": 128, "sk_first": 512, "xcd": 0}             # 23 x 23 = 529 tiles: 512 data-parallel, 17 cut along k
    for f32 in (0, 1):
        ops = Ops(2944, 2944, 1024, 0, 0, "int1" if f32 else "int8", f32, seed=4)
        for n, (ak, bk) in enumerate(LAYOUTS if not f32 else ((1, 0),)):
            for walk in (0, 1, 2, 3):
                exact_case(lib, ops, want, ak, bk, 0, walk, ab=AB if n == 0 else (AB[1 + (n + walk) % 2],), seed=walk)
    ops = Ops(2944, 2944, 1024, kind="normal", seed=5)
    c1 = rounding_case(lib, ops, want, walk=2)
    c2 = rounding_case(lib, ops, want, walk=2)
    assert torch.equal(c1, c2), "two runs of a stream-K tail launch differ"
    ops = Ops(2944, 2944, 1024, kind="normal", f32=1, seed=5)
    rounding_case(lib, ops, want)


@pytest.mark.parametrize("walk", [0, 1, 2, 3])
def test_streamk_tail_lower(lib, walk):
    """4096 x 4096 x 1024, lower output: 528 tiles = 512 data-parallel + 16 cut along k.  With the tail enumerated by
    rows whatever the walk, walks 2 and 3 (column-major) left ten tiles unwritten -- walk 2: (27, 27), (28, 27), (28, 28),
    (29, 27) .. (29, 29), (30, 27) .. (30, 30) -- and applied alpha A B twice to ten others."""
    want = {"tile": 128, "sk_first": 512, "xcd": 0}
    ops = Ops(4096, 4096, 1024, seed=6)
    for ak, bk in ((0, 0), (0, 1)):
        exact_case(lib, ops, want, ak, bk, 1, walk, seed=walk)
    if walk == 2:
        exact_case(lib, Ops(4096, 4096, 1024, kind="int1", f32=1, seed=6), want, 0, 0, 1, walk)
        rounding_case(lib, Ops(4096, 4096, 1024, kind="normal", seed=7), want, 0, 0, 1, walk)


# ------------------------------------------------------------------------------------------------ XCD-aware table
def test_xcd_table(lib):
    want = {"tile": 128, "sk_first": -1, "xcd": 1}
    ops = Ops(5120, 5120, 1024, seed=8)                          # 1600 tiles
    for n, (ak, bk) in enumerate(LAYOUTS):
        for walk in (8, 9, 12):
            exact_case(lib, ops, want, ak, bk, 0, walk, ab=(AB[(n + walk) % 3],), seed=walk)
    check_route(route(lib, 0, gemm_args(*ops.stored(0, 0), None, 5120, 5120, 1024, ldc=5120)), {"xcd": 0}, "walk bit 3 off")
    del ops
    ops = Ops(7168, 7168, 1024, seed=9)                          # lower: 1596 tiles (Q = I - T T^T)
    for walk, (ak, bk) in ((8, (0, 0)), (9, (0, 1)), (12, (1, 0)), (9, (1, 1))):
        exact_case(lib, ops, want, ak, bk, 1, walk, ab=AB if ak == bk == 0 else (AB[1],), seed=walk)
    del ops
    exact_case(lib, Ops(7168, 7168, 1024, kind="int1", f32=1, seed=9), want, 0, 0, 1, 9, ab=(AB[2],))
    rounding_case(lib, Ops(7168, 7168, 1024, kind="normal", seed=10), want, 0, 0, 1, 9)
    ops = Ops(7168, 7168, 7168, 1, 1, seed=11, ref_on_device=True)    # a block of T = L^-1 L_V large enough for a table
    for walk, (ak, bk) in ((8, (0, 1)), (12, (0, 0))):
        exact_case(lib, ops, want, ak, bk, 1, walk, ab=(AB[1],), seed=walk)


# ------------------------------------------------------------------------------------------------ data-parallel
def test_data_parallel_128(lib):
    want = {"tile": 128, "sk_first": -1, "xcd": 0, "stages": 2, "edge": 0, "half_occ": 0}
    ops = Ops(2560, 2560, 512, seed=12)                          # 400 tiles: 128-tiles by the launcher's own choice
    for walk in range(8):
        exact_case(lib, ops, want, walk & 1, (walk >> 1) & 1, 0, walk, ab=(AB[walk % 3],), seed=walk)
    exact_case(lib, ops, {**want, "half_occ": 1}, 0, 1, 0, 16 | 1)
    ops = Ops(2048, 2560, 512, seed=13)                          # 320 tiles: forced
    for walk in range(8):
        exact_case(lib, ops, want, 0, walk & 1, 0, walk, tile=128, ab=(AB[(walk + 1) % 3],), seed=walk)
    exact_case(lib, ops, {**want, "half_occ": 1}, 1, 1, 0, 16, tile=128)
    exact_case(lib, Ops(2048, 2560, 512, kind="int1", f32=1, seed=13), want, 0, 1, 0, 3, tile=128)
    ops = Ops(2560, 2560, 2560, 2, 0, seed=14)                   # one-sided triangle: heavy-first walks, no stream-K
    for walk in range(8):
        exact_case(lib, ops, want, 0, 1, 0, walk, ab=(AB[walk % 3],), seed=walk)
    for walk in (0, 3, 6):
        exact_case(lib, ops, want, 1, 0, 1, walk, tile=128, ab=(AB[1],), seed=walk)   # lower output (210 tiles: forced)
    opn = Ops(2048, 2560, 512, kind="normal", seed=15)
    c = rounding_case(lib, opn, want, tile=128)
    h = rounding_case(lib, opn, {**want, "half_occ": 1}, tile=128, walk=16)
    assert torch.equal(c, h), "half-occupancy launch != normal launch"
    rounding_case(lib, Ops(2048, 2560, 512, kind="normal", f32=1, seed=15), want, tile=128)


def test_small_tiles_shallow_deep_and_edge(lib):
    base = {"sk_first": -1, "xcd": 0}
    # (M, N, K), forced tile -> (tile, stages): the deep pipelines run when the launch has at most 512 workgroups
    table = (((1024, 1024, 1024), 0, (64, 4)), ((1024, 1024, 1024), 32, (32, 2)), ((1024, 1024, 1024), 128, (128, 2)),
             ((512, 512, 512), 0, (32, 8)), ((512, 512, 512), 64, (64, 4)), ((512, 512, 512), 128, (128, 2)),
             ((512, 256, 2048), 0, (32, 8)), ((512, 256, 2048), 64, (64, 4)), ((2048, 1280, 256), 0, (64, 2)),
             ((2048, 1280, 256), 32, (32, 2)))
    cache = {}
    for f32 in (0, 1):
        for shape, tile, (t, st) in table:
            if f32 and tile:
                continue
            key = (shape, f32)
            if key not in cache:
                cache[key] = Ops(*shape, kind="int1" if f32 else "int8", f32=f32, seed=16)
            for n, (ak, bk) in enumerate(LAYOUTS):
                for walk in ((0, 5) if n % 2 else (3, 6)):
                    exact_case(lib, cache[key], {**base, "tile": t, "stages": st, "edge": 0}, ak, bk, 0, walk, tile,
                               ab=(AB[(n + walk) % 3],), seed=walk)
    # lower outputs on the small tiles, triangular operands included (deep or shallow is the launcher's business here)
    for n_ in (512, 1024):
        for at, bt in ((0, 0), (1, 1), (2, 0), (0, 2), (1, 2)):
            ops = Ops(n_, n_, n_, at, bt, seed=17)
            for tile in (0, 32, 64, 128):
                exact_case(lib, ops, {**base, **({"tile": tile} if tile else {})}, tile // 64 % 2, 1 - at // 2, 1, tile // 32 % 4,
                           tile, ab=(AB[(at + bt) % 3],), seed=tile)
    # ragged shapes: the predicated instances (k upwards only), every forced tile
    for f32, shapes in ((0, ((1000, 616, 528), (130, 66, 16))), (1, ((1000, 616, 544), (130, 66, 32)))):
        for shape in shapes:
            ops = Ops(*shape, kind="int1" if f32 else "int8", f32=f32, seed=18)
            for tile in (0, 32, 64, 128):
                for n, (ak, bk) in enumerate(LAYOUTS):
                    exact_case(lib, ops, {**base, "edge": 1, "stages": 2, **({"tile": tile} if tile else {})}, ak, bk, 0, n, tile,
                               ab=(AB[(n + tile // 32) % 3],), seed=n)
    # lower output whose side is not a multiple of 128: the last block row is ragged
    ops = Ops(320, 320, 64, seed=19)
    for tile in (0, 32, 64, 128):
        exact_case(lib, ops, {**base, "edge": 1}, 0, 1, 1, 0, tile, seed=tile)
    # rounding, and the claim that the block tile does not change the bits (k upwards, data-parallel, full tiles)
    for f32 in (0, 1):
        ops = Ops(1024, 768, 512, kind="normal", f32=f32, seed=20)
        c = [rounding_case(lib, ops, {**base, "tile": t, "edge": 0}, tile=t) for t in (32, 64, 128)]
        assert torch.equal(c[0], c[1]) and torch.equal(c[1], c[2]), f"forced tiles 32 / 64 / 128 differ (f32 {f32})"
        ops = Ops(512, 512, 512, 1, 2, kind="normal", f32=f32, seed=21)
        c = [rounding_case(lib, ops, {**base, "tile": t}, lower=1, tile=t) for t in (32, 64, 128)]
        assert torch.equal(torch.nan_to_num(c[0]), torch.nan_to_num(c[1])) and torch.equal(torch.nan_to_num(c[1]), torch.nan_to_num(c[2]))


# ------------------------------------------------------------------------------------------------ split-K
def splitk_for(M, N, K):
    """The slabs the truncated / sparse closures ask for: about one and a half rounds of 128-tile workgroups, each with a
    k range of at least 256.  A COPY of the file-static splitk_for of csrc/fit.hip: it must follow that function, the
    slab counts asserted below (32 and 3) are what it gives for the closures' two shapes today."""
    tiles = -(-M // T) * -(-N // T)
    if tiles >= 384:
        return 1
    return max(1, min(-(-768 // tiles), max(1, K // 256)))


def test_split_k(lib):
    for (M, N, K), splits, f32 in (((512, 512, 8192), splitk_for(512, 512, 8192), 0), ((8192, 512, 8192), splitk_for(8192, 512, 8192), 0),
                                   ((256, 256, 64), 8, 0), ((512, 512, 8192), 5, 1), ((256, 256, 64), 8, 1)):
        assert (M, splits) in ((512, 32), (8192, 3), (256, 8), (512, 5))
        ops = Ops(M, N, K, kind="int1" if f32 else "int8", f32=f32, seed=22)
        for (ak, bk), tile, alpha in (((0, 1), 128, 1.0), ((1, 1), 128, -0.5), ((0, 0), 0, 2.0)):
            A, B = ops.stored(ak, bk)
            buf = torch.full((splits, M + 2 * G, N + 2 * G), NAN, dtype=DT[f32], device=dev())
            a = gemm_args(A, B, buf[0, G:G + M, G:G + N], M, N, K, alpha, -2.0, ak, bk, tile=tile, split_k=splits,
                          sC=(M + 2 * G) * (N + 2 * G))
            what = f"split-K {M} x {N} x {K} splits {splits} ak {ak} bk {bk} tile {tile} f32 {f32}"
            r = route(lib, f32, a)
            check_route(r, {"rc": 0, "sk_first": -1, "xcd": 0, **({"tile": 128} if tile else {})}, what)
            assert r.blocks % splits == 0
            assert launch(lib, f32, a) == 0, what
            total = torch.zeros(M, N, dtype=torch.float64, device=dev())
            for z in range(splits):                                  # slab order; beta is ignored
                total += buf[z, G:G + M, G:G + N].double()
            exp = torch.full((M + 2 * G, N + 2 * G), NAN, dtype=torch.float64, device=dev())
            exp[G:G + M, G:G + N] = alpha * ops.P()
            got = torch.full_like(exp, NAN)
            got[G:G + M, G:G + N] = total
            assert_same(got, exp, what)
            frame = torch.ones_like(buf, dtype=torch.bool)
            frame[:, G:G + M, G:G + N] = False
            assert bool(buf[frame].isnan().all()), what + ": wrote outside the slabs"
            steps = K // (32 if f32 else 16)
            per = -(-steps // splits)
            for z in range(splits):                                  # slabs past the last k-step hold zeros
                if z * per >= steps:
                    assert bool((buf[z, G:G + M, G:G + N] == 0).all()), (what, z)
    ops = Ops(8192, 512, 8192, kind="normal", seed=23)
    A, B = ops.stored(0, 1)
    buf = torch.full((3, 8192 + 2 * G, 512 + 2 * G), NAN, dtype=torch.float64, device=dev())
    a = gemm_args(A, B, buf[0, G:-G, G:-G], 8192, 512, 8192, 1.0, 0.0, 0, 1, tile=128, split_k=3, sC=buf.stride(0))
    check_route(route(lib, 0, a), {"rc": 0, "tile": 128, "sk_first": -1}, "split-K rounding")
    assert launch(lib, 0, a) == 0
    C = (buf[0, G:-G, G:-G] + buf[1, G:-G, G:-G]) + buf[2, G:-G, G:-G]
    u = 2.0 ** -53
    bound = 2 * 8192 * u / (1 - 8192 * u) * ops.absP() + u * ops.P().abs()
    worst = float(((C - ops.P()).abs() / bound).max())
    print(f"split-K rounding: worst |C - C_ref| / bound = {worst:.3e}")
    assert bool(((C - ops.P()).abs() <= bound).all()), worst


# ------------------------------------------------------------------------------------------------ batches
def batch_problems(n, M, N, K, at, bt, kind, f32, seed):
    return [Ops(M, N, K, at, bt, kind, f32, seed=seed + 31 * b) for b in range(n)]


def run_pointer_batch(lib, probs, want, ak, bk, lower, walk, tile, alpha, beta, single_too=False, **kw):
    """A pointer batch over separately allocated buffers; every problem against its own reference.  Returns the outputs."""
    p0 = probs[0]
    f32 = p0.f32
    st = [p.stored(ak, bk) for p in probs]
    kind = "int8" if float(p0.opA.abs().max()) > 1 else "int1"
    bufs = [c_buffer(p0.M, p0.N, beta, f32, 5 + b, kind) for b in range(len(probs))]
    a = gemm_args(None, None, None, p0.M, p0.N, p0.K, alpha, beta, ak, bk, lower, p0.at, p0.bt, walk, tile,
                  lda=st[0][0].stride(0), ldb=st[0][1].stride(0), ldc=bufs[0][1].stride(0), nptr=len(probs),
                  Ap=[s[0] for s in st], Bp=[s[1] for s in st], Cp=[b[1] for b in bufs], **kw)
    what = f"pointer batch of {len(probs)}: M {p0.M} N {p0.N} K {p0.K} f32 {f32} ak {ak} bk {bk} lower {lower} tri {p0.at}{p0.bt} walk {walk} tile {tile}"
    check_route(route(lib, f32, a), {"rc": 0, "sk_first": -1, "xcd": 0, **want}, what)
    exps = [expected(buf, p.P(), alpha, beta, lower, f32) for p, (buf, _) in zip(probs, bufs)]
    assert launch(lib, f32, a) == 0, what + ": " + _lib.last_error()
    for b, (exp, (buf, _)) in enumerate(zip(exps, bufs)):
        assert_same(buf, exp, f"{what}, problem {b}")
    return [c for _, c in bufs]


def test_strided_and_pointer_batches(lib):
    # strided batch: three problems in one allocation each for A, B, C
    for f32 in (0, 1):
        M = N = K = 256
        g = torch.Generator().manual_seed(3)
        A = torch.randint(-1, 2, (3, M, K + 8), generator=g).to(DT[f32]).to(dev())
        B = torch.randint(-1, 2, (3, K, N + 8), generator=g).to(DT[f32]).to(dev())
        buf = torch.full((3, M + 2 * G, N + 2 * G), NAN, dtype=DT[f32], device=dev())
        a = gemm_args(A[0, :, :K], B[0, :, :N], buf[0, G:G + M, G:G + N], M, N, K, 2.0, 0.0, 0, 1, batch=3, sA=A.stride(0),
                      sB=B.stride(0), sC=buf.stride(0))
        check_route(route(lib, f32, a), {"rc": 0, "sk_first": -1, "blocks": 3 * 64}, "strided batch")
        assert launch(lib, f32, a) == 0
        exp = torch.full_like(buf, NAN)
        exp[:, G:G + M, G:G + N] = (2.0 * torch.matmul(A[:, :, :K].double().cpu(), B[:, :, :N].double().cpu())).to(DT[f32]).to(dev())
        for z in range(3):
            assert_same(buf[z], exp[z], f"strided batch f32 {f32}, problem {z}")
    # pointer batches, each problem in buffers of its own
    for n_ in (256, 512):
        for nptr in (1, 2, 7, 32):
            for (at, bt, lower), (ak, bk) in (((0, 0, 0), (0, 1)), ((0, 0, 1), (0, 0)), ((0, 2, 0), (0, 0)), ((1, 1, 1), (0, 1)),
                                              ((0, 1, 0), (1, 1))):
                if n_ == 512 and nptr > 7 and (at, bt, lower) != (0, 0, 1):
                    continue
                probs = batch_problems(nptr, n_, n_, n_, at, bt, "int8", 0, seed=40)
                ab = AB[(nptr + at + bt) % 3]
                run_pointer_batch(lib, probs, {}, ak, bk, lower, at % 2, 0, *ab)
    run_pointer_batch(lib, batch_problems(5, 256, 256, 256, 0, 2, "int1", 1, seed=41), {}, 0, 0, 0, 0, 0, -0.5, 1.0)
    run_pointer_batch(lib, batch_problems(33, 128, 128, 16, 0, 0, "int8", 0, seed=42)[:32], {"blocks": 32 * 16}, 0, 1, 0, 0, 0, 1.0, 0.0)
    # 2048-sized triangular blocks: 64-tiles below GPFIT_T128_TRI_MIN = 1024 128-tiles, 128-tiles from there on
    for nptr, tile in ((2, 64), (4, 128)):
        probs = batch_problems(nptr, 2048, 2048, 2048, 0, 1, "int8", 0, seed=43)
        run_pointer_batch(lib, probs, {"tile": tile}, 0, 1, 0, 1, 0, *AB[1])
    probs = batch_problems(2, 2048, 2048, 2048, 0, 0, "int8", 0, seed=44)            # dense: 512 128-tiles >= 384
    run_pointer_batch(lib, probs, {"tile": 128}, 0, 0, 0, 0, 0, *AB[2])
    # a batch gives every problem the bits of its own launch
    for f32 in (0, 1):
        probs = batch_problems(7, 512, 512, 512, 0, 1, "normal", f32, seed=45)
        st = [p.stored(0, 1) for p in probs]
        bufs = [c_buffer(512, 512, 0.0, f32, 0) for _ in probs]
        a = gemm_args(None, None, None, 512, 512, 512, -0.5, 0.0, 0, 1, 0, 0, 1, 1, 0, lda=st[0][0].stride(0), ldb=st[0][1].stride(0),
                      ldc=bufs[0][1].stride(0), nptr=7, Ap=[s[0] for s in st], Bp=[s[1] for s in st], Cp=[b[1] for b in bufs])
        check_route(route(lib, f32, a), {"rc": 0, "sk_first": -1}, "batch of 7")
        assert launch(lib, f32, a) == 0
        for p, (_, c) in zip(probs, bufs):
            single = rounding_case(lib, p, {"sk_first": -1}, 0, 1, 0, 1)
            assert torch.equal(single, c), f"pointer batch != single launch (f32 {f32})"


def pair_members(n, nb2, nb3, kind, f32, seed):
    """The two launches potrf_lockstep shares on its latency-bound levels: A22 -= L21 L21^T (lower, beta = 1) for nb2
    chains and Tmp = L21 Li11 (Li11 lower triangular) for nb3 of them."""
    syrk = batch_problems(nb2, n, n, n, 0, 0, kind, f32, seed)
    merge = batch_problems(nb3, n, n, n, 0, 1, kind, f32, seed + 7)
    return syrk, merge


def pair_args(syrk, merge, bufs2, bufs3, tile):
    n = syrk[0].M
    s2, s3 = [p.stored(0, 0) for p in syrk], [p.stored(0, 1) for p in merge]
    g2 = gemm_args(None, None, None, n, n, n, -1.0, 1.0, 0, 0, 1, 0, 0, 0, tile, lda=s2[0][0].stride(0), ldb=s2[0][1].stride(0),
                   ldc=bufs2[0][1].stride(0), nptr=len(syrk), Ap=[s[0] for s in s2], Bp=[s[1] for s in s2], Cp=[b[1] for b in bufs2])
    g3 = gemm_args(None, None, None, n, n, n, 1.0, 0.0, 0, 1, 0, 0, 1, 1, tile, lda=s3[0][0].stride(0), ldb=s3[0][1].stride(0),
                   ldc=bufs3[0][1].stride(0), nptr=len(merge), Ap=[s[0] for s in s3], Bp=[s[1] for s in s3], Cp=[b[1] for b in bufs3])
    return g2, g3


def test_pair_launch(lib):
    # (n, chains of the SYRK, chains of the merge, forced tile) -> (tile, stages); tiles: lower 32-tiles of n = 128: 16
    table = ((128, 2, 1, 0, (32, 8)), (128, 16, 7, 0, (32, 8)), (256, 4, 2, 0, (32, 8)), (256, 7, 4, 0, (32, 2)),
             (256, 2, 2, 64, (64, 4)), (512, 2, 1, 0, (32, 2)), (512, 2, 1, 64, (64, 4)), (512, 8, 5, 64, (64, 2)))
    for f32 in (0, 1):
        for n, nb2, nb3, tile, (t, st) in table:
            if f32 and (n, nb2) not in ((256, 4), (512, 8)):
                continue
            syrk, merge = pair_members(n, nb2, nb3, "int1" if f32 else "int8", f32, seed=50)
            bufs2 = [c_buffer(n, n, 1.0, f32, 9 + b, "int1" if f32 else "int8") for b in range(nb2)]
            bufs3 = [c_buffer(n, n, 0.0, f32, 0) for _ in range(nb3)]
            g2, g3 = pair_args(syrk, merge, bufs2, bufs3, tile)
            what = f"pair n {n} chains {nb2} + {nb3} tile {tile} f32 {f32}"
            check_route(route(lib, f32, g2, g3), {"rc": 0, "pair": 1, "tile": t, "stages": st}, what)
            exp2 = [expected(buf, p.P(), -1.0, 1.0, 1, f32) for p, (buf, _) in zip(syrk, bufs2)]
            exp3 = [expected(buf, p.P(), 1.0, 0.0, 0, f32) for p, (buf, _) in zip(merge, bufs3)]
            assert launch(lib, f32, g2, g3) == 0, what + ": " + _lib.last_error()
            for b in range(nb2):
                assert_same(bufs2[b][0], exp2[b], f"{what}, SYRK of chain {b}")
            for b in range(nb3):
                assert_same(bufs3[b][0], exp3[b], f"{what}, merge of chain {b}")
    # the pair runs exactly the tile bodies of its two members: same bits as the two launches on their own
    for f32 in (0, 1):
        for n, tile in ((256, 0), (512, 64)):
            syrk, merge = pair_members(n, 3, 2, "normal", f32, seed=51)
            g = torch.Generator().manual_seed(8)
            c0 = [torch.randn(n, n, generator=g, dtype=torch.float64).to(DT[f32]) for _ in syrk]
            outs = []
            for together in (True, False):
                bufs2 = [c_buffer(n, n, 0.0, f32, 0) for _ in syrk]
                for (buf, c), x in zip(bufs2, c0):
                    c.copy_(x.to(dev()))
                bufs3 = [c_buffer(n, n, 0.0, f32, 0) for _ in merge]
                g2, g3 = pair_args(syrk, merge, bufs2, bufs3, tile)
                if together:
                    check_route(route(lib, f32, g2, g3), {"rc": 0, "pair": 1}, "pair bits")
                    assert launch(lib, f32, g2, g3) == 0
                else:
                    assert launch(lib, f32, g2) == 0 and launch(lib, f32, g3) == 0
                outs.append([b[0].clone() for b in bufs2 + bufs3])
            for x, y in zip(*outs):
                assert torch.equal(torch.nan_to_num(x), torch.nan_to_num(y)), f"pair != its members launched singly (n {n} f32 {f32})"
            u, kk = (2.0 ** -24, n + 2) if f32 else (2.0 ** -53, n)     # SYRK: one more rounding for beta C0
            for p, x, c in zip(syrk, c0, outs[0][:3]):
                ref = -p.P() + x.double().to(dev())
                bound = (2 - f32) * kk * u / (1 - kk * u) * (p.absP() + x.double().abs().to(dev())) + u * ref.abs()
                assert bool((((c[G:-G, G:-G].double() - ref).abs() <= bound) | ~block_lower_mask(n, n)).all())
    # members that cannot share a launch are refused
    syrk, merge = pair_members(256, 2, 2, "int8", 0, seed=52)
    bufs2, bufs3 = [c_buffer(256, 256, 1.0, 0, b) for b in range(2)], [c_buffer(256, 256, 0.0, 0, 0) for _ in range(2)]
    g2, g3 = pair_args(syrk, merge, bufs2, bufs3, 0)
    g3.tile = 64
    before = [b[0].clone() for b in bufs2 + bufs3]
    check_route(route(lib, 0, g2, g3), {"rc": -3, "pair": 0}, "mixed tiles")
    assert launch(lib, 0, g2, g3) == -3
    for x, (y, _) in zip(before, bufs2 + bufs3):
        assert_same(y, x, "a refused pair launch wrote something")


# ------------------------------------------------------------------------------------------------ fused epilogues
def test_epilogue_mirror(lib):
    for n_, walk, tile, want, f32 in ((1024, 0, 128, {"xcd": 0}, 0), (1024, 1, 128, {"xcd": 0}, 1), (7168, 9, 0, {"xcd": 1}, 0)):
        ops = Ops(n_, n_, 1024, kind="int1" if f32 else "int8", f32=f32, seed=60)
        A, B = ops.stored(0, 0)
        for alpha, beta in AB:
            buf, C = c_buffer(n_, n_, beta, f32, 1, "int1" if f32 else "int8")
            a = gemm_args(A, B, C, n_, n_, 1024, alpha, beta, 0, 0, 1, walk=walk, tile=tile, epi=1)
            what = f"mirror {n_} f32 {f32} alpha {alpha} beta {beta}"
            check_route(route(lib, f32, a), {"rc": 0, "tile": 128, "sk_first": -1, "epi": 1, **want}, what)
            exp = buf.clone()
            v = exp[G:-G, G:-G]
            R = (alpha * ops.P() if beta == 0 else alpha * ops.P() + beta * v.double()).to(DT[f32])
            v.copy_(torch.tril(R) + torch.tril(R, -1).T)       # the upper triangle = the lower one transposed, diagonal tiles complete
            assert launch(lib, f32, a) == 0, what
            assert_same(buf, exp, what)


def tile_norms(C, lower):
    M, N = C.shape
    s = (C.double() ** 2).reshape(M // T, T, N // T, T).sum(dim=(1, 3))
    if not lower:
        return s.reshape(-1)
    i, j = torch.tril_indices(M // T, M // T)
    out = torch.zeros(len(i), dtype=torch.float64, device=C.device)
    out[(i * (i + 1) // 2 + j).to(C.device)] = s[i.to(C.device), j.to(C.device)]
    return out


def test_epilogue_tile_norms(lib):
    # (M, N, K, lower, a_tri, b_tri, walk, tile) -> route; operands in {-1, 0, 1}, alpha = +-1, beta = 0, K <= 4096
    table = (((1024, 1024, 1024, 1, 0, 0, 0, 128), {"sk_first": -1, "xcd": 0}), ((1024, 768, 512, 0, 0, 0, 2, 128), {"sk_first": -1, "xcd": 0}),
             ((1024, 1024, 1024, 1, 1, 1, 1, 128), {"sk_first": -1, "xcd": 0}), ((7168, 7168, 1024, 1, 0, 0, 9, 0), {"xcd": 1}),
             ((3712, 3712, 3712, 1, 1, 1, 0, 0), {"sk_first": 0, "xcd": 0}))
    for f32 in (0, 1):
        for (M, N, K, lower, at, bt, walk, tile), want in table:
            if f32 and M == 7168:
                continue
            ops = Ops(M, N, K, at, bt, "int1", f32, seed=61)
            A, B = ops.stored(0, 1)
            for alpha in (1.0, -1.0):
                buf, C = c_buffer(M, N, 0.0, f32, 0)
                nt = (M // T) * (M // T + 1) // 2 if lower else (M // T) * (N // T)
                entries = 33 * nt if want.get("sk_first") == 0 else nt
                ss = torch.full((entries + 8,), NAN, dtype=torch.float64, device=dev())
                a = gemm_args(A, B, C, M, N, K, alpha, 0.0, 0, 1, lower, at, bt, walk, tile, epi=2, sumsq=ss)
                what = f"tile norms {M} x {N} x {K} lower {lower} tri {at}{bt} f32 {f32} alpha {alpha}"
                check_route(route(lib, f32, a), {"rc": 0, "tile": 128, "epi": 2, "sumsq_entries": entries, **want}, what)
                exp = expected(buf, ops.P(), alpha, 0.0, lower, f32)
                assert launch(lib, f32, a) == 0, what + ": " + _lib.last_error()
                assert_same(buf, exp, what)
                assert bool(ss[entries:].isnan().all()), what + ": wrote past the table"
                norms = tile_norms(torch.nan_to_num(exp[G:-G, G:-G]), lower)
                if entries == nt:
                    assert torch.equal(ss[:nt], norms), f"{what}: tile norms differ at {(ss[:nt] != norms).nonzero().flatten().tolist()[:20]}"
                else:
                    # stream-K: a whole tile leaves its norm in [idx] and zeros in its 32 band entries; a split tile zero
                    # in [idx] and the norms of its 4-row bands behind the table
                    whole, bands = ss[:nt], ss[nt:entries].reshape(nt, 32)
                    assert torch.equal(whole + bands.sum(1), norms), what
                    assert bool(((whole == 0) | (bands == 0).all(1)).all()), what + ": a tile reported twice"
                    Cx = torch.nan_to_num(exp[G:-G, G:-G]).double()
                    i, j = torch.tril_indices(M // T, M // T)
                    bn = (Cx ** 2).reshape(M // T, 32, 4, M // T, T).sum(dim=(2, 4))[i.to(dev()), :, j.to(dev())]   # [tile][band]
                    idx = (i * (i + 1) // 2 + j).to(dev())
                    split = whole[idx] == 0
                    assert bool(split.any()) and bool((~split).any()), what + ": expected whole and split tiles"
                    assert torch.equal(bands[idx][split], bn[split]), what + ": band norms of the split tiles"
    # pointer batch: per-problem tables
    probs = batch_problems(3, 512, 512, 512, 1, 1, "int1", 0, seed=62)
    tabs = [torch.full((10 + 8,), NAN, dtype=torch.float64, device=dev()) for _ in probs]
    outs = run_pointer_batch(lib, probs, {"tile": 128, "epi": 2, "sumsq_entries": 10}, 0, 1, 1, 0, 128, -1.0, 0.0, epi=2, sumsqp=tabs)
    for c, t in zip(outs, tabs):
        lowc = torch.where(block_lower_mask(512, 512), c, torch.zeros_like(c))
        assert torch.equal(t[:10], tile_norms(lowc, 1)) and bool(t[10:].isnan().all())


def test_epilogue_dual_update(lib):
    # H = alpha A B + D, then aux = H + D (beta ignored): 2048^3 with a lower-triangular op(B), 256 forced 128-tiles
    for f32 in (0, 1):
        kind = "int1" if f32 else "int8"
        for nptr in (0, 2):
            probs = batch_problems(max(nptr, 1), 2048, 2048, 2048, 0, 1, kind, f32, seed=63)
            st = [p.stored(0, 1) for p in probs]
            cb = [c_buffer(2048, 2048, 0.0, f32, 0) for _ in probs]
            db = [c_buffer(2048, 2048, 1.0, f32, 20 + b, kind) for b in range(len(probs))]
            for alpha in (-1.0, 2.0):
                d0 = [d[1].clone() for d in db]
                kw = dict(epi=4)
                if nptr:
                    a = gemm_args(None, None, None, 2048, 2048, 2048, alpha, 5.0, 0, 1, 0, 0, 1, 0, 128, lda=st[0][0].stride(0),
                                  ldb=st[0][1].stride(0), ldc=cb[0][1].stride(0), nptr=nptr, Ap=[s[0] for s in st], Bp=[s[1] for s in st],
                                  Cp=[c[1] for c in cb], auxp=[d[1] for d in db], **kw)
                else:
                    a = gemm_args(st[0][0], st[0][1], cb[0][1], 2048, 2048, 2048, alpha, 5.0, 0, 1, 0, 0, 1, 0, 128, aux=db[0][1], **kw)
                what = f"dual update nptr {nptr} f32 {f32} alpha {alpha}"
                check_route(route(lib, f32, a), {"rc": 0, "tile": 128, "sk_first": -1, "xcd": 0, "epi": 4}, what)
                expc, expd = [], []
                for p, (bufc, _), (bufd, _), d in zip(probs, cb, db, d0):
                    H = (alpha * p.P() + d.double()).to(DT[f32])
                    ec, ed = bufc.clone(), bufd.clone()
                    ec[G:-G, G:-G] = H
                    ed[G:-G, G:-G] = H + d
                    expc.append(ec)
                    expd.append(ed)
                assert launch(lib, f32, a) == 0, what + ": " + _lib.last_error()
                for b in range(len(probs)):
                    assert_same(cb[b][0], expc[b], f"{what}: C of problem {b}")
                    assert_same(db[b][0], expd[b], f"{what}: aux of problem {b}")


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_launches_return_minus_3_and_write_nothing(lib):
    ops = Ops(1024, 1024, 1024, seed=70)
    A, B = ops.stored(0, 1)
    A00, B00 = ops.stored(0, 0)
    ss = torch.full((64,), NAN, dtype=torch.float64, device=dev())
    buf, C = c_buffer(1024, 1024, 1.0, 0, 0)
    before = buf.clone()
    cases = {
        "tile norms on the 64-tiles the launcher picks": gemm_args(A, B, C, 1024, 1024, 1024, 1.0, 0.0, 0, 1, 1, epi=2, sumsq=ss),
        "mirror of a full output": gemm_args(A00, B00, C, 1024, 1024, 1024, 1.0, 0.0, 0, 0, 0, tile=128, epi=1),
        "mirror with a k-major B": gemm_args(A, B, C, 1024, 1024, 1024, 1.0, 0.0, 0, 1, 1, tile=128, epi=1),
        "dual update without aux": gemm_args(A, B, C, 1024, 1024, 1024, 1.0, 0.0, 0, 1, 0, tile=128, epi=4),
        "tile norms under split-K": gemm_args(A, B, C, 1024, 1024, 1024, 1.0, 0.0, 0, 1, 1, tile=128, epi=2, sumsq=ss, split_k=2),
        "tile norms at half occupancy": gemm_args(A, B, C, 1024, 1024, 1024, 1.0, 0.0, 0, 1, 1, walk=16, tile=128, epi=2, sumsq=ss),
        "K not a multiple of the k-step": gemm_args(A, B, C, 1024, 1024, 1000, 1.0, 1.0, 0, 1),
        "odd lda": gemm_args(A, B, C, 1024, 1024, 1024, 1.0, 1.0, 0, 1),
        "lower with M != N": gemm_args(A, B, C, 1024, 896, 1024, 1.0, 1.0, 0, 1, 1),
    }
    for what, a in cases.items():
        if what == "odd lda":
            a.lda = a.lda + 1
        check_route(route(lib, 0, a), {"rc": -3}, what)
        assert launch(lib, 0, a) == -3, what
        assert _lib.last_error(), what
        assert_same(buf, before, what + ": wrote something")
        assert bool(ss.isnan().all()), what
    # a stream-K tail launch cannot carry the tile norms: refused as well
    a = gemm_args(A, B, C, 2944, 2944, 1024, 1.0, 0.0, 0, 1, 0, epi=2, sumsq=ss)
    check_route(route(lib, 0, a), {"rc": -3}, "tile norms on a stream-K tail")
    # 33 problems in a pointer batch
    probs = batch_problems(1, 128, 128, 16, 0, 0, "int8", 0, seed=71)
    sA, sB = probs[0].stored(0, 1)
    b2, c2 = c_buffer(128, 128, 1.0, 0, 0)
    keep = b2.clone()
    a = gemm_args(None, None, None, 128, 128, 16, 1.0, 1.0, 0, 1, lda=sA.stride(0), ldb=sB.stride(0), ldc=c2.stride(0),
                  Ap=[sA] * 33, Bp=[sB] * 33, Cp=[c2] * 33, nptr=33)
    check_route(route(lib, 0, a), {"rc": -3}, "a pointer batch of 33")
    assert launch(lib, 0, a) == -3
    assert_same(b2, keep, "a pointer batch of 33 wrote something")


# ------------------------------------------------------------------------------------------------ caller-owned workspace
def streamk_plan(lib, f32, a):
    need = lib.gpfit_dev_gemm_plan(f32, ctypes.byref(a), 2, None, 0)
    assert need > 0, need
    buf = (ctypes.c_int32 * need)()
    assert lib.gpfit_dev_gemm_plan(f32, ctypes.byref(a), 2, buf, need) == need
    p = list(buf)
    nt, nfix, nslot, ws_slots = p[1], p[5], p[6], p[7]
    return p[8 + 5 * nt + 2 * nfix + 1:][:nslot], ws_slots


def test_streamk_on_a_caller_owned_workspace(lib):
    """sk_ws: the partial tiles of a stream-K launch go to the caller's buffer (as the fit's contexts have it), to the
    slots the plan names and nowhere else."""
    want = {"tile": 128, "sk_first": 512, "xcd": 0}
    for f32 in (0, 1):
        ops = Ops(2944, 2944, 1024, kind="int1" if f32 else "int8", f32=f32, seed=80)
        a = gemm_args(*ops.stored(0, 1), None, 2944, 2944, 1024, ak=0, bk=1, walk=2, ldc=2944 + 2 * G)
        slots, ws_slots = streamk_plan(lib, f32, a)
        assert slots and ws_slots == 1024
        guard, slot = 4096, T * T
        ws = torch.full((2 * guard + ws_slots * slot * (8 // (4 if f32 else 8)),), NAN, dtype=DT[f32], device=dev())
        body = ws[guard:ws.numel() - guard]
        exact_case(lib, ops, want, 0, 1, 0, 2, ab=(AB[1],), sk_ws=body)
        used = ~body[:ws_slots * slot].reshape(ws_slots, slot).isnan().all(1)
        assert sorted(used.nonzero().flatten().tolist()) == sorted(slots), f"f32 {f32}: slots written != the plan's"
        assert bool(body[:ws_slots * slot].reshape(ws_slots, slot)[used].isfinite().all())
        assert bool(ws[:guard].isnan().all()) and bool(ws[ws.numel() - guard:].isnan().all()) and bool(body[ws_slots * slot:].isnan().all())


# ------------------------------------------------------------------------------------------------ epilogues: rounding legs
def gamma(n, u):
    return n * u / (1 - n * u)


def sum_bound(ops, alpha, extra=0, absD=None):
    """Componentwise bound of a result that is a sum of K products (scaled by alpha) and, with absD, of further terms
    of that magnitude, each element rounded K + extra times: gamma_(K + extra) (|alpha| |opA| |opB| + absD); fp64: twice
    that (the host reference carries the same bound) + u of the magnitude; fp32: gamma_(K + 1 + extra), u = 2^-24."""
    mag = abs(alpha) * ops.absP() + (absD if absD is not None else 0.0)
    if ops.f32:
        return gamma(ops.K + 1 + extra, 2.0 ** -24) * mag
    return 2 * gamma(ops.K + extra, 2.0 ** -53) * mag + 2.0 ** -53 * mag


def assert_norms(got, C, lower, what):
    """Tile norms against the fp64 tile norms of the C the launch returned.  A sum of 128 x 128 non-negative terms, each
    one rounding for the square, summed in double in any order, plus at most 64 additions for the wave / band / table
    combination, is within gamma_(16384 + 64) of the exact value (u = 2^-53, both element types: the squares are taken
    in double); twice that, because the reference sum carries the same bound."""
    ref = tile_norms(C, lower)
    bound = 2 * gamma(T * T + 64, 2.0 ** -53) * ref
    worst = float(((got - ref).abs() / bound).max())
    print(f"{what}: worst |norm - ref| / bound = {worst:.3e}")
    assert bool(((got - ref).abs() <= bound).all()), f"{what}: worst {worst:.3e}"


def normal_like(view, seed):
    g = torch.Generator().manual_seed(seed)
    view.copy_(torch.randn(view.shape, generator=g, dtype=torch.float64).to(view.dtype).to(view.device))


def test_epilogue_rounding_legs(lib):
    """The fused epilogues have store arithmetic of their own (transposed store; sums of squares in double; o = alpha v + D,
    aux = o + D), in kernels of their own: standard-normal operands against derived bounds, fp64 and fp32 (fp32: K <= 1024
    wherever C is bounded)."""
    # --- 1 mirror: the lower part within the product bound, the upper triangle its transpose bit for bit
    for n_, walk, tile, want, f32 in ((1024, 0, 128, {"xcd": 0}, 0), (1024, 1, 128, {"xcd": 0}, 1), (7168, 9, 0, {"xcd": 1}, 0)):
        ops = Ops(n_, n_, 1024, kind="normal", f32=f32, seed=90)
        A, B = ops.stored(0, 0)
        buf, C = c_buffer(n_, n_, 0.0, f32, 0)
        a = gemm_args(A, B, C, n_, n_, 1024, -0.5, 0.0, 0, 0, 1, walk=walk, tile=tile, epi=1)
        what = f"mirror rounding {n_} f32 {f32}"
        check_route(route(lib, f32, a), {"rc": 0, "tile": 128, "sk_first": -1, "epi": 1, **want}, what)
        assert launch(lib, f32, a) == 0, what
        low = torch.tril(torch.ones(n_, n_, dtype=torch.bool, device=dev()))
        err, bound = (C.double() + 0.5 * ops.P()).abs(), sum_bound(ops, -0.5)
        print(f"{what}: worst |C - C_ref| / bound = {float((err / bound)[low].max()):.3e}")
        assert bool((err <= bound)[low].all()), what
        assert torch.equal(torch.triu(C, 1), torch.tril(C, -1).T), what + ": upper triangle != lower triangle transposed"
        frame = torch.ones_like(buf, dtype=torch.bool)
        frame[G:-G, G:-G] = False
        assert bool(buf[frame].isnan().all()), what
        del ops
    # --- 2 tile norms: C within the product bound (where the bound is stated), the table against the norms of that C
    table = (((1024, 1024, 1024, 1, 0, 0, 0, 128), {"sk_first": -1, "xcd": 0}, (0, 1)), ((1024, 768, 512, 0, 0, 0, 2, 128), {"sk_first": -1, "xcd": 0}, (0, 1)),
             ((7168, 7168, 1024, 1, 0, 0, 9, 0), {"xcd": 1}, (0,)), ((3712, 3712, 3712, 1, 1, 1, 0, 0), {"sk_first": 0, "xcd": 0}, (0, 1)))
    for (M, N, K, lower, at, bt, walk, tile), want, types in table:
        for f32 in types:
            ops = Ops(M, N, K, at, bt, "normal", f32, seed=91)
            A, B = ops.stored(0, 1)
            buf, C = c_buffer(M, N, 0.0, f32, 0)
            nt = (M // T) * (M // T + 1) // 2 if lower else (M // T) * (N // T)
            entries = 33 * nt if want.get("sk_first") == 0 else nt
            ss = torch.full((entries + 8,), NAN, dtype=torch.float64, device=dev())
            a = gemm_args(A, B, C, M, N, K, -1.0, 0.0, 0, 1, lower, at, bt, walk, tile, epi=2, sumsq=ss)
            what = f"tile-norm rounding {M} x {N} x {K} lower {lower} tri {at}{bt} f32 {f32}"
            check_route(route(lib, f32, a), {"rc": 0, "tile": 128, "epi": 2, "sumsq_entries": entries, **want}, what)
            assert launch(lib, f32, a) == 0, what + ": " + _lib.last_error()
            written = block_lower_mask(M, N) if lower else torch.ones(M, N, dtype=torch.bool, device=dev())
            assert bool(C[written].isfinite().all()) and bool(C[~written].isnan().all()), what
            if not f32 or K <= 1024:
                err, bound = (C.double() + ops.P()).abs(), sum_bound(ops, -1.0)
                print(f"{what}: worst |C - C_ref| / bound = {float((err / bound.clamp_min(1e-300))[written].max()):.3e}")
                assert bool((err <= bound)[written].all()), what
            got = ss[:nt] if entries == nt else ss[:nt] + ss[nt:entries].reshape(nt, 32).sum(1)
            assert_norms(got, torch.nan_to_num(C), lower, what)
            assert bool(ss[entries:].isnan().all()), what
            del ops
    probs = batch_problems(3, 512, 512, 512, 1, 1, "normal", 0, seed=92)
    st = [p.stored(0, 1) for p in probs]
    bufs = [c_buffer(512, 512, 0.0, 0, 0) for _ in probs]
    tabs = [torch.full((10 + 8,), NAN, dtype=torch.float64, device=dev()) for _ in probs]
    a = gemm_args(None, None, None, 512, 512, 512, 1.0, 0.0, 0, 1, 1, 1, 1, 0, 128, lda=st[0][0].stride(0), ldb=st[0][1].stride(0),
                  ldc=bufs[0][1].stride(0), nptr=3, Ap=[x[0] for x in st], Bp=[x[1] for x in st], Cp=[b[1] for b in bufs], epi=2, sumsqp=tabs)
    check_route(route(lib, 0, a), {"rc": 0, "tile": 128, "epi": 2, "sumsq_entries": 10}, "tile-norm rounding, pointer batch")
    assert launch(lib, 0, a) == 0
    for p, (_, c), t in zip(probs, bufs, tabs):
        m = block_lower_mask(512, 512)
        assert bool(((c - p.P()).abs() <= sum_bound(p, 1.0))[m].all())
        assert_norms(t[:10], torch.nan_to_num(c), 1, "tile-norm rounding, pointer batch")
    # --- 4 dual update: C = fl(fl(alpha v) + D) is two more roundings than the product, aux = fl(C + D) three
    for f32, n_, nptr in ((0, 2048, 0), (0, 2048, 2), (1, 1024, 0), (1, 1024, 2)):
        probs = batch_problems(max(nptr, 1), n_, n_, n_, 0, 1, "normal", f32, seed=93)
        st = [p.stored(0, 1) for p in probs]
        cb = [c_buffer(n_, n_, 0.0, f32, 0) for _ in probs]
        db = [c_buffer(n_, n_, 0.0, f32, 0) for _ in probs]
        for b, (_, d) in enumerate(db):
            normal_like(d, 94 + b)
        d0 = [d.clone() for _, d in db]
        alpha = 1.5
        if nptr:
            a = gemm_args(None, None, None, n_, n_, n_, alpha, 5.0, 0, 1, 0, 0, 1, 0, 128, lda=st[0][0].stride(0), ldb=st[0][1].stride(0),
                          ldc=cb[0][1].stride(0), nptr=nptr, Ap=[x[0] for x in st], Bp=[x[1] for x in st], Cp=[c[1] for c in cb],
                          auxp=[d[1] for d in db], epi=4)
        else:
            a = gemm_args(st[0][0], st[0][1], cb[0][1], n_, n_, n_, alpha, 5.0, 0, 1, 0, 0, 1, 0, 128, aux=db[0][1], epi=4)
        what = f"dual-update rounding {n_} nptr {nptr} f32 {f32}"
        check_route(route(lib, f32, a), {"rc": 0, "tile": 128, "sk_first": -1, "xcd": 0, "epi": 4}, what)
        assert launch(lib, f32, a) == 0, what + ": " + _lib.last_error()
        for p, (bufc, c), (bufd, d), x in zip(probs, cb, db, d0):
            xd = x.double()
            eh = (c.double() - (alpha * p.P() + xd)).abs()
            ea = (d.double() - (alpha * p.P() + 2 * xd)).abs()
            bh, ba = sum_bound(p, alpha, 2, xd.abs()), sum_bound(p, alpha, 3, 2 * xd.abs())
            print(f"{what}: worst |C - ref| / bound = {float((eh / bh).max()):.3e}, aux {float((ea / ba).max()):.3e}")
            assert bool((eh <= bh).all()) and bool((ea <= ba).all()), what
            assert torch.equal(d, c + x), what + ": aux != C + D"
            for buf in (bufc, bufd):
                frame = torch.ones_like(buf, dtype=torch.bool)
                frame[G:-G, G:-G] = False
                assert bool(buf[frame].isnan().all()), what
