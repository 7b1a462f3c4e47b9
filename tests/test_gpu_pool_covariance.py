"""The posterior covariance of a shortlist in one device call (gpfit_pool_covariance through utils.pool_covariance) against
the long-double covariance of select_cases.sigma_longdouble and against today's composition on the device
(acosker(xs, xs) + (Z S) Z^T from utils.acosker / utils.matmul); the diagonal (bits of pool_moments' sigma2), symmetry, the
lower-triangle convention of S, repeats / capacity / row offset, the mask path, stale workspace, refusals.

Shortlists are the pools of predict_cases.CASES, the smallest shapes at which a tile mechanism can fail: one row; 130 rows
(two ragged tiles with one mirrored off-diagonal tile), with the identity basis and projected; 300 rows (three tiles).

Accuracy bound, as in test_gpu_predict_pool.py: the error of the call may be at most ten times that of the composition on
the same inputs (both against long double, relative to max |Sigma|, floored at 1e-15) -- the same leading error term, a
different association and summation order."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import predict_cases as cases
import select_cases as sel

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
WORK_MATRICES = (b"Abuf", b"Tbuf", b"Wbuf", b"Zbuf", b"Cos", b"TmpV", b"Tmp", b"Kbuf")
IDS = lambda s: "P{}-nt{}-k{}-px{}".format(*s)  # noqa: E731


def T(a):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()      # a copy: shared inputs are read-only


def bits(t):
    return t.detach().cpu().numpy().view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def gp():
    from gaussian_processes_amd import utils
    return utils


@pytest.fixture(scope="module")
def lib():
    from gaussian_processes_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _unit(shape):
    """The case on the device (shared between the tests, never written), as test_gpu_predict_pool builds it."""
    from gaussian_processes_amd import utils as gp
    c = cases.make_case(*shape)
    mask = torch.from_numpy(c["mask"]).cuda()
    u = {k: T(c[k]) for k in ("C", "K", "Kinv", "m", "V")}
    u["xs_full"], u["xt_full"], u["mask"] = T(c["xstar"]), T(c["xtilde"]), mask
    u["xs"], u["xt"] = u["xs_full"][:, mask].contiguous(), u["xt_full"][:, mask].contiguous()
    u["B"] = gp._mark_identity(torch.eye(c["nt"], dtype=torch.float64, device="cuda")) if c["B"] is None else T(c["B"])
    u["theta"] = c["theta"]
    u["folded"] = gp.fold_posterior(u["K"], u["Kinv"], u["m"], u["V"], u["B"])
    return u


@functools.lru_cache(maxsize=None)
def _reference(shape):
    Sigma, _ = sel.sigma_longdouble(cases.make_case(*shape))
    Sigma.setflags(write=False)
    return Sigma


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def raw(lib, ctx, u, xs=None, S=None, Sigma=None, ldsig=None, M=None):
    """gpfit_pool_covariance itself on the masked inputs of a unit: (rc, Sigma); Sigma starts as the sentinel."""
    f = u["folded"]
    xs = u["xs"] if xs is None else xs
    S = f["S"] if S is None else S
    B = f["B"]
    M = xs.shape[0] if M is None else M
    nt, d = u["xt"].shape[0], u["xt"].shape[1]
    if Sigma is None:
        Sigma = torch.full((max(M, 1), max(M, 1)), SENTINEL, dtype=torch.float64, device="cuda")
    rc = lib.gpfit_pool_covariance(ctx, _stream(), float(u["theta"]["sigma_0"]), xs.data_ptr() if xs is not None else None,
                                   xs.stride(0), M, None, d, u["xt"].data_ptr(), u["xt"].stride(0), nt, d, u["C"].data_ptr(),
                                   u["C"].stride(0), B.data_ptr() if B is not None else None, B.stride(0) if B is not None else 0,
                                   f["k"], S.data_ptr(), S.stride(0), Sigma.data_ptr() if Sigma is not False else None,
                                   Sigma.stride(0) if ldsig is None else ldsig)
    torch.cuda.synchronize()
    return rc, Sigma


# ------------------------------------------------------------------ 1. accuracy, diagonal, symmetry
@pytest.mark.parametrize("shape", cases.CASES, ids=IDS)
def test_covariance_is_as_accurate_as_todays_composition(gp, shape):
    u = _unit(shape)
    ref = _reference(shape)
    Sigma = gp.pool_covariance(u["xs"], u["xt"], u["C"], u["theta"], u["folded"])
    assert tuple(Sigma.shape) == (shape[0], shape[0]) and not torch.isnan(Sigma).any()
    # symmetric bit for bit; the diagonal is the pool call's sigma2
    assert same_bits(Sigma, Sigma.T.contiguous())
    _, s2 = gp.pool_moments(u["xs"], u["xt"], u["C"], u["theta"], u["folded"])
    assert same_bits(torch.diagonal(Sigma).contiguous(), s2)
    # today's composition on the device
    Z = gp.acosker(u["theta"], u["xs"], u["xt"], C=u["C"])
    if u["folded"]["B"] is not None:
        Z = gp.matmul(Z, u["folded"]["B"])
    if shape[0] > 1:
        Kss = gp.acosker(u["theta"], u["xs"], u["xs"], C=u["C"])
    else:
        Kss = gp.acosker(u["theta"], u["xs"], x2=None, C=u["C"], diag=True).reshape(1, 1)
    old = Kss + gp.matmul(gp.matmul(Z, u["folded"]["S"]), Z, transB=True)
    off = ~np.eye(shape[0], dtype=bool) if shape[0] > 1 else np.ones((1, 1), dtype=bool)
    scale = np.max(np.abs(ref))
    e_new = float(np.max(np.abs(Sigma.cpu().numpy().astype(cases.LD) - ref)[off]) / scale)
    e_old = float(np.max(np.abs(old.cpu().numpy().astype(cases.LD) - ref)[off]) / scale)
    print(f"\n{shape}: off-diagonal e_new {e_new:.2e} e_old {e_old:.2e}")
    assert e_new <= 10 * max(e_old, 1e-15)


def test_diagonal_is_not_that_of_the_off_diagonal_formula(gp):
    """k(x, x) of the off-diagonal formula carries the + 1e-7 of its cosine; the moments' k** does not."""
    u = _unit(cases.CASES[1])
    Sigma = gp.pool_covariance(u["xs"], u["xt"], u["C"], u["theta"], u["folded"])
    Kss = gp.acosker(u["theta"], u["xs"], u["xs"], C=u["C"])
    kss = gp.acosker(u["theta"], u["xs"], x2=None, C=u["C"], diag=True).reshape(-1)
    d_new = torch.diagonal(Sigma)
    Z = gp.acosker(u["theta"], u["xs"], u["xt"], C=u["C"])
    quad = (gp.matmul(Z, u["folded"]["S"]) * Z).sum(1)
    assert float(torch.max(torch.abs(d_new - (kss + quad)))) < float(torch.max(torch.abs(d_new - (torch.diagonal(Kss) + quad))))


# ------------------------------------------------------------------ 2. the lower triangle of S is canonical
def test_strict_upper_triangle_of_S_is_never_read(gp, lib):
    u = _unit(cases.PROJECTED)
    k = u["folded"]["k"]
    eng = gp.get_engine(256, u["xs"].shape[1])
    S_nan = u["folded"]["S"].clone()
    S_nan[torch.triu(torch.ones(k, k, dtype=torch.bool, device="cuda"), diagonal=1)] = float("nan")
    rc0, a = raw(lib, eng._ctx, u)
    rc1, b = raw(lib, eng._ctx, u, S=S_nan)
    assert rc0 == 0 and rc1 == 0 and not torch.isnan(a).any()
    assert same_bits(a, b)


# ------------------------------------------------------------------ 3. repeats, capacity, position in the shortlist
@pytest.mark.parametrize("shape", [cases.CASES[1], cases.PROJECTED, cases.CHUNKED], ids=IDS)
def test_repeat_capacity_and_row_offset_do_not_change_a_bit(gp, lib, shape):
    from gaussian_processes_amd.engine import GPFitEngine
    u = _unit(shape)
    args = (u["xt"], u["C"], u["theta"], u["folded"])
    base = gp.pool_covariance(u["xs"], *args)
    assert same_bits(base, gp.pool_covariance(u["xs"], *args))
    big = GPFitEngine(1024, 64)
    try:
        rc, other = raw(lib, big._ctx, u)
        assert rc == 0 and same_bits(base, other)
    finally:
        big.close()
    # rows moved inside the shortlist: without the first three rows every row sits three places earlier, row 128 in another tile
    moved = gp.pool_covariance(u["xs"][3:].contiguous(), *args)
    assert same_bits(base[3:, 3:].contiguous(), moved)
    # two rows alone, taken from two different tiles
    pair = gp.pool_covariance(u["xs"][[5, 129]].contiguous(), *args)
    assert same_bits(base[[5, 129]][:, [5, 129]].contiguous(), pair)


# ------------------------------------------------------------------ 4. the mask path
def test_whole_images_with_a_mask_equal_masked_images(gp):
    u = _unit(cases.CASES[1])
    keep = torch.ones(64, dtype=torch.bool)
    keep[torch.tensor([0, 5, 9, 17, 30, 31, 32, 50, 63])] = False
    keep = keep.cuda()
    Csub = u["C"][keep][:, keep].contiguous()
    xt = u["xt_full"][:, keep].contiguous()
    a = gp.pool_covariance(u["xs_full"][:, keep].contiguous(), xt, Csub, u["theta"], u["folded"])
    b = gp.pool_covariance(u["xs_full"], xt, Csub, u["theta"], u["folded"], mask=keep)
    c = gp.pool_covariance(u["xs_full"], u["xt_full"], Csub, u["theta"], u["folded"], mask=keep)
    full = gp.pool_covariance(u["xs"], u["xt"], u["C"], u["theta"], u["folded"])
    assert same_bits(a, b) and same_bits(a, c)
    assert not same_bits(a, full)


# ------------------------------------------------------------------ 5. stale workspace
def test_padding_is_written_not_assumed(gp, lib):
    u = _unit(cases.PROJECTED)
    clean = gp.pool_covariance(u["xs"], u["xt"], u["C"], u["theta"], u["folded"])
    eng = gp.get_engine(200, 64, 64)
    for name in WORK_MATRICES:
        assert lib.gpfit_dev_ctx_fill(eng._ctx, name, 0xFF) == 0          # every double a NaN
    assert gp.get_engine(200, 64, 64) is eng
    Sigma = gp.pool_covariance(u["xs"], u["xt"], u["C"], u["theta"], u["folded"])
    assert not torch.isnan(Sigma).any() and same_bits(Sigma, clean)
    for name in WORK_MATRICES:
        assert lib.gpfit_dev_ctx_fill(eng._ctx, name, 0) == 0             # as a fresh context holds them


# ------------------------------------------------------------------ 6. edges and refusals
def test_empty_shortlist(gp):
    u = _unit(cases.CASES[1])
    Sigma = gp.pool_covariance(u["xs"][:0], u["xt"], u["C"], u["theta"], u["folded"])
    assert tuple(Sigma.shape) == (0, 0) and Sigma.dtype == torch.float64


def test_refusals_write_nothing(gp, lib):
    from gaussian_processes_amd import _lib
    from gaussian_processes_amd.engine import GPFitEngine
    u = _unit(cases.CASES[1])
    small = GPFitEngine(200, 64)            # capacity 256: nt = k = 200 fit, 300 rows do not
    try:
        xs = _unit(cases.CHUNKED)["xs"]
        rc, Sigma = raw(lib, small._ctx, u, xs=xs)
        assert rc == -3 and "larger than the context capacity" in _lib.last_error()
        assert bool((Sigma == SENTINEL).all())
    finally:
        small.close()
    eng = gp.get_engine(256, 64)
    M = u["xs"].shape[0]
    Sigma = torch.full((M, M), SENTINEL, dtype=torch.float64, device="cuda")
    rc, _ = raw(lib, eng._ctx, u, Sigma=Sigma, ldsig=M - 1)
    assert rc == -3 and "bad argument" in _lib.last_error() and bool((Sigma == SENTINEL).all())
    rc, _ = raw(lib, eng._ctx, u, Sigma=False, ldsig=M)
    assert rc == -3 and "bad argument" in _lib.last_error()
    rc = lib.gpfit_pool_covariance(None, _stream(), 1.0, u["xs"].data_ptr(), u["xs"].stride(0), M, None, 64, u["xt"].data_ptr(),
                                   u["xt"].stride(0), 200, 64, u["C"].data_ptr(), u["C"].stride(0), None, 0, 200,
                                   u["folded"]["S"].data_ptr(), 200, Sigma.data_ptr(), M)
    assert rc == -3 and bool((Sigma == SENTINEL).all())
