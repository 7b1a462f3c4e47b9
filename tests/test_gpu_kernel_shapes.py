"""GPU parity of the materialising entry points beyond a single tile: gpfit_acosker (K and the six dK),
gpfit_acosker_diag, gpfit_acosker_pullback, gpfit_localker, gpfit_nd_utility, and the context's state between them.

``tests/test_gpu_kernels.py`` compares these entry points with the real reference at shapes that are one workgroup
of the Gram kernel (128 x 128 tiles), one 256-wide block of the element-wise derivative kernels and one padded pixel
count.  Here they run at n = 129 ... 385 (two and three tile rows, the 256-thread column block crossed, odd leading
dimensions of the products written into dK), d = 9 ... 576 (dp = 32, 64, 128, 160), with duplicate, negated, scaled
and all-zero rows planted across the tile boundary, against the extended-precision restatement of the reference in
``tests/test_kernel_reference_cpu.py`` (longdouble; mpmath for the utility).  Every matrix is compared as a whole
and per 128 x 128 tile.  Inputs: seeds, ``gaussian_processes_amd.synthetic`` and ``oracle.gp_oracle``; the metric
C, dC handed to the device acosker is the oracle's, so that localker's error stays out of these tests.

Bars.  ``FLOOR`` is the error of the fp64 oracle (for the pull-back: of two fp64 host evaluations, the materialised
contraction and the adjoint form) against the extended-precision reference on the same inputs, as measured on the
CPU; ``test_kernel_reference_cpu.py`` asserts that what it measures lies within a factor of two of the table.  A
kernel's bar is the larger of the project's bar (K 1e-12, dK 1e-11, Kvec 1e-13, dKvec 1e-12, localker 1e-13;
``conftest.relerr``) and 8 x the floor; for the pull-back
(each component scaled by sum |W dK_p| + sum |t dKvec_p|) and for U (scaled by |H_r| + |H_mean|), whose summation order
no host order reproduces, 16 x the floor and never looser than 1e-9 (``test_kernel_reference_cpu.bar``)."""
import ctypes

import numpy as np
import pytest
import torch

from gaussian_processes_amd import synthetic as syn
from oracle import gp_oracle as orc
import test_kernel_reference_cpu as ref
from test_kernel_reference_cpu import DCK, KEYS, LD, LOWER, UPPER, bar, tile_relerr

# case -> quantity -> floor as measured (see the module docstring); every bar below is
# ref.bar(quantity, FLOOR[case][quantity])
FLOOR = {
    # acosker: K and the worst of the six dK, whole matrix and per tile      -> bars: the project's 1e-12 / 1e-11
    "same_dC-129-3x3": {"K": 4.28e-14, "dK": 4.52e-14},
    "same_dC-129-12x12": {"K": 8.69e-15, "dK": 1.36e-14},
    "same_dC-257-8x8": {"K": 4.38e-14, "dK": 6.98e-14},
    "same_dC-257-16x16m": {"K": 5.65e-14, "dK": 5.69e-14},
    "same_dC-257-12x12": {"K": 7.64e-15, "dK": 2.77e-14},
    "same-129-16x16n": {"K": 4.44e-14},
    "same-129-12x12": {"K": 8.36e-15},
    "same-257-3x3": {"K": 5.42e-14},
    "same-257-8x8": {"K": 1.83e-14},
    "same-257-16x16m": {"K": 3.01e-14},
    "same-257-12x12": {"K": 6.10e-15},
    "same-385-12x12n": {"K": 4.79e-14},
    "same-385-12x12": {"K": 1.36e-14},
    "same-385-16x8": {"K": 7.17e-15},
    "clip-140-3x3": {"K": 3.90e-16, "dK": 4.91e-16},
    "clip-140-12x12": {"K": 3.90e-16, "dK": 7.69e-16},
    "clip_nodC-140-3x3": {"K": 3.90e-16},
    "clip_nodC-140-12x12": {"K": 4.15e-16},
    "distinct-129-12x12": {"K": 4.15e-15, "dK": 5.20e-15},
    "distinct-257-3x3": {"K": 2.83e-14, "dK": 3.84e-14},
    "distinct-257-16x16n": {"K": 1.04e-15, "dK": 1.35e-14},
    "rect-129x300-12x12": {"K": 1.01e-15, "dK": 1.37e-15},
    "rect-129x300-3x3": {"K": 2.74e-15, "dK": 7.82e-15},
    "rect-300x129-12x12n": {"K": 6.21e-16, "dK": 1.05e-15},
    "rect-300x129-16x8": {"K": 9.31e-15, "dK": 1.36e-14},
    "rect-1x257-12x12": {"K": 7.62e-15, "dK": 7.65e-15},
    "rect-1x257-3x3": {"K": 9.10e-15, "dK": 1.28e-14},
    "rect-257x1-12x12": {"K": 3.48e-16, "dK": 8.87e-16},
    "rect-257x1-16x16m": {"K": 1.24e-15, "dK": 7.40e-15},
    "rect-131x77-12x12": {"K": 6.84e-15, "dK": 1.15e-14},
    "rect-131x77-3x3": {"K": 1.91e-15, "dK": 5.81e-15},
    "rect-131x77-16x16m": {"K": 1.05e-14, "dK": 4.06e-14},
    "rect-2x3-3x3": {"K": 2.95e-16, "dK": 6.00e-16},
    "rect-2x3-12x12": {"K": 1.69e-16, "dK": 8.74e-16},
    "rect-1x129-8x8-nodC": {"K": 2.76e-14},
    # acosker(diag=True)                                                     -> bars: the project's 1e-13 / 1e-12
    "diag-1-3x3": {"Kvec": 0.0, "dKvec": 2.79e-16},
    "diag-257-3x3": {"Kvec": 1.12e-16, "dKvec": 2.44e-16},
    "diag-300-3x3": {"Kvec": 1.47e-16, "dKvec": 3.16e-16},
    "diag-1-12x12": {"Kvec": 0.0, "dKvec": 1.96e-15},
    "diag-257-12x12": {"Kvec": 1.93e-16, "dKvec": 3.97e-16},
    "diag-300-12x12": {"Kvec": 2.19e-16, "dKvec": 3.96e-16},
    # the pull-back, error / (sum |W dK_p| + sum |t dKvec_p|)                -> bars: 16 x, 1.5e-16 ... 2.1e-14
    "pull-65x63-3x3": {"pullback": 5.28e-17},
    "pull-129x300-3x3": {"pullback": 2.01e-17},
    "pull-300x129-3x3": {"pullback": 9.17e-18},
    "pull-130x130-3x3": {"pullback": 2.60e-17},
    "pull-1x64-3x3": {"pullback": 3.93e-16},
    "pull-65x63-16x16m": {"pullback": 5.53e-17},
    "pull-129x300-16x16m": {"pullback": 1.25e-17},
    "pull-300x129-16x16m": {"pullback": 1.29e-17},
    "pull-130x130-16x16m": {"pullback": 1.53e-17},
    "pull-1x64-16x16m": {"pullback": 1.30e-15},
    # nd_utility, error / (|H_r| + |H_mean|)                                 -> bars: 16 x, 2.2e-14 ... 9.7e-13
    "utility": {"U": 6.06e-14},
    "utility-nr1": {"U": 1.99e-15},
    "utility-nr127": {"U": 1.39e-15},
    "utility-nr128": {"U": 1.50e-15},
    "utility-nr129": {"U": 1.38e-15},
    "utility-nr300": {"U": 1.51e-14},
}

pytestmark = pytest.mark.gpu
SENTINEL = -7.25


def tth(theta):
    return {k: torch.tensor(float(theta[k]), dtype=torch.float64) for k in KEYS}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def dev_dC(dC):
    return None if dC is None else {k: dC[k].cuda() for k in DCK}


@pytest.fixture(scope="module")
def gp():
    from gaussian_processes_amd import utils
    return utils


def check(name, quantity, got, want):
    e, b = tile_relerr(got, want), bar(quantity, FLOOR[name][quantity])
    print(f"{name} {quantity}: {e:.3e} (bar {b:.3e})")
    assert e < b, (name, quantity, e, b)


# ------------------------------------------------------------------ acosker
@pytest.mark.parametrize("name", [c[0] for c in ref.ACOS_CASES])
def test_acosker_matches_reference(gp, name):
    """K and the six dK against the longdouble reference, whole and per tile; K exactly symmetric whenever
    n1 == n2 (lower tiles + mirror, or the average of both triangles), dK as the reference leaves it."""
    _, _, n1, n2, kind, _ = ref.ACOS_BY_NAME[name]
    s0, x1, x2, C, dC = ref.acos_inputs(name)
    Kr, dKr = ref.acos_reference(name)
    th = tth({**dict.fromkeys(KEYS, 0.0), "sigma_0": s0})
    X1 = T(x1)
    X2 = X1 if kind == "same" else T(x2)
    if name.startswith("rect-1x129"):
        X1 = X1[0]                                   # a 1-D x1
    out = gp.acosker(th, X1, X2, C=C.cuda(), dC=dev_dC(dC), diag=False)
    K, dK = out if dC is not None else (out, None)
    assert K.shape == (n1, n2)
    check(name, "K", K.cpu().numpy(), Kr)
    if n1 == n2:
        assert torch.equal(K, K.T)
    if dC is not None:
        assert list(dK) == list(KEYS)
        for k in KEYS:
            assert dK[k].shape == (n1, n2)
            check(name, "dK", dK[k].cpu().numpy(), dKr[k])


@pytest.mark.parametrize("name", ["same_dC-129-3x3", "same_dC-257-12x12", "same_dC-257-16x16m"])
def test_acosker_same_matrix_by_every_route(gp, name):
    """acosker(x, x) without dC (lower tiles + mirror), with dC (full grid + average) and with x2 = x.clone() (two
    gathers, two q vectors) are one K; the clone's dK are the same-pointer call's."""
    s0, x1, _, C, dC = ref.acos_inputs(name)
    Kr, dKr = ref.acos_reference(name)
    th = tth({**dict.fromkeys(KEYS, 0.0), "sigma_0": s0})
    X, Cd, dCd = T(x1), C.cuda(), dev_dC(dC)
    K0 = gp.acosker(th, X, X, C=Cd)
    K1, dK1 = gp.acosker(th, X, X, C=Cd, dC=dCd)
    K2, dK2 = gp.acosker(th, X, X.clone(), C=Cd, dC=dCd)
    K3 = gp.acosker(th, X, X.clone(), C=Cd)
    kbar, dbar = bar("K", FLOOR[name]["K"]), bar("dK", FLOOR[name]["dK"])
    for K in (K0, K2, K3):
        assert torch.equal(K, K.T)
        assert tile_relerr(K.cpu().numpy(), K1.cpu().numpy()) < kbar
        assert tile_relerr(K.cpu().numpy(), Kr) < kbar
    for k in KEYS:
        assert tile_relerr(dK2[k].cpu().numpy(), dK1[k].cpu().numpy()) < dbar, k
        assert tile_relerr(dK2[k].cpu().numpy(), dKr[k]) < dbar, k


def test_acosker_strided_operands_through_the_c_abi(gp):
    """ld1, ld2 > d, ldC > d and ldk > n2 through ctypes: the columns of K from n2 to ldk keep the caller's bytes,
    nothing is written behind the six dK planes (nor, with dC = NULL, behind the first), and what lies beyond d in
    the operands is not read."""
    from gaussian_processes_amd import _lib
    name = "rect-131x77-12x12"
    s0, x1, x2, C, dC = ref.acos_inputs(name)
    Kr, dKr = ref.acos_reference(name)
    n1, d = x1.shape
    n2 = x2.shape[0]
    ld1, ld2, ldC, ldk, tail = d + 3, d + 5, d + 1, n2 + 7, 64
    dev = torch.device("cuda")

    def strided(a, ld):
        buf = torch.full((a.shape[0], ld), 1e30, dtype=torch.float64, device=dev)
        buf[:, :a.shape[1]] = T(a)
        return buf

    X1, X2, Cb = strided(x1, ld1), strided(x2, ld2), strided(C.numpy(), ldC)
    dCb = torch.stack([dC[k] for k in DCK]).contiguous().cuda()
    K = torch.full((n1, ldk), SENTINEL, dtype=torch.float64, device=dev)
    dK = torch.full((6 * n1 * n2 + tail,), SENTINEL, dtype=torch.float64, device=dev)
    eng = gp.get_engine(max(n1, n2), d)
    lib = _lib.load()
    _lib.check(lib.gpfit_acosker(eng._ctx, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), s0, X1.data_ptr(), ld1,
                                 n1, X2.data_ptr(), ld2, n2, d, Cb.data_ptr(), ldC, dCb.data_ptr(), K.data_ptr(), ldk,
                                 dK.data_ptr()), "gpfit_acosker")
    torch.cuda.synchronize()
    assert torch.all(K[:, n2:] == SENTINEL)
    assert torch.all(dK[6 * n1 * n2:] == SENTINEL)
    check(name, "K", K[:, :n2].cpu().numpy(), Kr)
    planes = dK[:6 * n1 * n2].view(6, n1, n2).cpu().numpy()
    for i, k in enumerate(KEYS):
        check(name, "dK", planes[i], dKr[k])
    # dC = NULL: only the sigma_0 plane is written, so an overrun of it would show in the five behind it
    K.fill_(SENTINEL)
    dK.fill_(SENTINEL)
    _lib.check(lib.gpfit_acosker(eng._ctx, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), s0, X1.data_ptr(), ld1,
                                 n1, X2.data_ptr(), ld2, n2, d, Cb.data_ptr(), ldC, None, K.data_ptr(), ldk, dK.data_ptr()),
               "gpfit_acosker")
    torch.cuda.synchronize()
    assert torch.all(K[:, n2:] == SENTINEL) and torch.all(dK[n1 * n2:] == SENTINEL)
    check(name, "K", K[:, :n2].cpu().numpy(), Kr)
    check(name, "dK", dK[:n1 * n2].view(n1, n2).cpu().numpy(), dKr["sigma_0"])


# ------------------------------------------------------------------ acosker(diag=True)
@pytest.mark.parametrize("name", [c[0] for c in ref.DIAG_CASES])
def test_acosker_diag_matches_reference(gp, name):
    s0, x1, C, dC = ref.diag_inputs(name)
    Kvr, dKvr = ref.diag_reference(name)
    n1 = x1.shape[0]
    th = tth({**dict.fromkeys(KEYS, 0.0), "sigma_0": s0})
    X, Cd = T(x1), C.cuda()
    Kv, dKv = gp.acosker(th, X, x2=None, C=Cd, dC=dev_dC(dC), diag=True)
    assert Kv.shape == (n1,) and list(dKv) == list(KEYS)
    check(name, "Kvec", Kv.cpu().numpy(), Kvr)
    for k in KEYS:
        assert dKv[k].shape == (n1,)
        check(name, "dKvec", dKv[k].cpu().numpy(), dKvr[k])
    Kv0 = gp.acosker(th, X, x2=None, C=Cd, dC=None, diag=True)
    assert Kv0.shape == (() if n1 == 1 else (n1,))          # the reference squeezes (utils.py:1030)
    assert torch.equal(Kv0.reshape(-1), Kv)


# ------------------------------------------------------------------ the rectangular pull-back
@pytest.mark.parametrize("with_t", [False, True], ids=["t_null", "t_random"])
@pytest.mark.parametrize("name", [c[0] for c in ref.PULLBACK_CASES])
def test_acosker_pullback_matches_contraction(gp, name, with_t):
    """gpfit_acosker_pullback through ctypes against the contraction of W (and t) with the materialised longdouble
    derivatives: <dC_p, (M + M^T)/2> for the five metric parameters, sigma_0 (2 out[0] + out[1] + out[2]) for sigma_0;
    the columns of M_out beyond d keep the caller's bytes."""
    from gaussian_processes_amd import _lib
    s0, x1, x2, C, dC, W, t = ref.pullback_inputs(name)
    g_ref, scale = ref.pullback_reference(name, with_t)
    n1, d = x1.shape
    n2 = x2.shape[0]
    ldm = d + 3
    X1, X2, Cd, Wd = T(x1), T(x2), C.cuda().contiguous(), T(W)
    td = T(t) if with_t else None
    M = torch.full((d, ldm), SENTINEL, dtype=torch.float64, device=X1.device)
    out3 = (ctypes.c_double * 3)()
    eng = gp.get_engine(max(n1, n2), d)
    lib = _lib.load()
    _lib.check(lib.gpfit_acosker_pullback(eng._ctx, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), s0,
                                          X1.data_ptr(), X1.stride(0), n1, X2.data_ptr(), X2.stride(0), n2, d, Cd.data_ptr(),
                                          Cd.stride(0), Wd.data_ptr(), Wd.stride(0), td.data_ptr() if with_t else None,
                                          M.data_ptr(), ldm, out3), "gpfit_acosker_pullback")
    torch.cuda.synchronize()
    assert torch.all(M[:, d:] == SENTINEL)
    Mh = M[:, :d].cpu().numpy().astype(LD)
    Ms = (Mh + Mh.T) / 2
    g = {k: (dC[k].numpy().astype(LD) * Ms).sum() for k in DCK}
    g["sigma_0"] = LD(s0) * (2 * LD(out3[0]) + LD(out3[1]) + LD(out3[2]))
    b = bar("pullback", FLOOR[name]["pullback"])
    assert b <= ref.LOOSEST
    for k in KEYS:
        e = abs(float(g[k] - g_ref[k])) / float(scale[k])
        print(f"{name} t={with_t} {k}: {e:.3e} (bar {b:.3e})")
        assert e < b, (name, with_t, k, e, b)


# ------------------------------------------------------------------ localker
@pytest.mark.parametrize("mname", ["24x24", "24x24n", "16x8", "8x16", "2x2", "1x1"])
def test_localker_matches_oracle(gp, mname):
    grid, theta, C, mask, dC = ref.metric(mname)
    Cd, maskd, dCd = gp.localker(tth(theta), UPPER, LOWER, grid, grad=True)
    assert np.array_equal(maskd.cpu().numpy(), mask.numpy())
    e = tile_relerr(Cd.cpu().numpy(), C.numpy())
    print(f"localker {mname} d={C.shape[0]} C: {e:.3e}")
    assert e < ref.PROJECT_BAR["localker"]
    assert list(dCd) == list(DCK)
    for k in DCK:
        e = tile_relerr(dCd[k].cpu().numpy(), dC[k].numpy())
        print(f"localker {mname} dC {k}: {e:.3e}")
        assert e < ref.PROJECT_BAR["localker"], k
    C2, mask2 = gp.localker(tth(theta), UPPER, LOWER, grid, grad=False)
    assert torch.equal(C2, Cd) and torch.equal(mask2, maskd)


# ------------------------------------------------------------------ the context between calls
def test_acosker_between_two_evaluations_keeps_the_context_state(gp):
    """One context, as a notebook interleaves the drop-in calls: a fused evaluation with gradients, then localker
    and acosker with dC at a size that rewrites the shared work buffers (Xt, XCt, q, Cos, dCpad), then the same
    evaluation reusing the factor of V: the bits of the first."""
    N, mname = 200, "4x4"
    grid, theta, C, mask, dC = ref.metric(mname)
    assert bool(mask.all()) and mask.numel() == 16
    X = torch.from_numpy(syn.stimuli(N, 16, 3))
    r_np, m_np = syn.cell_inputs(N)
    th0, th1 = syn.theta0(), syn.theta_eval()
    C0, mask0 = orc.spatial_metric(th0, LOWER, UPPER, grid)
    assert bool(mask0.all())
    V = 0.5 * orc.arccos_gram(th0, X, X, C0)
    eng = gp.reserve(N, 16, 16)
    args = (th1, LOWER, UPPER, grid, X.cuda(), T(r_np), T(m_np), V.cuda(), syn.F_PARAMS["logA"], syn.F_PARAMS["lambda0"])
    first = eng.fit_eval(*args, want_grad=True)
    loss, grad = orc.mstep_closure_cholesky(th1, LOWER, UPPER, grid, X, torch.from_numpy(r_np), torch.from_numpy(m_np), V,
                                            syn.F_PARAMS["logA"], syn.F_PARAMS["lambda0"])
    assert abs(first["loss"] - loss) < 1e-9 * abs(loss)
    Cd, _, dCd = gp.localker(tth(theta), UPPER, LOWER, grid, grad=True)
    x1, x2 = T(ref.stimuli(N, 16, 11)), T(ref.stimuli(137, 16, 12))
    K, dK = gp.acosker(tth(theta), x1, x2, C=Cd, dC=dCd)
    assert gp.get_engine(N, 16, 16) is eng
    Kr, dKr = ref.acosker_ld(theta["sigma_0"], x1.cpu().numpy(), x2.cpu().numpy(), C, dC)
    assert tile_relerr(K.cpu().numpy(), Kr) < ref.PROJECT_BAR["K"]
    again = eng.fit_eval(*args, want_grad=True, reuse_V=True)
    for k in ("loss", "loglik", "KL", "logdet_K", "logdet_V", "tr_KinvV", "mKinvm", "d"):
        assert again[k] == first[k], k
    assert again["grad"] == first["grad"]
    for k in ("lam_m", "lam_var", "f"):
        assert torch.equal(again[k], first[k]), k


# ------------------------------------------------------------------ nd_utility
def test_nd_utility_matches_mpmath(gp):
    """The device utility (Fritsch iteration for Lambert W) against mpmath (``mpmath.lambertw``) on chosen points:
    both sides of the start value's seam z = 2, z ~ 1e-300, z = 0 by underflow, z ~ 1e300, candidates with some and
    with all r >= 1 terms overflowing."""
    s2, mu, r = ref.utility_points()
    want = ref.utility_reference()
    U = gp.nd_utility(T(s2), T(mu), T(r)).cpu().numpy()
    assert np.all(np.isfinite(U))
    e, b = ref.utility_err(U, want), bar("U", FLOOR["utility"]["U"])
    print(f"nd_utility vs mpmath: {e:.3e} (bar {b:.3e})")
    assert b <= ref.LOOSEST
    assert e < b


@pytest.mark.parametrize("nstar", [1, 257])
@pytest.mark.parametrize("nr", ref.UTILITY_NR)
def test_nd_utility_block_seams(gp, nr, nstar):
    """nr on either side of the 128-thread stride, one and several candidates (one workgroup each): against mpmath
    and against the oracle."""
    s2, mu, r = ref.utility_seam_points(nr, nstar)
    want = ref.utility_seam_reference(nr)
    base = len(want["U"])
    tiled = {k: v[np.arange(nstar) % base] for k, v in want.items() if v.ndim == 1}
    U = gp.nd_utility(T(s2), T(mu), T(r)).cpu().numpy()
    floor = FLOOR[f"utility-nr{nr}"]["U"]
    e = ref.utility_err(U, tiled)
    print(f"nd_utility nr={nr} nstar={nstar} vs mpmath: {e:.3e} (bar {bar('U', floor):.3e})")
    assert e < bar("U", floor) <= ref.LOOSEST
    Uo = orc.active_utility(s2, mu, r).numpy()
    eo = float(np.max(np.abs(U - Uo) / np.maximum(np.abs(tiled["H_r"]) + np.abs(tiled["H_mean"]), 1e-300)))
    assert eo < bar("U", floor)
