"""Extended-precision restatement of the references behind the GPU tests of the materialising entry points
(acosker with its six dK, its diagonal form, its pull-back, nd_utility), pinned on the CPU.

``oracle.arccos_gram`` / ``arccos_gram_diag`` are the fp64 statement of reference utils.py:968-1044; here the same
formulas are evaluated in ``numpy.longdouble`` (eps 1.1e-19), and ``nd_utility`` (utils.py:414-525) in mpmath at 50
digits with ``mpmath.lambertw`` -- an evaluation that shares nothing with the Fritsch iteration the oracle and the
device both use.  The tests below pin these restatements to the fixtures of the real reference (G2, G8) and measure
the error of the fp64 oracle against them: that error is the floor from which ``tests/test_gpu_kernel_shapes.py``
sets its bars (table ``FLOOR`` there, asserted here so that it cannot rot).

The inputs of both modules are defined here once (``metric``, ``stimuli``, ``ACOS_CASES`` ...): seeds,
``gaussian_processes_amd.synthetic`` and ``oracle.gp_oracle`` only."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden, relerr
from gaussian_processes_amd import synthetic as syn
from oracle import gp_oracle as orc

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "numpy.longdouble is no extended precision here: the references below need it"
PI32 = LD(orc.PI32)             # a float32 value: exact in every wider format
KEYS = syn.THETA_KEYS
DCK = orc.DC_KEYS
LOWER, UPPER = syn.limits()
TILE = 128                      # output tile of the Gram kernel

# the project's bars (tests/test_gpu_kernels.py, conftest.relerr)
PROJECT_BAR = {"K": 1e-12, "dK": 1e-11, "Kvec": 1e-13, "dKvec": 1e-12, "localker": 1e-13}
LOOSEST = 1e-9                  # no pull-back or utility bar may be looser than this


def bar(quantity, floor):
    """Bar of a kernel against the extended-precision reference: the project's own bar, or 8 x the error the fp64
    oracle itself makes on the same inputs where that is larger.  The pull-back and U, whose summation order no
    host order reproduces, get 16 x their floor."""
    if quantity in ("pullback", "U"):
        return 16.0 * floor
    return max(PROJECT_BAR[quantity], 8.0 * floor)


# ------------------------------------------------------------------ inputs shared with the GPU module
def _g1_theta(case):
    return {k: float(v) for k, v in zip(KEYS, load_golden("g1_localker.npz")[f"c{case}_theta"])}


# name -> (pixel grid, G1 case whose theta is used): d, dp = round_up(d, 32)
METRICS = {
    "3x3": (3, 0),             # d = 9, dp = 32
    "8x8": (8, 0),             # d = 64 = dp
    "12x12n": (12, 2),         # narrow field: d = 54 of 144
    "16x16n": (16, 3),         # narrow field: d = 48 of 256
    "16x16m": (16, 2),         # narrow field: d = 99 of 256, odd
    "12x12": (12, 0),          # d = 144, dp = 160: no multiple of 64
    "16x8": ((16, 8), 0),      # d = 128
    "24x24": (24, 0),          # d = 576                                  (localker only)
    "24x24n": (24, 3),         # narrow field: d = 113 of 576, odd        (localker only)
    "8x16": ((8, 16), 0),      # d = 128                                  (localker only)
    "2x2": (2, 0),             # d = 4                                    (localker only)
    "1x1": (1, 0),             # d = 1                                    (localker only)
    "4x4": (4, 0),             # d = 16                                   (the state test)
}


@functools.lru_cache(maxsize=None)
def metric(name):
    """(grid, theta, C, mask, dC) of ``oracle.spatial_metric``; C, dC are fp64 torch tensors."""
    grid, case = METRICS[name]
    theta = _g1_theta(case)
    C, mask, dC = orc.spatial_metric(theta, LOWER, UPPER, grid, grad=True)
    return grid, theta, C, mask, dC


def stimuli(n, d_full, seed):
    """``syn.stimuli`` with planted rows that straddle the 128-row tile boundary: row 130 = row 0, row 131 = -row 0,
    row 132 = 2 row 1 (|cos| within 1e-7 / q^2 of 1 away from the diagonal tile; the +1e-7 keeps such rows off the clip
    itself, which the clip-* cases reach with rows scaled by 1e8) and the all-zero row 127 (q = sigma_0)."""
    X = syn.stimuli(n, d_full, seed).copy()
    if n > 130:
        X[130] = X[0]
    if n > 131:
        X[131] = -X[0]
    if n > 132:
        X[132] = 2.0 * X[1]
    if n > 127:
        X[127] = 0.0
    return X


def second_stimuli(n2, d_full, seed, x1):
    """A second matrix of its own, with two rows tied to ``x1``: |cos| next to 1 across the two matrices too."""
    X = stimuli(n2, d_full, seed)
    if n2 > 3:
        X[3] = x1[0]
    if n2 > 5 and x1.shape[0] > 1:
        X[n2 - 2] = -x1[1]
    return X


# (name, metric, n1, n2, kind, with dC); kind: "same" = acosker(x, x), "distinct" / "rect" = two matrices
ACOS_CASES = [
    # same matrix, with dC: full-grid Gram + symmetrize_avg of an already symmetric K
    ("same_dC-129-3x3", "3x3", 129, 129, "same", True),
    ("same_dC-129-12x12", "12x12", 129, 129, "same", True),
    ("same_dC-257-8x8", "8x8", 257, 257, "same", True),
    ("same_dC-257-16x16m", "16x16m", 257, 257, "same", True),
    ("same_dC-257-12x12", "12x12", 257, 257, "same", True),
    # same matrix, without dC: lower-tile path + mirror over up to three tile rows
    ("same-129-16x16n", "16x16n", 129, 129, "same", False),
    ("same-129-12x12", "12x12", 129, 129, "same", False),
    ("same-257-3x3", "3x3", 257, 257, "same", False),
    ("same-257-8x8", "8x8", 257, 257, "same", False),
    ("same-257-16x16m", "16x16m", 257, 257, "same", False),
    ("same-257-12x12", "12x12", 257, 257, "same", False),
    ("same-385-12x12n", "12x12n", 385, 385, "same", False),
    ("same-385-12x12", "12x12", 385, 385, "same", False),
    ("same-385-16x8", "16x8", 385, 385, "same", False),
    # rows 5 = 138 = 1e8 x row 2, row 137 = -1e9 x row 2: q1 q2 so large that the +1e-7 and sigma_0^2 are lost
    # and the fp64 cosine sits on its clip in the off-diagonal tiles (1, 0) / (0, 1); with dC (full grid + average) and
    # without (lower tiles + mirror)
    ("clip-140-3x3", "3x3", 140, 140, "same", True),
    ("clip-140-12x12", "12x12", 140, 140, "same", True),
    ("clip_nodC-140-3x3", "3x3", 140, 140, "same", False),
    ("clip_nodC-140-12x12", "12x12", 140, 140, "same", False),
    # n1 == n2, two matrices: the symmetrize_avg branch
    ("distinct-129-12x12", "12x12", 129, 129, "distinct", True),
    ("distinct-257-3x3", "3x3", 257, 257, "distinct", True),
    ("distinct-257-16x16n", "16x16n", 257, 257, "distinct", True),
    # rectangular
    ("rect-129x300-12x12", "12x12", 129, 300, "rect", True),
    ("rect-129x300-3x3", "3x3", 129, 300, "rect", True),
    ("rect-300x129-12x12n", "12x12n", 300, 129, "rect", True),
    ("rect-300x129-16x8", "16x8", 300, 129, "rect", True),
    ("rect-1x257-12x12", "12x12", 1, 257, "rect", True),
    ("rect-1x257-3x3", "3x3", 1, 257, "rect", True),
    ("rect-257x1-12x12", "12x12", 257, 1, "rect", True),
    ("rect-257x1-16x16m", "16x16m", 257, 1, "rect", True),
    ("rect-131x77-12x12", "12x12", 131, 77, "rect", True),
    ("rect-131x77-3x3", "3x3", 131, 77, "rect", True),
    ("rect-131x77-16x16m", "16x16m", 131, 77, "rect", True),
    ("rect-2x3-3x3", "3x3", 2, 3, "rect", True),
    ("rect-2x3-12x12", "12x12", 2, 3, "rect", True),
    ("rect-1x129-8x8-nodC", "8x8", 1, 129, "rect", False),
]
ACOS_BY_NAME = {c[0]: c for c in ACOS_CASES}

DIAG_CASES = [(f"diag-{n}-{m}", m, n) for m in ("3x3", "12x12") for n in (1, 257, 300)]

# (name, metric, n1, n2): W standard normal, t1_extra NULL and random
PULLBACK_CASES = [(f"pull-{n1}x{n2}-{m}", m, n1, n2) for m in ("3x3", "16x16m")
                  for n1, n2 in ((65, 63), (129, 300), (300, 129), (130, 130), (1, 64))]


def _seed(name):
    return 1 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100000


@functools.lru_cache(maxsize=None)
def acos_inputs(name):
    """(sigma_0, x1, x2, C, dC or None) of an ACOS case; x1, x2 masked fp64 numpy arrays (x2 is x1 for "same")."""
    _, mname, n1, n2, kind, with_dC = ACOS_BY_NAME[name]
    grid, theta, C, mask, dC = metric(mname)
    m = mask.numpy()
    full = m.size
    X1 = stimuli(n1, full, _seed(name))
    if name.startswith("clip"):
        X1[5], X1[137], X1[138] = 1e8 * X1[2], -1e9 * X1[2], 1e8 * X1[2]
    x1 = np.ascontiguousarray(X1[:, m])
    x2 = x1 if kind == "same" else np.ascontiguousarray(second_stimuli(n2, full, _seed(name) + 1, X1)[:, m])
    return theta["sigma_0"], x1, x2, C, (dC if with_dC else None)


@functools.lru_cache(maxsize=None)
def diag_inputs(name):
    _, mname, n1 = next(c for c in DIAG_CASES if c[0] == name)
    grid, theta, C, mask, dC = metric(mname)
    m = mask.numpy()
    return theta["sigma_0"], np.ascontiguousarray(stimuli(n1, m.size, _seed(name))[:, m]), C, dC


@functools.lru_cache(maxsize=None)
def pullback_inputs(name):
    """(sigma_0, x1, x2, C, dC, W, t) of a pull-back case."""
    _, mname, n1, n2 = next(c for c in PULLBACK_CASES if c[0] == name)
    grid, theta, C, mask, dC = metric(mname)
    m = mask.numpy()
    X1 = stimuli(n1, m.size, _seed(name))
    x1 = np.ascontiguousarray(X1[:, m])
    x2 = np.ascontiguousarray(second_stimuli(n2, m.size, _seed(name) + 1, X1)[:, m])
    rng = np.random.default_rng(_seed(name) + 2)
    return theta["sigma_0"], x1, x2, C, dC, rng.standard_normal((n1, n2)), rng.standard_normal(n1)


# ------------------------------------------------------------------ acosker in longdouble (utils.py:968-1044)
def _ld(a):
    return np.asarray(a.detach().numpy() if isinstance(a, torch.Tensor) else a, dtype=LD)


def acosker_ld(sigma0, x1, x2, C, dC=None):
    """``acosker(diag=False)``: K[n1, n2] (symmetrised iff n1 == n2) and, with dC, the six un-symmetrised dK, all in
    longdouble.  float32 pi, the +1e-7 and the clip are the reference's."""
    s0, x1, x2, C = LD(sigma0), _ld(x1), _ld(x2), _ld(C)
    x1C = x1 @ C
    q1 = np.sqrt((x1C * x1).sum(1) + s0 * s0)                       # :978
    q2 = np.sqrt(((x2 @ C) * x2).sum(1) + s0 * s0)                  # :979
    qq = np.outer(q1, q2)                                           # :981
    G = x1C @ x2.T + s0 * s0                                        # :982
    cosd = np.clip(G / (qq + LD(1e-7)), LD(-1), LD(1))              # :984
    delta = np.arccos(cosd)                                         # :986
    J = (np.sqrt(1 - cosd * cosd) + PI32 * cosd - delta * cosd) / PI32   # :988
    K = qq * J                                                      # :990
    dK = None
    if dC is not None:
        dK = {}
        dqq = s0 * s0 * (q2[None, :] / q1[:, None] + q1[:, None] / q2[None, :])   # :996
        dcos = (2 * s0 * s0 - cosd * dqq) / qq                      # :998
        dJ = -(delta - PI32) * dcos / PI32                          # :1000
        dK["sigma_0"] = (qq * dJ + dqq * J) / s0                    # :1004
        for key in DCK:
            D = _ld(dC[key])
            x1D = x1 @ D
            dq1 = LD(0.5) * (x1D * x1).sum(1) / q1                  # :1012
            dq2 = LD(0.5) * ((x2 @ D) * x2).sum(1) / q2             # :1013
            dqq = dq1[:, None] * q2[None, :] + q1[:, None] * dq2[None, :]   # :1015
            dcos = (x1D @ x2.T - cosd * dqq) / qq                   # :1017
            dJ = -(delta - PI32) * dcos / PI32                      # :1019
            dK[key] = qq * dJ + dqq * J                             # :1021
        dK = {k: dK[k] for k in KEYS}
    if x1.shape[0] == x2.shape[0]:
        K = (K + K.T) / 2                                           # :1024-1025 (dK is never symmetrised)
    return K, dK


def acosker_diag_ld(sigma0, x1, C, dC=None):
    """``acosker(diag=True)`` (utils.py:1027-1044): Kvec and, with dC, the six dKvec, in longdouble."""
    s0, x1, C = LD(sigma0), _ld(x1), _ld(C)
    Kvec = ((x1 @ C) * x1).sum(1) + s0 * s0                         # :1029
    if dC is None:
        return Kvec, None
    dKvec = {"sigma_0": np.full(x1.shape[0], 2 * s0 * s0 / s0)}     # :1036
    for key in DCK:
        dKvec[key] = ((x1 @ _ld(dC[key])) * x1).sum(1)              # :1042
    return Kvec, {k: dKvec[k] for k in KEYS}


def pullback_ld(sigma0, x1, x2, C, dC, W, t=None):
    """The contraction ``gpfit_acosker_pullback`` stands for, from the materialised derivatives in longdouble:
    g_p = sum_ij W_ij dK_p,ij + sum_i t_i dKvec_p,i for the five metric parameters, g_sigma0 = sum_ij W_ij dK_sigma0,ij
    (the entry point returns no t term for sigma_0).  Also the scale sum |W dK_p| + sum |t dKvec_p| of each: the sums
    cancel, so an error is measured against what was added up."""
    W = _ld(W)
    _, dK = acosker_ld(sigma0, x1, x2, C, dC)
    _, dKv = acosker_diag_ld(sigma0, x1, C, dC)
    g, scale = {}, {}
    for k in KEYS:
        g[k], scale[k] = (W * dK[k]).sum(), np.abs(W * dK[k]).sum()
        if t is not None and k != "sigma_0":
            g[k] += (_ld(t) * dKv[k]).sum()
            scale[k] += np.abs(_ld(t) * dKv[k]).sum()
    return g, scale


def pullback_f64(sigma0, x1, x2, C, dC, W, t=None):
    """Two fp64 host evaluations of the same six numbers: (a) the contraction with the oracle's materialised dK,
    (b) the adjoint form the entry point implements (include/gpfit_mi355x.h; the rectangular sibling of
    ``oracle.mstep_closure_cholesky``): A_w = W o (pi - delta)/pi, B_m = W o sqrt(1 - c^2)/pi, u1 = B_m q2,
    u2 = B_m^T q1, M = x1^T A_w x2 + x1^T diag(u1/2q1 + t) x1 + x2^T diag(u2/2q2) x2, g_p = <dC_p, sym M>,
    g_sigma0 = sigma0 (2 sum A_w + sum u1/q1 + sum u2/q2).  Their errors against ``pullback_ld`` are the floor."""
    s0 = float(sigma0)
    theta = {"sigma_0": s0}
    x1, x2, W = orc._t(x1), orc._t(x2), orc._t(W)
    tt = orc._t(t) if t is not None else torch.zeros(x1.shape[0], dtype=torch.float64)
    _, dK = orc.arccos_gram(theta, x1, x2, C, dC)
    _, dKv = orc.arccos_gram_diag(theta, x1, C, dC)
    direct = {k: float((W * dK[k]).sum() + (0.0 if k == "sigma_0" else (tt * dKv[k]).sum())) for k in KEYS}
    q1 = torch.sqrt(((x1 @ C) * x1).sum(1) + s0 * s0)
    q2 = torch.sqrt(((x2 @ C) * x2).sum(1) + s0 * s0)
    cosd = torch.clip(((x1 @ C) @ x2.T + s0 * s0) / (torch.outer(q1, q2) + 1e-7), -1, 1)
    delta = torch.arccos(cosd)
    Aw = W * (orc.PI32 - delta) / orc.PI32
    Bm = W * torch.sqrt(1 - cosd * cosd) / orc.PI32
    u1, u2 = Bm @ q2, Bm.T @ q1
    M = x1.T @ (Aw @ x2) + x1.T @ ((u1 / (2 * q1) + tt)[:, None] * x1) + x2.T @ ((u2 / (2 * q2))[:, None] * x2)
    M = (M + M.T) / 2
    adjoint = {k: float((dC[k] * M).sum()) for k in DCK}
    adjoint["sigma_0"] = float(s0 * (2 * Aw.sum() + (u1 / q1).sum() + (u2 / q2).sum()))
    return direct, adjoint


def f64(a):
    return np.asarray(a, dtype=np.float64)


def tile_relerr(a, b, tile=TILE):
    """``relerr`` over the whole matrix and over every tile x tile block of it (each scaled by its own largest
    reference entry), the largest of them: a wrong corner tile cannot hide under the largest entry of the matrix."""
    a, b = f64(a), f64(b)
    assert a.shape == b.shape
    worst = relerr(a, b)
    if a.ndim == 2:
        for i in range(0, a.shape[0], tile):
            for j in range(0, a.shape[1], tile):
                worst = max(worst, relerr(a[i:i + tile, j:j + tile], b[i:i + tile, j:j + tile]))
    return worst


@functools.lru_cache(maxsize=None)
def acos_reference(name):
    s0, x1, x2, C, dC = acos_inputs(name)
    return acosker_ld(s0, x1, x2, C, dC)


@functools.lru_cache(maxsize=None)
def diag_reference(name):
    s0, x1, C, dC = diag_inputs(name)
    return acosker_diag_ld(s0, x1, C, dC)


@functools.lru_cache(maxsize=None)
def pullback_reference(name, with_t):
    s0, x1, x2, C, dC, W, t = pullback_inputs(name)
    return pullback_ld(s0, x1, x2, C, dC, W, t if with_t else None)


# ------------------------------------------------------------------ nd_utility in mpmath (utils.py:414-525)
def nd_utility_mp(sigma2, mu, r, digits=50):
    """U, H(r|x,D), <H(r|f,x)>, p and log p of ``nd_utility`` at ``digits`` digits, Lambert W from mpmath.  The
    reference zeroes a term exactly where the fp64 value exp(r sigma2 + mu) sigma2 is inf (utils.py:448-450, 492-493):
    that decision is taken in fp64, as the reference takes it; everything else is mpmath on the fp64 inputs.

    The reference writes log(e sigma2 + 1), not log1p: in fp64 the term is lost once e sigma2 < 1e-16 (mu below about
    -37), and every overflowed term repeats the loss -- 1e-2 of |H_r| + |H_mean| at (sigma2, mu) = (10, -50), where U
    is 1e-19.  That is the reference's arithmetic; oracle and kernel restate it.  At ``digits`` = 50 the same sum
    rounds the same way only below 1e-50, so the chosen points have mu > -37 or mu < -600 (z ~ 1e-300 and below),
    never in between, where fp64 has no floor worth the name."""
    import mpmath as mp
    sigma2, mu, r = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (sigma2, mu, r))
    with np.errstate(over="ignore"):
        keep = np.exp(np.outer(r, sigma2) + mu[None, :]) * sigma2[None, :] != np.inf
    out = {k: np.zeros(sigma2.size) for k in ("U", "H_r", "H_mean")}
    out["p"], out["logp"] = np.zeros(keep.shape), np.zeros(keep.shape)
    with mp.workdps(digits):
        for i in range(sigma2.size):
            s2, m = mp.mpf(float(sigma2[i])), mp.mpf(float(mu[i]))
            H_r, plrf = mp.mpf(0), mp.mpf(0)
            for k in range(r.size):
                if keep[k, i]:
                    rk = mp.mpf(float(r[k]))
                    rs = rk * s2
                    z = mp.exp(rs + m) * s2                          # :445
                    lrf = mp.loggamma(rk + 1)                        # :484
                else:
                    rk = rs = z = lrf = mp.mpf(0)                    # :449-450, 492-493
                lam = rs + m - (mp.lambertw(z) if z != 0 else 0)     # :466
                e = mp.exp(lam)
                logp = lam * rk - e - (lam - m) ** 2 / (2 * s2) - mp.log(e * s2 + 1) / 2 - lrf   # :496
                p = mp.exp(logp)
                H_r -= p * logp                                      # :519
                plrf += p * lrf                                      # :429
                out["p"][k, i], out["logp"][k, i] = float(p), float(logp)
            H_mean = -mp.exp(m + s2 / 2) * (m + s2 - 1) + plrf       # :432
            out["U"][i], out["H_r"][i], out["H_mean"][i] = float(H_r - H_mean), float(H_r), float(H_mean)
    return out


def utility_points():
    """About 40 chosen (sigma2, mu) pairs for r = 0 .. 99: with z = exp(r sigma2 + mu) sigma2,
    z on either side of 2 (the seam of the Lambert W start value), z ~ 1e-300, z = 0 by underflow, z ~ 1e300,
    candidates in which some terms overflow and a candidate in which every term with r >= 1 does."""
    pts = []
    ln2 = float(np.log(2.0))
    for eps in (-1e-3, -1e-9, 1e-9, 1e-3):             # r = 0: z = 2 (1 + eps), sigma2 = 1
        pts.append((1.0, ln2 + eps))
    for eps in (-1e-6, 1e-6):                          # the seam crossed at r = 7: 7 * 0.25 + mu = ln 8 + eps
        pts.append((0.25, float(np.log(8.0)) - 1.75 + eps))
    pts += [(1.0, -690.7), (0.5, -690.0), (2.0, -700.0)]             # z ~ 1e-300 at small r
    pts += [(1.0, -760.0), (0.3, -800.0), (3.0, -1200.0)]            # z = 0 by underflow (for every r, or for small r)
    pts += [(7.0, 0.0), (6.95, 2.5), (1.0, 690.0), (0.5, 690.5)]     # z ~ 1e300
    pts += [(8.0, 0.0), (10.0, -5.0), (7.2, -3.0), (20.0, -12.0), (3.0, 500.0)]     # some terms overflow
    pts += [(800.0, 0.0), (710.0, -0.5)]                             # every term with r >= 1 overflows
    # the ordinary range of the notebook, small and large variances
    pts += [(1e-3, -7.0), (1e-3, 2.5), (0.05, -3.0), (0.37, -1.1), (0.9, 0.0), (1.5, 1.0), (3.0, -7.0), (3.0, 2.5),
            (2.0, -2.0), (1e-6, 0.5), (5.0, -4.0), (0.2, 3.5), (1e-2, 4.0), (4.0, 1.0)]
    s2, mu = (np.array(v, dtype=np.float64) for v in zip(*pts))
    return s2, mu, np.arange(100, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def utility_reference():
    return nd_utility_mp(*utility_points())


UTILITY_NR = (1, 127, 128, 129, 300)      # response counts on either side of the 128-thread stride of the kernel
_SEAM_BASE = ((0.37, -1.1), (1e-3, 2.5), (3.0, -7.0), (1.5, 1.0), (0.05, -3.0), (2.4, 2.0), (0.9, 0.0))


def utility_seam_points(nr, nstar):
    """``nstar`` candidates cycling through seven pairs of the notebook's range (so that seven mpmath evaluations
    are the reference of every candidate), r = 0 .. nr - 1."""
    s2, mu = (np.array(v, dtype=np.float64) for v in zip(*_SEAM_BASE))
    idx = np.arange(nstar) % len(_SEAM_BASE)
    return s2[idx], mu[idx], np.arange(nr, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def utility_seam_reference(nr):
    return nd_utility_mp(*utility_seam_points(nr, len(_SEAM_BASE)))


def utility_err(U, ref):
    """|U - U_ref| scaled by |H_r| + |H_mean|: U is their difference."""
    den = np.maximum(np.abs(ref["H_r"]) + np.abs(ref["H_mean"]), 1e-300)
    return float(np.max(np.abs(f64(U) - ref["U"]) / den))


# ------------------------------------------------------------------ the CPU tests
def _floor_table():
    import test_gpu_kernel_shapes as shapes   # the table lives at the top of the GPU module
    return shapes.FLOOR


def _check_floor(name, quantity, measured):
    """The table holds the measured floor: what is measured here lies within a factor of two of it on either side
    (another BLAS or thread count moves the figure; that variation is absorbed here, not in the kernel's bar).
    Figures below one rounding of fp64 count as one rounding."""
    recorded = _floor_table()[name][quantity]
    print(f"floor {name} {quantity}: measured {measured:.3e} recorded {recorded:.3e} bar {bar(quantity, recorded):.3e}")
    lo = 0.0 if quantity == "pullback" else 2.0 ** -53      # (the pull-back's scale is a sum of absolute values)
    assert max(recorded, lo) / 2.0 <= max(measured, lo) <= 2.0 * max(recorded, lo), (name, quantity, measured, recorded)
    if quantity in ("pullback", "U"):
        assert bar(quantity, recorded) <= LOOSEST


def test_longdouble_acosker_matches_golden():
    """The longdouble restatement against the real reference's own output (G2): square, rectangular, one row,
    diagonal, duplicate rows; K and the six dK."""
    g = load_golden("g2_acosker.npz")
    theta = dict(zip(KEYS, g["theta"]))
    C, mask, dC = orc.spatial_metric(theta, LOWER, UPPER, int(g["n_px"]), grad=True)
    m = mask.numpy()
    s0 = theta["sigma_0"]
    X, X2, X1 = g["X"][:, m], g["X2"][:, m], g["X1row"][:, m]
    K, dK = acosker_ld(s0, X, X, C, dC)
    assert relerr(f64(K), g["Ksq"]) < 1e-12
    assert np.array_equal(K, K.T)
    for k in KEYS:
        assert relerr(f64(dK[k]), g[f"dKsq_{k}"]) < 1e-11, k
    K, dK = acosker_ld(s0, X, X2, C, dC)
    assert relerr(f64(K), g["Krc"]) < 1e-12
    for k in KEYS:
        assert relerr(f64(dK[k]), g[f"dKrc_{k}"]) < 1e-11, k
    assert relerr(f64(acosker_ld(s0, X1, X, C)[0]), g["K1"]) < 1e-12
    Kv, dKv = acosker_diag_ld(s0, X, C, dC)
    assert relerr(f64(Kv), g["Kv"]) < 1e-13
    assert relerr(f64(acosker_diag_ld(s0, X1, C)[0]), g["Kv1"]) < 1e-13
    for k in KEYS:
        assert relerr(f64(dKv[k]), g[f"dKv_{k}"]) < 1e-12, k
    Xd = g["X"].copy()
    Xd[1] = Xd[0]
    Xd[2] = -Xd[0]
    assert relerr(f64(acosker_ld(s0, Xd[:, m], Xd[:, m], C)[0]), g["Kdup"]) < 1e-12


@pytest.mark.parametrize("name", [c[0] for c in ACOS_CASES])
def test_oracle_acosker_floor(name):
    """The fp64 oracle against the longdouble restatement at the shapes of the GPU module, over the whole matrix
    and per 128 x 128 tile: the oracle's own error, from which the kernel's bar is set."""
    s0, x1, x2, C, dC = acos_inputs(name)
    K, dK = acos_reference(name)
    out = orc.arccos_gram({"sigma_0": s0}, x1, x2, C, dC)
    Ko, dKo = out if dC is not None else (out, None)
    _check_floor(name, "K", tile_relerr(Ko.numpy(), K))
    assert tile_relerr(Ko.numpy(), K) < PROJECT_BAR["K"]
    if dC is not None:
        e = max(tile_relerr(dKo[k].numpy(), dK[k]) for k in KEYS)
        _check_floor(name, "dK", e)
        assert e < PROJECT_BAR["dK"]
        if x1.shape[0] == x2.shape[0] and x1 is not x2:
            assert not np.array_equal(dK["Amp"], dK["Amp"].T)      # dK is not symmetrised
    if x1.shape[0] == x2.shape[0]:
        assert np.array_equal(K, K.T)
    if name.startswith("clip"):              # the fp64 cosine does reach +-1, in an off-diagonal tile among others
        q = np.sqrt(((x1 @ C.numpy()) * x1).sum(1) + s0 * s0)
        c = np.clip(((x1 @ C.numpy()) @ x1.T + s0 * s0) / (np.outer(q, q) + 1e-7), -1, 1)
        i, j = np.nonzero(np.abs(c) == 1.0)
        assert np.any(i // TILE != j // TILE)


@pytest.mark.parametrize("name", [c[0] for c in DIAG_CASES])
def test_oracle_acosker_diag_floor(name):
    s0, x1, C, dC = diag_inputs(name)
    Kv, dKv = diag_reference(name)
    Kvo, dKvo = orc.arccos_gram_diag({"sigma_0": s0}, x1, C, dC)
    _check_floor(name, "Kvec", relerr(Kvo.numpy(), f64(Kv)))
    _check_floor(name, "dKvec", max(relerr(dKvo[k].numpy(), f64(dKv[k])) for k in KEYS))


def pullback_err(g, ref, scale):
    return max(abs(float(LD(g[k]) - ref[k])) / float(scale[k]) for k in KEYS)


@pytest.mark.parametrize("name", [c[0] for c in PULLBACK_CASES])
def test_host_pullback_floor(name):
    """Two fp64 host evaluations of the pull-back (materialised dK; adjoint form) against the longdouble
    contraction, each component scaled by what was added up: the larger error is the floor.  Also pins the adjoint
    algebra of the entry point's contract to the reference's materialised derivatives."""
    s0, x1, x2, C, dC, W, t = pullback_inputs(name)
    worst = 0.0
    for with_t in (False, True):
        ref, scale = pullback_reference(name, with_t)
        direct, adjoint = pullback_f64(s0, x1, x2, C, dC, W, t if with_t else None)
        worst = max(worst, pullback_err(direct, ref, scale), pullback_err(adjoint, ref, scale))
    _check_floor(name, "pullback", worst)


def test_mpmath_utility_matches_golden():
    """The mpmath restatement against the real reference's nd_utility (scipy's Lambert W) on G8: U for r = 0..99 and
    for the shorter list, the 0-d call form, p and log p of every term."""
    g = load_golden("g8_nd_utility.npz")
    ref = nd_utility_mp(g["sigma2"], g["mu"], g["r"])
    assert utility_err(g["U"], ref) < 1e-12
    assert np.max(np.abs(ref["U"] - g["U"]) / np.abs(g["U"])) < 1e-9      # the bar of test_nd_utility_matches_reference
    assert relerr(ref["p"], g["p"]) < 1e-12
    assert np.max(np.abs(ref["logp"] - g["logp"]) / np.maximum(np.abs(g["logp"]), 1.0)) < 1e-12
    short = nd_utility_mp(g["sigma2"], g["mu"], g["r_short"])
    assert utility_err(g["U_short"], short) < 1e-12
    one = nd_utility_mp(g["sigma2_scalar"], g["mu_scalar"], g["r"])
    assert abs(one["U"][0] - float(g["U_scalar"][0])) < 1e-12


def test_oracle_utility_floor():
    """The fp64 oracle (Fritsch iteration) against mpmath on the chosen points: the floor of U."""
    s2, mu, r = utility_points()
    ref = utility_reference()
    with np.errstate(over="ignore"):
        z = np.exp(np.outer(r, s2) + mu[None, :]) * s2[None, :]
    over = np.isinf(z)
    assert np.any(over.any(0) & ~over[1:].all(0))                  # some terms overflow, not all
    assert np.any(over[1:].all(0) & ~over[0])                      # every term with r >= 1 overflows
    assert np.any((z > 0) & (z < 1e-299)) and np.any(z == 0) and np.any((z > 1e299) & ~over)
    assert np.any((z > 2 - 1e-5) & (z < 2)) and np.any((z > 2) & (z < 2 + 1e-5))
    assert np.all(np.isfinite(ref["U"]))
    _check_floor("utility", "U", utility_err(orc.active_utility(s2, mu, r).numpy(), ref))


@pytest.mark.parametrize("nr", UTILITY_NR)
def test_oracle_utility_floor_by_response_count(nr):
    s2, mu, r = utility_seam_points(nr, len(_SEAM_BASE))
    _check_floor(f"utility-nr{nr}", "U", utility_err(orc.active_utility(s2, mu, r).numpy(), utility_seam_reference(nr)))
