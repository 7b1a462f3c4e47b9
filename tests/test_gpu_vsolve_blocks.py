"""The row solve of a chain that needs no inverse (V's chain of the closures), as a block substitution with the inverses
of the first half's own halves (fit.hip:potrf_lockstep, VSOLVE_MIN).  Run with `-m gpu` on an MI355X.

The default threshold (first halves from 4096 on) keeps the route out of every other test's reach, and the knob
GPFIT_VSOLVE_MIN is read once per process: child processes run the same matrices through gpfit_dev_potrf, one with
GPFIT_VSOLVE_MIN=256, one with the route off (0) and one with 256 on 128-tiles (GPFIT_T128_MIN=1).  Two chains, need = 0b01: chain 0 gets its full inverse and keeps
the single product, chain 1 is in neither mask and substitutes.  n = 512 (256 + 256, first half 128 + 128) and n = 640
(384 + 256, first half 256 + 128: unequal on both levels).  The matrices are diagonally dominant (condition number
below 3) with a fixed seed; the reference is numpy's float64 Cholesky.

The launch log is that of the calls before any evaluation of the process (GPFIT_GEMM_LOG=0: the hook is no evaluation,
so the count the knob is compared with stays 0)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import potrf_cases as pc

pytestmark = pytest.mark.gpu
SIZES = (512, 640)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import ctypes, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from gaussian_processes_amd import _lib, utils
lib = _lib.load()
ctx = utils.get_engine(640, 1)._ctx


def hook(mats, need):
    nb, n = len(mats), mats[0].shape[0]
    dA = torch.from_numpy(np.stack(mats)).cuda()
    dL, dLi, dT = (torch.full((nb, n, n), float("nan"), dtype=torch.float64, device="cuda") for _ in range(3))
    dinfo = torch.zeros(nb, dtype=torch.int32, device="cuda")
    ptrs = lambda t: (ctypes.c_void_p * nb)(*[t[b].data_ptr() for b in range(nb)])
    rc = lib.gpfit_dev_potrf(ctx, utils._stream(), 0, nb, ptrs(dA), ptrs(dL), ptrs(dLi), ptrs(dT), ptrs(dinfo), n, n, need, 0, 0)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert not dinfo.cpu().numpy().any()
    return dL.cpu().numpy(), dLi.cpu().numpy()


inp = np.load(sys.argv[2])
out = {}
for n in (512, 640):
    mats = [inp[f"A{n}_{b}"] for b in range(2)]
    print(f"MARK two {n}", file=sys.stderr, flush=True)
    L, Li = hook(mats, 0b01)
    print(f"MARK alone {n}", file=sys.stderr, flush=True)
    L1, _ = hook(mats[1:], 0)
    out[f"L{n}"], out[f"Li{n}_0"], out[f"alone{n}"] = np.tril(L), np.tril(Li[0]), np.tril(L1[0])
np.savez(sys.argv[3], **out)
"""


def dominant(n, seed):
    """Symmetric, every diagonal entry twice the absolute sum of the rest of its row plus one: eigenvalues within
    [d / 2, 3 d / 2] of each row's diagonal d by Gershgorin."""
    rng = np.random.default_rng(1000 * n + seed)
    M = rng.standard_normal((n, n))
    A = (M + M.T) / 2
    np.fill_diagonal(A, 0.0)
    np.fill_diagonal(A, 2.0 * np.abs(A).sum(axis=1) + 1.0)
    return A


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The child processes, once: {knob: (arrays, launch log lines by marker)} and the inputs.  "t128": the route on
    with GPFIT_T128_MIN=1, under which these sizes run on 128-tiles as the headline's launches do."""
    tmp = tmp_path_factory.mktemp("vsolve")
    mats = {f"A{n}_{b}": dominant(n, b) for n in SIZES for b in range(2)}
    np.savez(tmp / "in.npz", **mats)
    (tmp / "child.py").write_text(CHILD)
    got = {}
    for knob, extra in (("256", {}), ("0", {}), ("t128", {"GPFIT_T128_MIN": "1"})):
        env = dict(os.environ, GPFIT_VSOLVE_MIN="0" if knob == "0" else "256", GPFIT_GEMM_LOG="0",
                   PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **extra)
        res = subprocess.run([sys.executable, str(tmp / "child.py"), ROOT, str(tmp / "in.npz"), str(tmp / f"out{knob}.npz")],
                             env=env, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr[-2000:]
        log, key = {}, None
        for ln in res.stderr.splitlines():
            if ln.startswith("MARK "):
                key = ln[5:]
                log[key] = []
            elif "[gpfit gemm]" in ln and key:
                log[key].append(ln)
        got[knob] = (dict(np.load(tmp / f"out{knob}.npz")), log)
    return mats, got


@pytest.mark.parametrize("n", SIZES)
def test_backward_error_against_the_single_product(runs, n):
    """max |L L^T - A| / max |A| of chain 1 on both routes, and the factor against numpy's.  The new route must stay
    within 4 x the old route's figure and below 1e-12; the forward bound is that of test_gpu_potrf.py (1e-12: condition
    number below 3, n = 640, 2^-53).  Measured on the MI355X (2026-10-20), substitution | single product:
      n = 512   |L L^T - A| / |A| 1.335e-15 | 1.335e-15   |L - L_numpy| / |L_numpy| 8.401e-16 | 8.401e-16
      n = 640                     1.160e-15 | 1.160e-15                             6.306e-16 | 6.306e-16
    (equal to the digits shown, although the bits of the rows below the first half differ)."""
    mats, got = runs
    A = mats[f"A{n}_1"]
    ref = np.linalg.cholesky(A)
    new, old = got["256"][0][f"L{n}"][1], got["0"][0][f"L{n}"][1]
    e_new, e_old = pc.err_backward(new, A), pc.err_backward(old, A)
    f_new = float(np.max(np.abs(new - ref)) / np.max(np.abs(ref)))
    f_old = float(np.max(np.abs(old - ref)) / np.max(np.abs(ref)))
    print(f"n {n} chain 1: |L L^T - A| / |A| substitution {e_new:.3e}, single product {e_old:.3e}; "
          f"|L - L_numpy| / |L_numpy| substitution {f_new:.3e}, single product {f_old:.3e}")
    assert e_new <= 4 * e_old and e_new < 1e-12
    assert f_new < 1e-12
    # the chain that substitutes is really another computation below the first half
    assert not pc.same_bits(new, old)
    n1 = pc.top_block(n)
    assert pc.same_bits(new[:n1, :n1], old[:n1, :n1])


@pytest.mark.parametrize("n", SIZES)
def test_the_chain_with_the_full_inverse_keeps_its_bits(runs, n):
    """Chain 0 (need) takes the single product on both sides of the knob: L and L^-1 bit for bit."""
    _, got = runs
    on, off = got["256"][0], got["0"][0]
    assert pc.same_bits(on[f"L{n}"][0], off[f"L{n}"][0])
    assert pc.same_bits(on[f"Li{n}_0"], off[f"Li{n}_0"])


@pytest.mark.parametrize("n", SIZES)
def test_the_chain_alone_reproduces_its_lockstep_bits(runs, n):
    """Chain 1 as a batch of one (need = 0) against chain 1 of the batch of two, on either side of the knob."""
    _, got = runs
    for knob in ("256", "0"):
        arr = got[knob][0]
        assert pc.same_bits(arr[f"alone{n}"], arr[f"L{n}"][1]), knob


def _lines(log, M, N, K, atri, btri, alpha, beta):
    pat = re.compile(rf"\] M {M} N {N} K {K} atri {atri} btri {btri} lower 0 nb (\d+) .* alpha {alpha} beta {beta} ")
    return [int(m.group(1)) for m in map(pat.search, log) if m]


@pytest.mark.parametrize("n", SIZES)
def test_launch_log(runs, n):
    """With the knob on, the merge [L11^-1]21 = -S^-1 (R P^-1) of the top node's first half (h2 x h1 x h2, lower x
    dense, alpha -1) is issued for chain 0 alone (nb 1), with it off for both (nb 2); and the three products of the
    substitution are there, n2 x h1 x h1 and n2 x h2 x h2 against an upper-triangular op(B), n2 x h2 x h1 dense with
    alpha -1, beta 1 -- none of them with the knob off."""
    _, got = runs
    n1 = pc.top_block(n)
    n2, h1 = n - n1, pc.top_block(n1)
    h2 = n1 - h1
    on, off = got["256"][1][f"two {n}"], got["0"][1][f"two {n}"]
    # (at n = 512 the top node's second half has the same shape: its merge is chain 0's alone on both sides)
    assert 2 in _lines(off, h2, h1, h2, 1, 0, -1, 0)
    assert 2 not in _lines(on, h2, h1, h2, 1, 0, -1, 0) and 1 in _lines(on, h2, h1, h2, 1, 0, -1, 0)
    assert _lines(on, n2, h2, h1, 0, 0, -1, 1) == [1] and _lines(off, n2, h2, h1, 0, 0, -1, 1) == []
    assert 1 in _lines(on, n2, h1, h1, 0, 2, 1, 0) and 1 in _lines(on, n2, h2, h2, 0, 2, 1, 0)
    assert _lines(off, n2, h1, h1, 0, 2, 1, 0) == [] and _lines(off, n2, h2, h2, 0, 2, 1, 0) == []
    # the single product of the row solve: both chains in one launch with the knob off, chain 0 alone with it on
    assert _lines(off, n2, n1, n1, 0, 2, 1, 0) == [2] and _lines(on, n2, n1, n1, 0, 2, 1, 0) == [1]



@pytest.mark.parametrize("n", SIZES)
def test_half_width_solves_on_64_tiles(runs, n):
    """Where a half-width solve would be a 128-tile launch of less than two rounds of the chip it runs on 64-tiles (the
    headline's 4096 x 2048 solves; here with GPFIT_T128_MIN=1): the two solves are logged on tile 64, the dense update
    between them on tile 128, and both chains keep the bits they have on the launcher's own tiles."""
    _, got = runs
    n1 = pc.top_block(n)
    n2, h1 = n - n1, pc.top_block(n1)
    h2 = n1 - h1
    log = got["t128"][1][f"two {n}"]
    tile = lambda M, N, K, bt, alpha, beta: [int(m.group(1)) for m in map(re.compile(
        rf"\] M {M} N {N} K {K} atri 0 btri {bt} lower 0 nb 1 tile (\d+) .* alpha {alpha} beta {beta} ").search, log) if m]
    assert set(tile(n2, h1, h1, 2, 1, 0)) == {64} and set(tile(n2, h2, h2, 2, 1, 0)) == {64}
    assert tile(n2, h2, h1, 0, -1, 1) == [128]
    assert tile(n2, n1, n1, 2, 1, 0) == [128]   # chain 0's single product: more than one shape, the launcher's tile
    assert pc.same_bits(got["t128"][0][f"L{n}"], got["256"][0][f"L{n}"])
    assert pc.same_bits(got["t128"][0][f"Li{n}_0"], got["256"][0][f"Li{n}_0"])
