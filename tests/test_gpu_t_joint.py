"""T's lower row of blocks as one launch, [T21 | T22] = C [S | LV22], and S with LV21 added in its launch's epilogue
(fit.hip:t_in_blocks).  Run with `-m gpu` on an MI355X.

The joint launch is taken where it qualifies for the XCD-aware table, from 1536 tiles with a k range on: N = 8192.  Here it
is forced at N = 2048 (1024 + 1024) and N = 2100 (padded 2176, 1152 + 1024) by GPFIT_XCD_MIN_TILES=1 in a child process
(the knob is read once), with GPFIT_T128_MIN=1 so that the launches of these sizes run on 128-tiles, the only tile with a
table.  A second child sets GPFIT_T128_MIN=1 alone: the same launches except that T22 and T21 are the two launches they
were.  A third adds GPFIT_FUSED_EPI=7 to that: S from a copy of LV21 and beta = 1, the route before this launch sequence
and still the one of small tiles.  Per size and child: one evaluation without gradients, whose T is read back (with gradients the buffer is reused
by the two-sided product), one with gradients, and a group of three units against the same units one by one."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from gaussian_processes_amd import synthetic as syn
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu
KEYS = syn.THETA_KEYS
LOWER, UPPER = syn.limits()
LOGA, LAM0 = syn.F_PARAMS["logA"], syn.F_PARAMS["lambda0"]
SIZES = (2048, 2100)
D, UNITS = 64, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("loss", "loglik", "KL", "logdet_K", "logdet_V", "tr_KinvV", "mKinvm")

CHILD = r"""
import json, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from gaussian_processes_amd import synthetic as syn
from gaussian_processes_amd.engine import GPFitEngine, fit_eval_group
from oracle import gp_oracle as orc
d, units = 64, 3
dev = torch.device("cuda:0")
KEYS = syn.THETA_KEYS
LOWER, UPPER = syn.limits()
LOGA, LAM0 = syn.F_PARAMS["logA"], syn.F_PARAMS["lambda0"]
NAMES = ("loss", "loglik", "KL", "logdet_K", "logdet_V", "tr_KinvV", "mKinvm")
T = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
flat = lambda o: [float(o[k]).hex() for k in NAMES] + [float(o["grad"][k]).hex() for k in KEYS]
out, arrays = {}, {}
first = True
for N in (2048, 2100):
    grid = syn.grid_for(d)
    X = T(syn.stimuli(N, d))
    inp = []
    for c in range(units):   # as cells() of tests/test_gpu_top_inverse.py
        r_np, m_np = syn.cell_inputs(N, c)
        th0 = syn.theta0(c)
        C0, mask0 = orc.spatial_metric(th0, LOWER, UPPER, grid)
        V = 0.5 * orc.arccos_gram(th0, X[:, mask0], X[:, mask0], C0)
        inp.append((T(r_np).to(dev), T(m_np).to(dev), V.to(dev), syn.theta_eval(c)))
    X = X.to(dev)
    engs = [GPFitEngine(N, d) for _ in range(units)]
    r, m, V, th = inp[0]
    np_ = -(-N // 128) * 128
    # the launch log is that of the first evaluation of the process (GPFIT_GEMM_LOG=1)
    print(f"MARK first {N}" if first else f"MARK later {N}", file=sys.stderr, flush=True)
    first = False
    fwd = engs[0].fit_eval(th, LOWER, UPPER, grid, X, r, m, V, LOGA, LAM0, want_grad=False, want_vectors=False)
    t = torch.empty(np_ * np_, dtype=torch.float64, device=dev)
    assert engs[0].lib.gpfit_dev_ctx_copy(engs[0]._ctx, b"Tbuf", 0, t.data_ptr(), t.numel() * 8, 0) == 0
    arrays[f"T{N}"] = t.view(np_, np_).cpu().numpy()
    alone = [engs[0].fit_eval(th, LOWER, UPPER, grid, X, r, m, V, LOGA, LAM0, want_vectors=False) for r, m, V, th in inp]
    grouped = fit_eval_group(engs, [q[3] for q in inp], LOWER, UPPER, grid, X, [q[0] for q in inp], [q[1] for q in inp],
                             [q[2] for q in inp], LOGA, LAM0)
    out[str(N)] = {"fwd_trace": float(fwd["tr_KinvV"]).hex(), "alone": [flat(o) for o in alone], "grouped": [flat(o) for o in grouped]}
    for e in engs:
        e.close()
np.savez(sys.argv[2], **arrays)
print("RESULT " + json.dumps(out))
"""


def split(N):
    k = -(-N // 128)
    n1 = (k + 1) // 2 * 128
    return k * 128, n1, k * 128 - n1


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The children, once: {"joint" | "separate" | "copy": (results, T arrays, launch log of the first evaluation)}."""
    tmp = tmp_path_factory.mktemp("tjoint")
    (tmp / "child.py").write_text(CHILD)
    got = {}
    for name, extra in (("joint", {"GPFIT_XCD_MIN_TILES": "1"}), ("separate", {}), ("copy", {"GPFIT_FUSED_EPI": "7"})):
        env = dict(os.environ, GPFIT_T128_MIN="1", GPFIT_GEMM_LOG="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""),
                   **extra)
        res = subprocess.run([sys.executable, str(tmp / "child.py"), ROOT, str(tmp / f"{name}.npz")], env=env, capture_output=True,
                             text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-3000:]
        log, on = [], False
        for ln in res.stderr.splitlines():
            if ln.startswith("MARK "):
                on = ln.startswith("MARK first")
            elif on and ln.startswith("[gpfit "):
                log.append(ln)
        result = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
        got[name] = (result, dict(np.load(tmp / f"{name}.npz")), log)
    return got


@pytest.fixture(scope="module")
def oracle():
    """Unit 0 of each size on the CPU, once."""
    out = {}
    for N in SIZES:
        grid = syn.grid_for(D)
        X = torch.from_numpy(syn.stimuli(N, D))
        r_np, m_np = syn.cell_inputs(N, 0)
        th0 = syn.theta0(0)
        C0, mask0 = orc.spatial_metric(th0, LOWER, UPPER, grid)
        V = 0.5 * orc.arccos_gram(th0, X[:, mask0], X[:, mask0], C0)
        out[N] = orc.mstep_closure_cholesky(syn.theta_eval(0), LOWER, UPPER, grid, X, torch.from_numpy(r_np), torch.from_numpy(m_np), V,
                                            LOGA, LAM0, want_parts=True)
    return out


def test_the_launch_log_shows_the_new_sequence(runs):
    """First evaluation (N = 2048, n1 = n2 = 1024), T's part of the log: T11 alone (lower x lower, lower output), S with
    the added-matrix epilogue (epi 8, beta 0) and no rectangular copy, then ONE launch of 1024 x 2048 x 1024 with the
    split operand and the tile norms; the other child has T11 and T22 (two problems of that shape), S, and T21."""
    joint, separate = runs["joint"][2], runs["separate"][2]
    diag = re.compile(r"\] M 1024 N 1024 K 1024 atri 1 btri 1 lower 1 nb 1 tile 128 .* epi 2 ")
    s_line = re.compile(r"\] M 1024 N 1024 K 1024 atri 0 btri 1 lower 0 nb 1 tile 128 ak 0 bk 1 epi 8 .* alpha -1 beta 0 ")
    j_line = re.compile(r"\] M 1024 N 2048 K 1024 atri 1 btri 1 lower 0 nb 1 tile 128 ak 0 bk 1 epi 2 .* bsplit 1024$")
    t21 = re.compile(r"\] M 1024 N 1024 K 1024 atri 1 btri 0 lower 0 nb 1 tile 128 ak 0 bk 1 epi 2 ")
    count = lambda log, pat: sum(1 for ln in log if pat.search(ln))
    assert count(joint, diag) == 1 and count(joint, s_line) == 1 and count(joint, j_line) == 1 and count(joint, t21) == 0
    assert count(separate, diag) == 2 and count(separate, s_line) == 1 and count(separate, j_line) == 0 and count(separate, t21) == 1
    for log in (joint, separate):
        assert not [ln for ln in log if ln.startswith("[gpfit copy]")]
    # without epilogue 8: the copy, then S with beta = 1 and no epilogue
    copy = runs["copy"][2]
    s_beta = re.compile(r"\] M 1024 N 1024 K 1024 atri 0 btri 1 lower 0 nb 1 tile 128 ak 0 bk 1 epi 0 .* alpha -1 beta 1 ")
    assert len([ln for ln in copy if ln.startswith("[gpfit copy] rows 1024 cols 1024 ")]) == 1
    assert count(copy, s_beta) == 1 and count(copy, s_line) == 0 and count(copy, t21) == 1
    # in order: T11, S, the joint launch
    at = lambda pat: [i for i, ln in enumerate(joint) if pat.search(ln)][0]
    assert at(diag) < at(s_line) < at(j_line)


@pytest.mark.parametrize("N", SIZES)
def test_T_has_the_same_bits(runs, N):
    """Every 128-tile of T on or below the block diagonal, joint against separate launches: every data-parallel instance
    sums k in ascending order per element, so which launch computes a tile does not show.  (The strict upper tiles are
    never written by either.)"""
    a, b, c = (runs[name][1][f"T{N}"] for name in ("joint", "separate", "copy"))
    np_, n1, n2 = split(N)
    assert a.shape == b.shape == (np_, np_)
    tiles = np.kron(np.tril(np.ones((np_ // 128, np_ // 128), dtype=bool)), np.ones((128, 128), dtype=bool))
    assert np.all(np.isfinite(a[tiles]))
    assert a[tiles].tobytes() == b[tiles].tobytes()
    assert a[tiles].tobytes() == c[tiles].tobytes()   # LV21 added in the epilogue = copied and added with beta = 1
    assert float(np.abs(a[n1:, :n1]).max()) > 0 and float(np.abs(a[n1:, n1:][np.tril_indices(n2)]).max()) > 0


@pytest.mark.parametrize("N", SIZES)
def test_trace_loss_and_gradients(runs, oracle, N):
    """tr(K~^-1 V) = sum of the tile partials: the same positive partials in another order, so the two routes agree to
    2 (P - 1) 2^-53 relative, P the number of partials (T's lower tiles).  Loss terms and gradients of unit 0 against
    the CPU oracle to the tolerances of tests/test_gpu_parity.py (1e-9, 1e-6 of the largest component).
    Measured on the MI355X (2026-10-20): the two traces equal to the last bit at both sizes (962.8794353102631 and
    987.4284722654988); loss against the oracle 2e-16 and 3e-16 relative."""
    np_, n1, n2 = split(N)
    t1, t2 = n1 // 128, n2 // 128
    P = t1 * (t1 + 1) // 2 + t2 * (t2 + 1) // 2 + t1 * t2
    j, s = runs["joint"][0][str(N)], runs["separate"][0][str(N)]
    it = NAMES.index("tr_KinvV")
    tj, ts = float.fromhex(j["fwd_trace"]), float.fromhex(s["fwd_trace"])
    print(f"N {N}: tr_KinvV joint {tj!r} separate {ts!r} rel {abs(tj - ts) / abs(ts):.3e} (bound {2 * (P - 1) * 2.0 ** -53:.3e})")
    assert abs(tj - ts) <= 2 * (P - 1) * 2.0 ** -53 * abs(ts)
    tj, ts = float.fromhex(j["alone"][0][it]), float.fromhex(s["alone"][0][it])
    assert abs(tj - ts) <= 2 * (P - 1) * 2.0 ** -53 * abs(ts)
    loss, grad, p = oracle[N]
    vals = [float.fromhex(h) for h in j["alone"][0]]
    print(f"N {N}: loss {vals[0]!r} oracle {float(loss)!r}")
    for got, ref in ((vals[0], loss), (vals[1], p["loglik"]), (vals[2], p["KL"])):
        assert abs(got - float(ref)) <= 1e-9 * abs(float(ref))
    ref = np.array([grad[k] for k in KEYS])
    assert np.abs(ref - np.array(vals[len(NAMES):])).max() <= 1e-6 * np.abs(ref).max()


@pytest.mark.parametrize("N", SIZES)
def test_a_group_of_three_equals_its_single_calls(runs, N):
    """The group issues the joint launch unit by unit: the same bits as the single calls, in every child."""
    for name in ("joint", "separate", "copy"):
        res = runs[name][0][str(N)]
        assert res["alone"] == res["grouped"], name
