"""The closure without the top-level block of the inverse Cholesky factor.  Run with `-m gpu` on an MI355X.

K~'s chain of the fused unit asks the recursion for the inverses of the two diagonal halves only; T, W and the
mean's solves substitute with the factor's own block L21 instead of multiplying by [L^-1]21 (padded sizes from
2048 up; below, the full inverse factor is the faster form and stays).  What the existing
parity and group tests do not cover: the executed flops really fall by the two merge products, and a group whose
top node splits unevenly."""
import numpy as np
import pytest
import torch

from gaussian_processes_amd import synthetic as syn
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu
KEYS = syn.THETA_KEYS
LOWER, UPPER = syn.limits()
LOGA, LAM0 = syn.F_PARAMS["logA"], syn.F_PARAMS["lambda0"]

# gemm_flops + small_gemm_flops + gram_flops of one evaluation with gradients (set_profile(1)) on commit 3dfc8ae,
# the last one whose closure formed the full inverse factor; inputs as in executed_flops() below
PARENT_COMMIT = "3dfc8ae"
PARENT_EXECUTED = {2048: 30206328832.0, 4096: 210460737536.0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


def T(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def cells(N, d, n_cells, dev):
    grid = syn.grid_for(d)
    X = T(syn.stimuli(N, d))
    out = []
    for c in range(n_cells):
        r_np, m_np = syn.cell_inputs(N, c)
        th0 = syn.theta0(c)
        C0, mask0 = orc.spatial_metric(th0, LOWER, UPPER, grid)
        V = 0.5 * orc.arccos_gram(th0, X[:, mask0], X[:, mask0], C0)
        out.append((T(r_np).to(dev), T(m_np).to(dev), V.to(dev), syn.theta_eval(c)))
    return grid, X.to(dev), out


def executed_flops(N, d, dev):
    from gaussian_processes_amd.engine import GPFitEngine
    grid, X, inp = cells(N, d, 1, dev)
    r, m, V, th = inp[0]
    eng = GPFitEngine(N, d)
    try:
        eng.fit_eval(th, LOWER, UPPER, grid, X, r, m, V, LOGA, LAM0, want_vectors=False)
        eng.set_profile(1)
        eng.fit_eval(th, LOWER, UPPER, grid, X, r, m, V, LOGA, LAM0, want_vectors=False)
        p = eng.get_profile()
        eng.set_profile(0)
    finally:
        eng.close()
    return p["gemm_flops"] + p["small_gemm_flops"] + p["gram_flops"]


@pytest.mark.parametrize("N", [2048, 4096])
def test_executed_flops_fall_by_the_merge_products(dev, N):
    """The two products of the top node's inverse merge, B = -C (L21 A), are gone: 2 n1^2 n2 algorithmic flops
    (n1, n2 the top split), and at 128-tile granularity T and W execute the same tile products in both forms.  The
    factor 0.9 leaves room for launches whose tile size changes when they lose their batch."""
    k = N // 128
    n1 = (k + 1) // 2 * 128
    n2 = N - n1
    got = executed_flops(N, 128, dev)
    print(f"executed flops N={N}: parent {PARENT_EXECUTED[N]:.6e} ({PARENT_COMMIT})  now {got:.6e}  "
          f"drop {PARENT_EXECUTED[N] - got:.6e}  required {0.9 * 2.0 * n1 * n1 * n2:.6e}")
    assert PARENT_EXECUTED[N] - got >= 0.9 * 2.0 * n1 * n1 * n2


def test_group_with_an_unequal_top_split(dev):
    """N = 2100 (padded 2176: seventeen 128-blocks, top split 1152 + 1024; the smallest sizes keep the full inverse
    factor, so an unequal split of the block form needs a size from 2048 up).  A group of 3 against the same units
    one by one (same bits) and against the CPU oracle (tolerances of tests/test_gpu_parity.py: 1e-9 on the loss
    terms, 1e-6 on the gradients)."""
    from gaussian_processes_amd.engine import GPFitEngine, fit_eval_group
    N, d, units = 2100, 64, 3
    grid, X, inp = cells(N, d, units, dev)
    engs = [GPFitEngine(N, d) for _ in range(units)]
    try:
        alone = [engs[0].fit_eval(th, LOWER, UPPER, grid, X, r, m, V, LOGA, LAM0, want_vectors=False) for r, m, V, th in inp]
        grouped = fit_eval_group(engs, [t[3] for t in inp], LOWER, UPPER, grid, X, [t[0] for t in inp], [t[1] for t in inp],
                                 [t[2] for t in inp], LOGA, LAM0)
    finally:
        for e in engs:
            e.close()
    names = ("loss", "loglik", "KL", "logdet_K", "logdet_V", "tr_KinvV", "mKinvm")
    for a, g in zip(alone, grouped):
        assert [float(a[k]).hex() for k in names] == [float(g[k]).hex() for k in names]
        assert [float(a["grad"][k]).hex() for k in KEYS] == [float(g["grad"][k]).hex() for k in KEYS]
    for (r, m, V, th), g in zip(inp, grouped):
        loss, grad, p = orc.mstep_closure_cholesky(th, LOWER, UPPER, grid, X.cpu(), r.cpu(), m.cpu(), V.cpu(), LOGA, LAM0,
                                                   want_parts=True)
        print(f"N=2100 group: loss {g['loss']!r} oracle {float(loss)!r}")
        for got, ref in ((g["loss"], loss), (g["loglik"], p["loglik"]), (g["KL"], p["KL"])):
            assert abs(got - float(ref)) <= 1e-9 * abs(float(ref))
        ref = np.array([grad[k] for k in KEYS])
        got = np.array([g["grad"][k] for k in KEYS])
        assert np.abs(ref - got).max() <= 1e-6 * np.abs(ref).max()


SPLIT_SCRIPT = r"""
import json, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from gaussian_processes_amd import synthetic as syn
from gaussian_processes_amd.engine import GPFitEngine, fit_eval_group
from oracle import gp_oracle as orc
N, d, units = 640, 64, 3
dev = torch.device("cuda:0")
KEYS = syn.THETA_KEYS
LOWER, UPPER = syn.limits()
LOGA, LAM0 = syn.F_PARAMS["logA"], syn.F_PARAMS["lambda0"]
T = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
grid = syn.grid_for(d)
X = T(syn.stimuli(N, d))
inp = []
for c in range(units):   # as cells() of the test module
    r_np, m_np = syn.cell_inputs(N, c)
    th0 = syn.theta0(c)
    C0, mask0 = orc.spatial_metric(th0, LOWER, UPPER, grid)
    V = 0.5 * orc.arccos_gram(th0, X[:, mask0], X[:, mask0], C0)
    inp.append((T(r_np).to(dev), T(m_np).to(dev), V.to(dev), syn.theta_eval(c)))
X = X.to(dev)
engs = [GPFitEngine(N, d) for _ in range(units)]
alone = [engs[0].fit_eval(th, LOWER, UPPER, grid, X, r, m, V, LOGA, LAM0, want_vectors=False) for r, m, V, th in inp]
grouped = fit_eval_group(engs, [t[3] for t in inp], LOWER, UPPER, grid, X, [t[0] for t in inp], [t[1] for t in inp],
                         [t[2] for t in inp], LOGA, LAM0)
names = ("loss", "loglik", "KL", "logdet_K", "logdet_V", "tr_KinvV", "mKinvm")
flat = lambda o: [float(o[k]).hex() for k in names] + [float(o["grad"][k]).hex() for k in KEYS]
print("RESULT " + json.dumps({"alone": [flat(o) for o in alone], "grouped": [flat(o) for o in grouped]}))
"""


def test_recursive_two_sided_product_at_640(dev, tmp_path):
    """The recursive two-sided product (two_sided_list's split), which the default GPFIT_TS_MIN = 4096 keeps out of
    every other test's reach: with GPFIT_TS_MIN=256 (read once, hence a process of its own) N = 640 walks
    640 -> 384 + 256 -> 256 + 128 -> 128 + 128, i.e. the unequal halves and the shared list of 2 cnt equal halves.  A
    group of 3 against the same units one by one (same bits: loss, log-likelihood, KL, the four diagnostics, the six
    gradients), the split's own products in the launch log, and every unit against the CPU oracle (tolerances of tests/test_gpu_parity.py: 1e-9 on the loss terms,
    1e-6 of the largest component on the gradients)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "split.py"
    script.write_text(SPLIT_SCRIPT)
    env = dict(os.environ, GPFIT_TS_MIN="256", GPFIT_GEMM_LOG="1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, str(script), root], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    # the split was really taken: its first product, Z21 = 1/2 Q22 B (256 x 384 x 256, Q read k-major, dense), is in the
    # launch log of the first evaluation -- at the top level and, with N 128 K 256, one level down
    import re
    log = [ln for ln in res.stderr.splitlines() if "[gpfit gemm]" in ln]
    for shape in ("M 256 N 384 K 256", "M 128 N 256 K 128"):
        assert [ln for ln in log if re.search(shape + r" atri 0 btri 0 lower 0 nb 1 tile \d+ ak 1 bk 1 epi 0 .* alpha 0\.5 beta 0 ", ln)], shape
    got = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    assert got["alone"] == got["grouped"]
    N, d, units = 640, 64, 3
    grid, X, inp = cells(N, d, units, torch.device("cpu"))
    for (r, m, V, th), row in zip(inp, got["alone"]):
        loss, grad, p = orc.mstep_closure_cholesky(th, LOWER, UPPER, grid, X, r, m, V, LOGA, LAM0, want_parts=True)
        vals = [float.fromhex(h) for h in row]
        print(f"N=640 TS_MIN=256: loss {vals[0]!r} oracle {float(loss)!r}")
        for gotv, ref in ((vals[0], loss), (vals[1], p["loglik"]), (vals[2], p["KL"])):
            assert abs(gotv - float(ref)) <= 1e-9 * abs(float(ref))
        ref = np.array([grad[k] for k in KEYS])
        assert np.abs(ref - np.array(vals[7:])).max() <= 1e-6 * np.abs(ref).max()
