"""The gradient pull-back in its Lambda form (csrc/fit.hip: adjoint_pass, lambda_t_x_list, pullback_to_metric).

The adjoint pass stores Lambda = tril(A_w, -1) + 1/2 diag(A_w) on the lower 64-tiles only and the metric matrix is
M = G + G^T with G = Xm^T (Lambda^T Xm + 1/2 diag(t) Xm).  Checked here, for the two closures that share the stage
(gpfit_fit_eval and gpfit_grad_pullback; the truncated-rank closures call the same pullback_to_metric):

 * M and the six gradients against a torch fp64 evaluation of Xm^T (A_w + diag t) Xm formed from the library's own W,
   cos(delta), b, q and t (read back through gpfit_dev_ctx_copy).  The bound is derived, not chosen: with
   gamma_n = n u / (1 - n u), u = 2^-53,
       |M - M_ref| <= 2 gamma_N (|Xm|^T (|A_w| + diag |t|) |Xm|)          (elementwise)
   the componentwise bound of an N-term fp64 product, once for the library and once for the reference, as
   tests/test_gpu_gemm_schedules.py derives its bounds.  (It is the tight choice: the worst case of the two nested
   N-term sums would allow gamma_2N per side.  The entries of A_w differ between the two sides by a few u from
   acos / sqrt, far inside gamma_N for N >= 192.)  A metric gradient is <dC_p, M>, d^2 more terms:
       |g_p - g_p,ref| <= sum |dC_p| bound_M + 2 gamma_(d^2 + 16) sum |dC_p| |M_ref|
   (16: the operations behind one entry of dC_p, which the library rebuilds from C and the pixel coordinates).  The
   sigma_0 row is 2 sigma_0 (sum A_w + sum u / q - sum wl), three sums of at most N^2 terms over quantities the
   adjoint pass forms from N-term sums: bound 2 sigma_0 * 2 gamma_(N^2 + N) (sum |A_w| + sum (|B_m| q) / q + sum |wl|).
 * a unit alone and inside a group of 4 and of 16: every output bit for bit.
 * the parts of the work matrices the Lambda form never reads (the tiles of A above the diagonal, the slabs of the
   scratch matrix below a row panel's k range) filled with NaN before the call: outputs unchanged, bit for bit.
 * executed flops (gpfit_set_profile 1) at N = 2048: the pull-back product runs np^2 dp + 64 np dp flops -- half of the
   2 np^2 dp of the product with the full A_w plus the upper halves of the diagonal 64-tiles -- and no launch with the
   full matrix remains.
"""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from gaussian_processes_amd import _lib, synthetic as syn
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu
KEYS = syn.THETA_KEYS
LOWER, UPPER = syn.limits()
LOGA, LAM0 = syn.F_PARAMS["logA"], syn.F_PARAMS["lambda0"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI32 = 3.1415927410125732
U = 2.0 ** -53


def gamma(n):
    return n * U / (1 - n * U)


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


def key(o):
    return (float(o["loss"]).hex(), float(o["loglik"]).hex(), float(o["KL"]).hex()) + tuple(float(o["grad"][k]).hex() for k in KEYS) \
        + (float(o["logdet_K"]).hex(), float(o["logdet_V"]).hex(), float(o["tr_KinvV"]).hex(), float(o["mKinvm"]).hex())


@pytest.fixture(scope="module")
def engines():
    from gaussian_processes_amd.engine import GPFitEngine
    made = {}

    def get(n, d, count):
        have = made.setdefault((n, d), [])
        while len(have) < count:
            have.append(GPFitEngine(n, d))
        return have[:count]
    yield get
    for lst in made.values():
        for e in lst:
            e.close()


def read(eng, name, rows, cols, ld):
    """rows x cols doubles of the context's buffer `name` (leading dimension ld)."""
    t = torch.empty(rows * ld, dtype=torch.float64, device=eng.tdev)
    assert eng.lib.gpfit_dev_ctx_copy(eng._ctx, name.encode(), 0, t.data_ptr(), t.numel() * 8, 0) == 0, name
    return t.view(rows, ld)[:, :cols]


def poison(eng, *names):
    for n in names:
        assert eng.lib.gpfit_dev_ctx_fill(eng._ctx, n.encode(), 0xFF) == 0, n      # all ones: NaN as fp64 and as fp32


def sym_from_lower(L):
    return torch.tril(L) + torch.tril(L, -1).T


def check_against_torch(eng, wname, n, d, theta, grid, grad_lib, what):
    """M and the six gradients of the evaluation that just ran on `eng`, whose adjoint W sits in buffer `wname`."""
    np_ = (n + 127) // 128 * 128
    dp = (d + 31) // 32 * 32
    W = sym_from_lower(read(eng, wname, np_, np_, np_)[:n, :n])
    c = sym_from_lower(read(eng, "Cos", np_, np_, np_)[:n, :n])
    b, q, wl, t = (read(eng, v, 1, n, np_)[0] for v in ("bv", "q", "wl", "tvec"))
    Xm = read(eng, "Xm", np_, dp, dp)[:n, :d]
    M = read(eng, "Mmat", dp, dp, dp)
    assert torch.equal(M, M.T), what + ": M = G + G^T must be exactly symmetric"
    assert bool((M[d:, :] == 0).all()), what + ": padding of M"
    M = M[:d, :d]
    w = W - 0.5 * torch.outer(b, b)
    Aw = w * (PI32 - torch.acos(c)) / PI32
    Bm = w * torch.sqrt(1.0 - c * c) / PI32
    M_ref = Xm.T @ (Aw @ Xm + t[:, None] * Xm)
    bound_M = 2 * gamma(n) * (Xm.abs().T @ (Aw.abs() @ Xm.abs() + t.abs()[:, None] * Xm.abs()))
    worst = float(((M - M_ref).abs() / bound_M.clamp_min(1e-300)).max())
    print(f"{what}: worst |M - M_ref| / bound = {worst:.3e}   (max |M| {float(M_ref.abs().max()):.3e})")
    assert bool(((M - M_ref).abs() <= bound_M).all()), f"{what}: M misses its bound by {worst:.3e}"
    # t itself, as the adjoint pass leaves it (an N-term sum per entry, then one division and one subtraction)
    u_ref = Bm @ q
    t_ref = u_ref / q - wl
    bound_t = 2 * gamma(n + 2) * ((Bm.abs() @ q.abs()) / q.abs() + wl.abs())
    assert bool(((t - t_ref).abs() <= bound_t).all()), what + ": t"
    # the five metric rows
    _, _, dC = orc.spatial_metric(theta, LOWER, UPPER, grid, grad=True)
    for k in KEYS:
        if k == "sigma_0":
            s0 = float(theta[k])
            ref = 2 * s0 * (float(Aw.sum()) + float((u_ref / q).sum()) - float(wl.sum()))
            bound = 2 * abs(s0) * 2 * gamma(n * n + n) * (float(Aw.abs().sum()) + float(((Bm.abs() @ q.abs()) / q.abs()).sum()) + float(wl.abs().sum()))
        else:
            D = dC[k].to(M.device)
            ref = float((D * M_ref).sum())
            bound = float((D.abs() * bound_M).sum()) + 2 * gamma(d * d + 16) * float((D.abs() * M_ref.abs()).sum())
        got = grad_lib[k]
        print(f"{what}: grad[{k}] = {got:.15e}  ref {ref:.15e}  |diff| / bound = {abs(got - ref) / max(bound, 1e-300):.3e}")
        assert abs(got - ref) <= bound, f"{what}: grad[{k}] {got!r} vs {ref!r}, bound {bound:.3e}"


@pytest.mark.parametrize("N,d", [(192, 64), (1024, 64), (4096, 256)])
def test_fit_eval_metric_and_gradients(dev, engines, N, d):
    grid, X, inp = cells(N, d, 1, dev)
    r, m, V, th = inp[0]
    eng = engines(N, d, 1)[0]
    out = eng.fit_eval(th, LOWER, UPPER, grid, X, r, m, V, LOGA, LAM0, want_vectors=False)
    check_against_torch(eng, "Tbuf", N, out["d"], th, grid, out["grad"], f"fit_eval N {N} d {d}")


@pytest.mark.parametrize("N,d", [(192, 64), (1024, 64), (4096, 256)])
def test_grad_pullback_metric_and_gradients(dev, engines, N, d):
    """gpfit_grad_pullback with an arbitrary symmetric adjoint and gvec (what the truncated-rank closure hands it)."""
    grid, X, inp = cells(N, d, 1, dev)
    th = inp[0][3]
    eng = engines(N, d, 1)[0]
    g = torch.Generator().manual_seed(N + d)
    W = torch.randn(N, N, generator=g, dtype=torch.float64)
    W = ((W + W.T) / (2 * N)).to(dev)
    gvec = torch.randn(N, generator=g, dtype=torch.float64).to(dev)
    rows, cols = (grid, grid) if not isinstance(grid, (tuple, list)) else grid
    out6 = (ctypes.c_double * 6)()
    rc = eng.lib.gpfit_grad_pullback(eng._ctx, eng._stream(), _lib.darr([float(th[k]) for k in KEYS]), int(rows), int(cols),
                                     X.data_ptr(), X.stride(0), N, W.data_ptr(), W.stride(0), gvec.data_ptr(), out6)
    _lib.check(rc, "gpfit_grad_pullback")
    _, dcount = eng.mask(th, grid)
    check_against_torch(eng, "Wbuf", N, dcount, th, grid, {k: out6[i] for i, k in enumerate(KEYS)}, f"grad_pullback N {N} d {d}")


@pytest.mark.parametrize("N,d,units", [(192, 64, 4), (192, 64, 16), (1024, 64, 4), (1024, 64, 16), (4096, 256, 4)])
def test_unit_alone_equals_unit_in_group(dev, engines, N, d, units):
    from gaussian_processes_amd.engine import fit_eval_group
    grid, X, inp = cells(N, d, units, dev)
    engs = engines(N, d, units)
    alone = [engs[0].fit_eval(th, LOWER, UPPER, grid, X, r, m, V, LOGA, LAM0, want_vectors=False) for r, m, V, th in inp[:2]]
    grouped = fit_eval_group(engs, [t[3] for t in inp], LOWER, UPPER, grid, X, [t[0] for t in inp], [t[1] for t in inp],
                             [t[2] for t in inp], LOGA, LAM0)
    assert [key(a) for a in alone] == [key(g) for g in grouped[:2]]
    # mixed precision (fp32 gradient products): the same route on the single-precision copies
    alone32 = engs[0].fit_eval(inp[0][3], LOWER, UPPER, grid, X, *inp[0][:3], LOGA, LAM0, want_vectors=False, grad_precision="f32")
    grouped32 = fit_eval_group(engs, [t[3] for t in inp], LOWER, UPPER, grid, X, [t[0] for t in inp], [t[1] for t in inp],
                               [t[2] for t in inp], LOGA, LAM0, grad_precision="f32")
    assert key(alone32) == key(grouped32[0])


@pytest.mark.parametrize("N,d", [(192, 64), (1024, 64), (4096, 256)])
def test_never_read_parts_may_hold_nan(dev, engines, N, d):
    """Abuf (Lambda: only the lower 64-tiles are written and read) and Zbuf (the slab scratch: the two-sided product
    rewrites what it reads of it, the pull-back reads only the slabs it wrote) start as NaN."""
    grid, X, inp = cells(N, d, 1, dev)
    r, m, V, th = inp[0]
    eng = engines(N, d, 1)[0]
    for prec in ("native", "f32"):
        clean = eng.fit_eval(th, LOWER, UPPER, grid, X, r, m, V, LOGA, LAM0, want_vectors=False, grad_precision=prec)
        poison(eng, "Abuf")
        dirty = eng.fit_eval(th, LOWER, UPPER, grid, X, r, m, V, LOGA, LAM0, want_vectors=False, grad_precision=prec)
        assert key(clean) == key(dirty), prec
        assert all(math.isfinite(v) for v in dirty["grad"].values())
    # the externally supplied adjoint: both work matrices are the pull-back's alone
    g = torch.Generator().manual_seed(N)
    W = torch.randn(N, N, generator=g, dtype=torch.float64)
    W = ((W + W.T) / (2 * N)).to(dev)
    gvec = torch.randn(N, generator=g, dtype=torch.float64).to(dev)
    rows, cols = (grid, grid) if not isinstance(grid, (tuple, list)) else grid
    res = []
    for dirty in (False, True):
        if dirty:
            poison(eng, "Abuf", "Zbuf")
        out6 = (ctypes.c_double * 6)()
        rc = eng.lib.gpfit_grad_pullback(eng._ctx, eng._stream(), _lib.darr([float(th[k]) for k in KEYS]), int(rows), int(cols),
                                         X.data_ptr(), X.stride(0), N, W.data_ptr(), W.stride(0), gvec.data_ptr(), out6)
        _lib.check(rc, "gpfit_grad_pullback")
        res.append([float(v).hex() for v in out6])
        assert all(math.isfinite(v) for v in out6)
    assert res[0] == res[1]


FLOPS_SCRIPT = r"""
import json, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from gaussian_processes_amd import synthetic as syn
from gaussian_processes_amd.engine import GPFitEngine
from oracle import gp_oracle as orc
N, d = 2048, 256
dev = torch.device("cuda:0")
LOWER, UPPER = syn.limits()
grid = syn.grid_for(d)
T = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
X = T(syn.stimuli(N, d))
r, m = syn.cell_inputs(N, 0)
th0 = syn.theta0(0)
C0, mask0 = orc.spatial_metric(th0, LOWER, UPPER, grid)
V = 0.5 * orc.arccos_gram(th0, X[:, mask0], X[:, mask0], C0)
eng = GPFitEngine(N, d)
eng.set_profile(1)
out = eng.fit_eval(syn.theta_eval(0), LOWER, UPPER, grid, X.to(dev), T(r).to(dev), T(m).to(dev), V.to(dev),
                   syn.F_PARAMS["logA"], syn.F_PARAMS["lambda0"], want_vectors=False)
p = eng.get_profile()
print("RESULT " + json.dumps({"d": out["d"], "gemm": p["gemm_flops"], "small": p["small_gemm_flops"], "gram": p["gram_flops"]}))
"""


def test_executed_flops_at_2048(dev, tmp_path):
    """The launch log of the first evaluation (GPFIT_GEMM_LOG=1) and the profile's totals, in a process of their own
    (the log switch is read once per process)."""
    script = tmp_path / "flops.py"
    script.write_text(FLOPS_SCRIPT)
    env = dict(os.environ, GPFIT_GEMM_LOG="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    import json
    tot = json.loads(re.search(r"RESULT (.*)", res.stdout).group(1))
    N, np_, d = 2048, 2048, tot["d"]
    dp = (d + 31) // 32 * 32
    rows = [{k: float(v) for k, v in re.findall(r"(\w+) ([-+.\de]+)", ln.split("[gpfit gemm]")[1])}
            for ln in res.stderr.splitlines() if "[gpfit gemm]" in ln]
    assert len(rows) > 10
    # (the pair launches of the recursion log a line of their own shape, without the layout fields)
    pull = [r for r in rows if (r["M"], r["N"], r["K"], r.get("ak"), r.get("bk")) == (np_, dp, np_, 1, 1)]
    assert len(pull) == 1, pull
    p = pull[0]
    dp64 = (dp + 63) // 64 * 64                                       # whole 64-tiles are executed
    assert (p["atri"], p["btri"], p["lower"], p["tile"]) == (2, 0, 0, 64)
    # 2 * 64 * 64 * (k steps of the triangle of 64-tiles) = np^2 dp + 64 np dp: against the 2 np^2 dp of the product with
    # the full A_w the count falls by np^2 dp - 64 np dp (the upper halves of the diagonal tiles stay)
    want = float(np_ * np_ * dp64 + 64 * np_ * dp64)
    assert abs(p["flops"] - want) <= 1e-6 * want, (p["flops"], want)                  # (the log prints seven digits)
    full = 2.0 * np_ * np_ * dp64
    print(f"pull-back product: {p['flops']:.6e} flops executed, {full:.6e} with the full matrix: falls by {full - p['flops']:.6e}")
    # the profile counts exactly the logged launches plus the split-k product Xm^T Y (dp x dp x np on whole tiles)
    logged = sum(r["flops"] for r in rows)
    xty = tot["gemm"] + tot["small"] - logged
    tiles = {t: 2.0 * ((dp + t - 1) // t * t) ** 2 * np_ for t in (32, 64, 128)}
    assert any(abs(xty - v) <= 1e-5 * (tot["gemm"] + tot["small"]) for v in tiles.values()), (xty, tiles)
    # nothing else of the evaluation multiplies with an np x np operand read k-major: the full-matrix product is gone
    assert not [r for r in rows if r.get("ak") == 1 and r["K"] == np_ and r["M"] == np_ and r.get("atri") == 0]
    print(f"executed: gemm {tot['gemm']:.6e} + small {tot['small']:.6e} + gram {tot['gram']:.6e} = {tot['gemm'] + tot['small'] + tot['gram']:.6e}")
