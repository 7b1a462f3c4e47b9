"""The rate-parameter L-BFGS port (csrc/lbfgs1d.h) against the installed torch's LBFGS, without a GPU.

gpfit_fparam_lbfgs_host runs the same template as the device kernel on host arrays.  The torch side is
torch.optim.LBFGS(lr=0.1, tolerance_change=1e-9, tolerance_grad=1e-7, line_search_fn='strong_wolfe',
history_size=max_iter) driving a float64 CPU closure with varGP's semantics (utils.py, E-step), built from the
oracle: call k evaluates at (logA_k, lambda0_{k-1}), then sets lambda0_k to the closed form at logA_k; lambda0_0 is
the closed form at the start; with loglambda0 every call uses the fixed exp(loglambda0); a non-finite sum f raises.

Two closures drive torch's side.  "sequential" sums in index order with libm's exp, as the host instance does, so
both sides see the same bits from every evaluation: then the port must reproduce torch exactly, and it does (counts,
final logA and lambda0, first and last loss all bit-equal in every case here).  "oracle" is built from
oracle.gp_oracle (expected_loglik(..., f_param_grad=True), lambda0_closed_form), which sums with torch.

Measured against the oracle closure (torch 2.10, the 100 cases of test_matches_torch_lbfgs): evaluation and
iteration counts equal in every case, first loss within 3e-15; final logA within 5.0e-8 and lambda0 within
6.6e-8 (relative to max(1, |x|)), last loss within 5.2e-8.  These are not last-bit: one ulp of difference in a
loss (torch's vectorised exp and summation order against libm's exp in index order) is amplified by the cubic
interpolation of the line search, 3 (f1 - f2) / (x1 - x2) with f1 ~ f2, into the steps that follow.  The same
amplification separates any two summation orders; the sequential runs show that the port adds none of its own.
ORACLE_X / ORACLE_LOSS are set about twenty times above the measured worst case.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.optim.lbfgs as torch_lbfgs

from gaussian_processes_amd import _lib
from gaussian_processes_amd.build import build_library
from oracle import gp_oracle as orc

TOL = 1e-13
ORACLE_X, ORACLE_LOSS = 1e-6, 1e-6   # measured worst 6.6e-8 / 5.2e-8: see the module docstring
LR, TOL_GRAD, TOL_CHANGE = 0.1, 1e-7, 1e-9


@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _lib.load()


def make_inputs(n, seed, logA_true=0.3, lambda0_true=-1.0):
    rng = np.random.default_rng(seed)
    lam_m = rng.standard_normal(n) * 0.8
    lam_var = rng.uniform(0.02, 0.3, n)
    A = math.exp(logA_true)
    r = rng.poisson(np.exp(A * lam_m + 0.5 * A * A * lam_var + lambda0_true)).astype(np.float64)
    if r.sum() == 0:
        r[0] = 1.0
    return lam_m, lam_var, r


def run_host(lib, lam_m, lam_var, r, logA0, max_iter, fixed=None):
    n = len(lam_m)
    out = (ctypes.c_double * 9)()
    f = np.empty(n)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.gpfit_fparam_lbfgs_host(ptr(lam_m), ptr(lam_var), ptr(r), n, logA0, 0 if fixed is None else 1,
                                     0.0 if fixed is None else fixed, max_iter, max_iter, LR, TOL_GRAD, TOL_CHANGE,
                                     ptr(f), out)
    assert rc == 0, _lib.last_error()
    o = list(out)
    return {"logA": o[0], "lambda0": o[1], "first_loss": o[2], "last_loss": o[3], "evals": int(o[4]),
            "iters": int(o[5]), "status": int(o[6]), "fail_logA": o[7], "fail_lambda0": o[8], "f": f}


def oracle_pass(lam_m, lam_var, r):
    """(loglik, dloglik/dlogA, sum f, closed-form lambda0) at (logA, lambda0) from the oracle (torch sums)."""
    lm, lv, rr = (torch.from_numpy(a) for a in (lam_m, lam_var, r))

    def ev(x, l0):
        A = math.exp(x)
        f = torch.exp(A * lm + 0.5 * A * A * lv + l0)
        L, g = orc.expected_loglik(rr, f, lm, lv, x, l0, f_param_grad=True)
        return float(L), float(g["logA"]), float(f.sum()), orc.lambda0_closed_form(x, rr, lm, lv)
    return ev


def cexp(v):
    """C's exp on a double: inf on overflow."""
    try:
        return math.exp(v)
    except OverflowError:
        return math.inf


def clog(v):
    """C's log on a double: -inf at 0, NaN below."""
    return -math.inf if v == 0 else (math.nan if not v > 0 else math.log(v))


def sequential_pass(lam_m, lam_var, r):
    """The same four numbers summed in index order with libm's exp, as gpfit_fparam_lbfgs_host sums them."""
    lm, lv, rr = lam_m.tolist(), lam_var.tolist(), r.tolist()
    sr = srm = 0.0
    for ri, mi in zip(rr, lm):
        sr += ri
        srm += ri * mi

    def ev(x, l0):
        A = cexp(x)
        se = sg = 0.0
        for mi, vi in zip(lm, lv):
            e = cexp(A * mi + 0.5 * A * A * vi)
            se += e
            sg += (mi + A * vi) * e
        el0 = cexp(l0)
        sf = se * el0
        closed = clog(sr) - clog(se)
        return A * srm + l0 * sr - sf, A * (srm - sg * el0), sf, closed
    return ev


def run_torch(lam_m, lam_var, r, logA0, max_iter, fixed=None, kind="oracle"):
    """varGP's E-step block (LBFGS over the rate-parameter closure); also what the line search did."""
    ev = (oracle_pass if kind == "oracle" else sequential_pass)(lam_m, lam_var, r)
    logA = torch.tensor(logA0, dtype=torch.float64, requires_grad=True)
    st = {"lambda0": ev(logA0, 0.0)[3], "calls": 0, "zoom": False, "ls_losses": []}
    opt = torch.optim.LBFGS([logA], lr=LR, max_iter=max_iter, tolerance_change=TOL_CHANGE, tolerance_grad=TOL_GRAD,
                            history_size=max_iter, line_search_fn="strong_wolfe")

    def closure():
        st["calls"] += 1
        x = float(logA.detach())
        l0 = fixed if fixed is not None else st["lambda0"]
        L, g, sf, closed = ev(x, l0)
        logA.grad = torch.tensor(-g, dtype=torch.float64)
        st["lambda0"] = closed
        if not math.isfinite(sf):
            raise ValueError(st["calls"])
        return torch.tensor(-L, dtype=torch.float64)

    mod = torch_lbfgs
    sw, ci = mod._strong_wolfe, mod._cubic_interpolate

    def strong_wolfe(*a, **k):
        res = sw(*a, **k)
        st["ls_losses"].append(float(res[0]))
        return res

    def cubic(*a, bounds=None):
        if bounds is None:
            st["zoom"] = True
        return ci(*a, bounds=bounds)

    mod._strong_wolfe, mod._cubic_interpolate = strong_wolfe, cubic
    status = 0
    try:
        first = float(opt.step(closure))
    except ValueError as e:
        status, first = int(e.args[0]), None
    finally:
        mod._strong_wolfe, mod._cubic_interpolate = sw, ci
    s = opt.state[logA]
    x = float(logA.detach())
    res = {"evals": st["calls"], "iters": s.get("n_iter", 0), "status": status, "zoom": st["zoom"],
           "pairs": len(s.get("old_dirs") or []), "first_loss": first,
           "last_loss": st["ls_losses"][-1] if st["ls_losses"] else first}
    if status:
        res.update(fail_logA=x, fail_lambda0=st["lambda0"])
    else:
        res.update(logA=x, lambda0=ev(x, 0.0)[3])
    return res


def close(a, b, tol=TOL):
    return abs(a - b) <= tol * max(1.0, abs(b))


def same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def check_case(lib, lam_m, lam_var, r, logA0, max_iter, fixed=None, kind="sequential"):
    """kind="sequential": torch's LBFGS over a closure that sums like the host instance, so every evaluation gives
    the same bits on both sides and everything must be equal.  kind="oracle": the oracle's closure (torch sums);
    counts must be equal, values within ORACLE_* (see the module docstring)."""
    h = run_host(lib, lam_m, lam_var, r, logA0, max_iter, fixed)
    t = run_torch(lam_m, lam_var, r, logA0, max_iter, fixed, kind)
    what = f"N={len(lam_m)} logA0={logA0} max_iter={max_iter} fixed={fixed} {kind}"
    assert (h["evals"], h["iters"], h["status"]) == (t["evals"], t["iters"], t["status"]), (what, h, t)
    if t["status"]:
        if kind == "sequential":
            assert same(h["fail_logA"], t["fail_logA"]) and same(h["fail_lambda0"], t["fail_lambda0"]), (what, h, t)
        else:
            assert close(h["fail_logA"], t["fail_logA"], ORACLE_X), what
            assert same(h["fail_lambda0"], t["fail_lambda0"]) or close(h["fail_lambda0"], t["fail_lambda0"], ORACLE_X), what
        return h, t
    if kind == "sequential":
        for k in ("logA", "lambda0", "first_loss", "last_loss"):
            assert same(h[k], t[k]), (what, k, h[k], t[k])
    else:
        assert close(h["logA"], t["logA"], ORACLE_X), (what, h["logA"], t["logA"])
        assert close(h["lambda0"], t["lambda0"], ORACLE_X), (what, h["lambda0"], t["lambda0"])
        assert abs(h["first_loss"] - t["first_loss"]) <= TOL * abs(t["first_loss"]), what
        assert abs(h["last_loss"] - t["last_loss"]) <= ORACLE_LOSS * abs(t["last_loss"]), what
    # the rate the kernel leaves behind: f at the final (logA, closed-form lambda0)
    A = math.exp(h["logA"])
    f_ref = np.exp(A * lam_m + 0.5 * A * A * lam_var + h["lambda0"])
    assert np.max(np.abs(h["f"] - f_ref) / np.abs(f_ref)) <= TOL, what
    return h, t


def profile_optimum(lam_m, lam_var, r):
    """logA where the closure's gradient at its own closed-form lambda0 vanishes (bisection in fp64)."""
    lm, lv, rr = (torch.from_numpy(a) for a in (lam_m, lam_var, r))

    def grad(x):
        l0 = orc.lambda0_closed_form(x, rr, lm, lv)
        A = math.exp(x)
        f = torch.exp(A * lm + 0.5 * A * A * lv + l0)
        return float(orc.expected_loglik(rr, f, lm, lv, x, l0, f_param_grad=True)[1]["logA"])

    lo, hi = -4.0, 1.5
    assert grad(lo) > 0 > grad(hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid in (lo, hi):
            break
        lo, hi = (mid, hi) if grad(mid) > 0 else (lo, mid)
    return lo if abs(grad(lo)) < abs(grad(hi)) else hi


def test_add_with_alpha_is_fused_in_installed_torch():
    """The port's x + t d and the two-loop updates are fused multiply-adds because ATen's CPU add(alpha) is."""
    a, b, c = 0.443, -0.542, 0.891
    p = torch.tensor(a, dtype=torch.float64)
    p.add_(torch.tensor(b, dtype=torch.float64), alpha=c)
    from fractions import Fraction as F
    exact = float(F(a) + F(c) * F(b))
    assert a + c * b != exact, "pick operands where the fused and the separate results differ"
    assert p.item() == exact


@pytest.mark.parametrize("n", [1, 5, 1000, 3160, 8192])
@pytest.mark.parametrize("max_iter", [1, 2, 4, 10, 25])
def test_matches_torch_lbfgs(lib, n, max_iter):
    lam_m, lam_var, r = make_inputs(n, seed=n)
    for logA0 in (-3.0, 1.2):            # far below and far above the optimum
        for fixed in (None, math.exp(-1.0)):
            for kind in ("sequential", "oracle"):
                check_case(lib, lam_m, lam_var, r, logA0, max_iter, fixed, kind)


@pytest.mark.parametrize("n", [1000, 3160])
def test_start_at_optimum_exits_after_one_evaluation(lib, n):
    lam_m, lam_var, r = make_inputs(n, seed=7)
    x = profile_optimum(lam_m, lam_var, r)
    for kind in ("sequential", "oracle"):
        h, t = check_case(lib, lam_m, lam_var, r, x, 10, kind=kind)
        assert h["evals"] == 1 and h["iters"] == 0


def test_line_search_paths_are_covered(lib):
    """The zoom phase, and a step() that exhausts max_eval (its line search evaluates past max_eval - current_evals's
    first trial).  The ys <= 1e-10 rule is ported but no input found reaches it: after a line search that ends on the
    Wolfe conditions ys >= 0.1 |g.d| t, a tenth of the loss decrease, so a skipped pair needs a loss change within a
    decade of tolerance_change (searched: N in 1..1000, rates scaled by 1e-6..1, starts -4..2.5, both lambda0 modes)."""
    lam_m, lam_var, r = make_inputs(5, seed=16)
    for kind in ("sequential", "oracle"):
        h, t = check_case(lib, lam_m, lam_var, r, -3.0, 4, math.exp(-1.0), kind)
        assert t["zoom"]
        h, t = check_case(lib, lam_m, lam_var, r, -3.0, 2, None, kind)
        assert t["evals"] >= 2 * 5 // 4 and t["iters"] < 2


def test_nan_in_r_fails_first_call(lib):
    lam_m, lam_var, r = make_inputs(1000, seed=11)
    r[3] = float("nan")
    for kind in ("sequential", "oracle"):
        h, t = check_case(lib, lam_m, lam_var, r, 0.0, 4, kind=kind)
        assert h["status"] == t["status"] == 1
    assert math.isnan(h["fail_lambda0"])


def test_exp_overflow_in_line_search(lib):
    """A start far below the optimum: the line search's extrapolation reaches a logA where exp overflows."""
    lam_m, lam_var, r = make_inputs(5, seed=16, logA_true=1.0)
    for kind in ("sequential", "oracle"):
        h, t = check_case(lib, lam_m, lam_var, r, -3.0, 4, math.exp(-1.0), kind)
        assert h["status"] == t["status"] == 5
        assert h["fail_logA"] == t["fail_logA"] and h["fail_lambda0"] == t["fail_lambda0"] == -math.inf
