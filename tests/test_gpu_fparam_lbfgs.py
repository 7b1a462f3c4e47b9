"""gpfit_fparam_lbfgs (the rate-parameter optimiser of an E-step in one launch) on the GPU, against the E-step block
varGP ran before it: torch.optim.LBFGS over closures that each call utils._fparam_eval (one fparam_kernel launch and
one wait per call), copied here as the reference."""
import contextlib
import ctypes
import io
import math
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden
from gaussian_processes_amd import _lib, synthetic as syn

pytestmark = pytest.mark.gpu
TOL = 1e-13
KEYS = syn.THETA_KEYS
LOWER, UPPER = syn.limits()


@pytest.fixture(scope="module")
def gp():
    from gaussian_processes_amd import utils
    return utils


def inputs(n, seed, logA_true=0.3, lambda0_true=-1.0):
    rng = np.random.default_rng(seed)
    lam_m = rng.standard_normal(n) * 0.8
    lam_var = rng.uniform(0.02, 0.3, n)
    A = math.exp(logA_true)
    r = rng.poisson(np.exp(A * lam_m + 0.5 * A * A * lam_var + lambda0_true)).astype(np.float64)
    if r.sum() == 0:
        r[0] = 1.0
    return lam_m, lam_var, r


def f_params_at(logA0, loglambda0=None):
    fp = {"logA": torch.tensor(logA0, dtype=torch.float64, requires_grad=True)}
    if loglambda0 is None:
        fp["lambda0"] = torch.tensor(0.0, dtype=torch.float64)
    else:
        fp["loglambda0"] = torch.tensor(loglambda0, dtype=torch.float64)
    return fp


def reference_block(gp, lambda_m, lambda_var, r, f_params, n_steps, i_estep):
    """varGP's E-step block before gpfit_fparam_lbfgs (utils.py:1892-1934), as it was."""
    f_params['lambda0'] = gp.lambda0_given_logA(f_params['logA'], r, lambda_m, lambda_var)
    opt_f = torch.optim.LBFGS([f_params['logA']], lr=0.1, max_iter=n_steps, tolerance_change=1.e-9,
                              tolerance_grad=1.e-7, history_size=n_steps, line_search_fn='strong_wolfe')
    calls = [0]

    def closure_f_params():
        calls[0] += 1
        _, out = gp._fparam_eval(lambda_m, lambda_var, r, f_params['logA'], False,
                                 gp._scalar(gp._lambda0_of(f_params)), want_f=False)
        f_params['logA'].grad = torch.tensor(-out[2], dtype=torch.float64)
        f_params['lambda0'] = torch.tensor(out[6], dtype=torch.float64)
        if not math.isfinite(out[3]):
            raise ValueError(f'Nan in f_mean during f param update in Estep, closure has been called '
                             f'{calls[0]} times in estep {i_estep} iteration.')
        return torch.tensor(-out[1], dtype=torch.float64)
    err = None
    try:
        opt_f.step(closure_f_params)
    except ValueError as e:
        err = e
    n_iter = opt_f.state[f_params['logA']].get('n_iter', 0)
    if err is not None:
        return err, calls[0], n_iter
    f, out = gp._fparam_eval(lambda_m, lambda_var, r, f_params['logA'], True)      # lambda0_and_rate()
    f_params['lambda0'] = torch.tensor(out[0], dtype=torch.float64)
    return None, calls[0], n_iter


def device_entry(gp, lm, lv, r, logA0, max_iter, loglambda0=None):
    lib = _lib.load()
    n = lm.shape[0]
    eng = gp.get_engine(n, 1)
    f = torch.empty(n, dtype=torch.float64, device=lm.device)
    out = (ctypes.c_double * 9)()
    fixed = loglambda0 is not None
    l0 = float(torch.exp(torch.tensor(loglambda0, dtype=torch.float64))) if fixed else 0.0
    _lib.check(lib.gpfit_fparam_lbfgs(eng._ctx, gp._stream(), lm.data_ptr(), lv.data_ptr(), r.data_ptr(), n, logA0,
                                      1 if fixed else 0, l0, max_iter, max_iter, 0.1, 1e-7, 1e-9, f.data_ptr(), out),
               "gpfit_fparam_lbfgs")
    return f, list(out)


def rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


# The kernel computes A = exp(logA) on the device; the reference block passes std::exp(logA) of the host to
# fparam_kernel.  The two differ in the last bit for some logA, and the line search amplifies a last-bit difference
# of the objective (tests/test_fparam_lbfgs_cpu.py measures that amplification between two summation orders: up to
# 6.6e-8).  Measured on the MI355X: 57 of the 84 cases give the reference's bits exactly (difference 0); of the 78
# compared, counts are equal in all and the worst difference is 2.9e-9 in logA / lambda0 (N = 1023, 1024, 3160,
# 8192 from logA0 = 1.2, max_iter = 10).
# N = 1 with the closed-form lambda0 is degenerate: lambda0 makes f = r, so the losses the line search compares
# differ by rounding only and the comparisons are ties.  There a one-ulp change of A moves the count (max_iter = 4
# from logA0 = -3: 6 evaluations with the device's A, 5 with the host's; a one-ulp lower A gives 5 on the host
# instance too) and the end point (4.8e-2 at max_iter = 10).  Those cases are run but not compared.
TIES = {(1, m, x0, None) for m in (1, 4, 10) for x0 in (-3.0, 1.2)}
TOL_REF = 1e-6


@pytest.mark.parametrize("n", [1, 1000, 1023, 1024, 1025, 3160, 8192])
def test_device_entry_matches_reference_block(gp, n):
    lam_m, lam_var, r = inputs(n, seed=n)
    lm, lv, rr = (torch.from_numpy(a).cuda() for a in (lam_m, lam_var, r))
    worst = 0.0
    for max_iter in (1, 4, 10):
        for logA0 in (-3.0, 1.2):
            for loglambda0 in (None, -1.0):
                f, out = device_entry(gp, lm, lv, rr, logA0, max_iter, loglambda0)
                fp = f_params_at(logA0, loglambda0)
                err, calls, n_iter = reference_block(gp, lm, lv, rr, fp, max_iter, 0)
                what = (n, max_iter, logA0, loglambda0)
                assert err is None and out[6] == 0, what
                d = max(rel(out[0], float(fp['logA'])), rel(out[1], float(fp['lambda0'])))
                print(f"{what}: evals {int(out[4])} / {calls}, iterations {int(out[5])} / {n_iter}, logA / lambda0 {d:.2e}")
                if what in TIES:
                    continue
                assert (int(out[4]), int(out[5])) == (calls, n_iter), (what, out, calls, n_iter)
                worst = max(worst, d)
                assert d <= TOL_REF, what
                f_ref = gp.mean_f_given_lambda_moments({'logA': torch.tensor(out[0]), 'lambda0': torch.tensor(out[1])},
                                                       lm, lv)
                assert float(torch.max(torch.abs(f - f_ref) / torch.abs(f_ref))) <= TOL, what
    print(f"N={n}: worst logA / lambda0 difference {worst:.2e}")


@pytest.mark.parametrize("n", [1, 1000, 1025, 8192])
def test_device_entry_matches_host_instance(gp, n):
    """Device against the host instance of the same template.  The two sum in different orders; counts are equal
    and the values agree to the bound tests/test_fparam_lbfgs_cpu.py measures between two summation orders."""
    lib = _lib.load()
    lam_m, lam_var, r = inputs(n, seed=n + 1)
    lm, lv, rr = (torch.from_numpy(a).cuda() for a in (lam_m, lam_var, r))
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for max_iter in (1, 4, 10):
        for logA0 in (-3.0, 1.2):
            f, out = device_entry(gp, lm, lv, rr, logA0, max_iter)
            oh = (ctypes.c_double * 9)()
            fh = np.empty(n)
            assert lib.gpfit_fparam_lbfgs_host(ptr(lam_m), ptr(lam_var), ptr(r), n, logA0, 0, 0.0, max_iter, max_iter,
                                               0.1, 1e-7, 1e-9, ptr(fh), oh) == 0
            oh = list(oh)
            assert out[4:7] == oh[4:7], (n, max_iter, logA0, out, oh)
            assert abs(out[2] - oh[2]) <= TOL * abs(oh[2])
            for i in (0, 1, 3):
                assert rel(out[i], oh[i]) <= 1e-6, (n, max_iter, logA0, i, out[i], oh[i])


def test_device_entry_overflow_matches_reference(gp):
    """A start whose line search reaches a logA where exp overflows: the status is the reference's closure count, and
    logA / lambda0 are left where the reference's closure leaves them."""
    lam_m, lam_var, r = inputs(5, seed=16, logA_true=1.0)
    lm, lv, rr = (torch.from_numpy(a).cuda() for a in (lam_m, lam_var, r))
    f, out = device_entry(gp, lm, lv, rr, -3.0, 4, -1.0)
    fp = f_params_at(-3.0, -1.0)
    err, calls, _ = reference_block(gp, lm, lv, rr, fp, 4, 0)
    assert err is not None and f"closure has been called {calls} times" in str(err)
    assert int(out[6]) == calls > 1
    assert out[7] == float(fp['logA']) and out[8] == float(fp['lambda0'])


def test_vargp_error_matches_reference_block(gp, monkeypatch):
    """varGP with the NaN response of test_vargp_error_in_first_iteration_returns_err_dict: the error (closure count
    in its message) and the f_params left behind equal those of a run with the reference block in the optimiser's
    place."""
    g = load_golden("g10_vargp_rollback_N128.npz")
    N = int(g["N"])
    X = torch.from_numpy(np.asarray(g["X"], dtype=np.float64)).cuda()
    r = torch.from_numpy(np.asarray(g["r"], dtype=np.float64)).cuda()
    r[3] = float("nan")

    def run():
        fit_parameters = {"ntilde": N, "maxiter": 4, "nEstep": 1, "nMstep": 1, "nFparamstep": 1, "kernfun": "acosker",
                          "cellid": 0, "n_px_side": 8, "display_hyper": False}
        theta = {k: torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for k, v in zip(KEYS, g["theta0"])}
        args = {"fit_parameters": fit_parameters, "xtilde": X.clone(), "hyperparams_tuple": (theta, LOWER, UPPER),
                "f_params": {"logA": torch.tensor(syn.F_PARAMS["logA"], dtype=torch.float64),
                             "lambda0": torch.tensor(syn.F_PARAMS["lambda0"], dtype=torch.float64)}}
        old = gp.EIGVAL_TOL
        gp.EIGVAL_TOL = 1e-14
        try:
            with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return gp.varGP(X, r, **args)
        finally:
            gp.EIGVAL_TOL = old

    fit, err = run()

    def ref(lambda_m, lambda_var, rr, f_params, n_steps, i_estep):
        e, _, _ = reference_block(gp, lambda_m, lambda_var, rr, f_params, n_steps, i_estep)
        if e is not None:
            raise e
        f = gp.mean_f_given_lambda_moments(f_params, lambda_m, lambda_var)
        return f, float(f_params['lambda0'])
    monkeypatch.setattr(gp, "_fparam_lbfgs", ref)
    fit_ref, err_ref = run()
    assert err["is_error"] and err_ref["is_error"]
    assert type(err["error"]) is type(err_ref["error"]) and str(err["error"]) == str(err_ref["error"])
    for k in ("logA", "lambda0"):
        a, b = float(fit["f_params"][k]), float(fit_ref["f_params"][k])
        assert a == b or (math.isnan(a) and math.isnan(b)), (k, a, b)


def test_two_calls_are_bit_equal(gp):
    lam_m, lam_var, r = inputs(3160, seed=9)
    lm, lv, rr = (torch.from_numpy(a).cuda() for a in (lam_m, lam_var, r))
    f1, o1 = device_entry(gp, lm, lv, rr, -1.0, 10)
    f2, o2 = device_entry(gp, lm, lv, rr, -1.0, 10)
    assert o1 == o2 and torch.equal(f1, f2)
