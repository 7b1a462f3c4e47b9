"""gpfit_estep_chain_full (the full-rank E-steps between two kernel rebuilds as one device call) on the GPU: against
itself step by step, against the calls a step stands for (gpfit_estep, the loop's moments expression,
gpfit_fparam_lbfgs), its failure gating, and varGP / varGP_cells with the chain on and off."""
import contextlib
import copy
import ctypes
import functools
import io
import math
import threading
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden, relerr
from gaussian_processes_amd import _lib, synthetic as syn

pytestmark = pytest.mark.gpu
KEYS = syn.THETA_KEYS
LOWER, UPPER = syn.limits()
SIZES = [100, 300, 640]   # one leaf, ragged; np = 384: the uneven 256 + 128 block-wise split, ragged; n1 = 384, n2 = 256
NFP = 10                  # nFparamstep of the lab's fits
TOL_REF = 1e-6            # logA / lambda0 between the device's and the host's exp (tests/test_gpu_estep_chain.py)
TOL_UPDATE = 1e-10        # m, V and the moments (the same)
FIXED = math.exp(-1.0)
JOIN_S = 120


@pytest.fixture(scope="module")
def gp():
    from gaussian_processes_amd import utils
    return utils


def T(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).cuda()


@functools.lru_cache(maxsize=None)
def case(n):
    """Synthetic inputs built like case() of tests/test_gpu_estep_chain.py; computed once per size, never written."""
    rng = np.random.default_rng(11)
    Mx = rng.standard_normal((n, n + 40))
    K = T(Mx @ Mx.T / (n + 40) + 0.05 * np.eye(n))
    f = T(np.exp(0.3 * rng.standard_normal(n)))
    r = T(rng.poisson(1.0, n).astype(np.float64))
    m = T(0.2 * rng.standard_normal(n))
    kv0 = T(1e-3 * rng.random(n))          # non-zero: the term is visible in lam_var
    return {"K": K, "kv0": kv0, "m": m, "f": f, "r": r}


def chain(gp, c, m, f, logA0, n_steps, fixed=None, nfp=NFP, **state):
    return gp._estep_chain_full(c["r"], c["K"], c["kv0"], m, f, logA0, n_steps, nfp, lambda0_fixed=fixed, **state)


def estep_raw(gp, c, m, f, logA):
    """gpfit_estep as varGP's host loop calls it."""
    n = c["K"].shape[0]
    m_new = torch.empty(n, dtype=torch.float64, device=m.device)
    V_new = torch.empty((n, n), dtype=torch.float64, device=m.device)
    eng = gp.get_engine(n, 1)
    rc = _lib.load().gpfit_estep(eng._ctx, gp._stream(), c["K"].data_ptr(), c["K"].stride(0), n, c["r"].data_ptr(),
                                 m.data_ptr(), f.data_ptr(), logA, m_new.data_ptr(), V_new.data_ptr(), V_new.stride(0))
    assert rc == 0, (rc, _lib.last_error())
    return m_new, V_new


def fparam_lbfgs_raw(gp, lm, lv, r, logA0, max_iter, fixed=None):
    n = lm.shape[0]
    eng = gp.get_engine(n, 1)
    f = torch.empty(n, dtype=torch.float64, device=lm.device)
    out = (ctypes.c_double * 9)()
    _lib.check(_lib.load().gpfit_fparam_lbfgs(eng._ctx, gp._stream(), lm.data_ptr(), lv.data_ptr(), r.data_ptr(), n, logA0,
                                              0 if fixed is None else 1, 0.0 if fixed is None else fixed, max_iter,
                                              max_iter, 0.1, 1e-7, 1e-9, f.data_ptr(), out), "gpfit_fparam_lbfgs")
    return f, list(out)


def same(x, y):
    """Lists of floats equal entry by entry, NaN equal to NaN."""
    return len(x) == len(y) and all(p == q or (math.isnan(p) and math.isnan(q)) for p, q in zip(x, y))


@pytest.mark.parametrize("fixed", [None, FIXED])
@pytest.mark.parametrize("n", SIZES)
def test_chaining_is_exact(gp, n, fixed):
    """chain(3) against three chain(1), each fed the m, f and logA (slot 0 of its record) of the one before."""
    c = case(n)
    logA0 = math.log(0.5)
    m3, V3, lm3, lv3, f3, rec3 = chain(gp, c, c["m"], c["f"], logA0, 3, fixed)
    m, f, logA = c["m"], c["f"], logA0
    for k in range(3):
        m, V, lm, lv, f, rec = chain(gp, c, m, f, logA, 1, fixed)
        assert rec[0][9] == 0 and rec[0][10] == 1 and rec[0][6] == 0, (k, rec)
        assert same(rec[0], rec3[k]), (k, rec[0], rec3[k])
        logA = rec[0][0]
    assert logA != logA0                                  # the optimiser moved: the steps really differ
    for x, y in ((m, m3), (V, V3), (lm, lm3), (lv, lv3), (f, f3)):
        assert torch.equal(x, y)


def test_one_step_against_the_calls_it_stands_for(gp):
    """chain(1) against gpfit_estep, the loop's moments expression (lambda_m = m, lambda_var = (Kvec - diag K~) + diag V)
    and gpfit_fparam_lbfgs.  The chain forms A = exp(logA) on the device, gpfit_estep takes the host's: where the two
    agree (record slot 11) every output has the bits of the three; where they differ in the last bits, the update agrees
    to rounding and the optimiser to the bound of tests/test_gpu_estep_chain.py with equal closure counts.  logA0 = 0
    (exp is exactly 1 on both sides) must take the exact branch, and every size must take it at least once."""
    total = 0
    for n in SIZES:
        c = case(n)
        exact = 0
        for fixed in (None, FIXED):
            for logA0 in (0.0, math.log(0.5), 0.3, -1.2, 0.77, -0.4321):
                what = (n, fixed, logA0)
                m1, V1, lm1, lv1, f1, rec = chain(gp, c, c["m"], c["f"], logA0, 1, fixed)
                m2, V2 = estep_raw(gp, c, c["m"], c["f"], logA0)
                lm2, lv2 = m2.clone(), c["kv0"] + torch.diagonal(V2)
                f2, out = fparam_lbfgs_raw(gp, lm2, lv2, c["r"], logA0, NFP, fixed)
                rec = rec[0]
                assert rec[9] == 0 and rec[10] == 1 and rec[6] == 0 and out[6] == 0, (what, rec, out)
                total += 1
                if rec[11] == math.exp(logA0):
                    exact += 1
                    for x, y in ((m1, m2), (V1, V2), (lm1, lm2), (lv1, lv2), (f1, f2)):
                        assert torch.equal(x, y), what
                    assert same(rec[:9], out), (what, rec, out)
                else:
                    assert logA0 != 0.0, what
                    assert abs(rec[11] - math.exp(logA0)) <= 2 * math.ulp(math.exp(logA0)), (what, rec[11])
                    for x, y in ((m1, m2), (V1, V2), (lm1, lm2), (lv1, lv2)):
                        assert relerr(x.cpu().numpy(), y.cpu().numpy()) <= TOL_UPDATE, what
                    for i in (0, 1):
                        assert abs(rec[i] - out[i]) / max(1.0, abs(out[i])) <= TOL_REF, (what, i, rec[i], out[i])
                    assert rec[4] == out[4], (what, rec, out)
        print(f"N = {n}: chain(1) against the three calls, {exact} of 12 cases exact (the device's exp(logA0) equal to the host's)")
        assert exact >= 1, n
    assert total == 36


def test_non_finite_rate_stops_the_chain(gp):
    """One entry of the starting f is inf: M = I + S K S is not positive definite at step 0, nothing is committed by that
    step or by the two behind it, and every array comes back with the bits it went in with."""
    c = case(300)
    rng = np.random.default_rng(3)
    f0 = c["f"].clone()
    f0[7] = float("inf")
    V0, lm0, lv0 = T(rng.standard_normal((300, 300))), T(rng.standard_normal(300)), T(rng.random(300))
    m, V, lm, lv, f, rec = chain(gp, c, c["m"], f0, math.log(0.5), 3, V=V0, lambda_m=lm0, lambda_var=lv0)
    assert rec[0][9] != 0 and rec[0][10] == 0, rec[0]
    assert rec[0][11] == pytest.approx(0.5, rel=1e-15) and rec[0][:9] == [0.0] * 9, rec[0]
    assert rec[1] == [0.0] * 12 and rec[2] == [0.0] * 12, rec
    for x, y in ((m, c["m"]), (V, V0), (lm, lm0), (lv, lv0), (f, f0)):
        assert torch.equal(x, y)
    # the rate that step read is not finite: the loop's ValueError (the reference reports the NaNs one step later)
    fp = {"logA": torch.tensor(0.25, dtype=torch.float64)}
    with pytest.raises(ValueError, match=r"closure has been called 1 times in estep 0 iteration\. Try substituting them with inf\."):
        gp._estep_chain_full_commit(rec, fp, f)
    assert float(fp["logA"]) == 0.25 and "lambda0" not in fp    # what the host loop leaves when its first update fails
    # a finite rate behind the same records: the loop's LinAlgError with the text of gpfit_estep
    with pytest.raises(torch.linalg.LinAlgError,
                       match=rf"Estep: gpfit_estep: I \+ S K S is not positive definite .*\(rc={int(rec[0][9])}\)"):
        gp._estep_chain_full_commit(rec, fp, c["f"])


OVERFLOW_R, OVERFLOW_M, OVERFLOW_NFP = 5000.0, -4.0, 1


def test_optimiser_overflow_stops_the_chain(gp):
    """Finite inputs that are merely out of range, as in test_optimiser_overflow_stops_the_chain of
    tests/test_gpu_estep_chain.py, arranged so that a later step fails whatever the line search does: in case(100)
    one response is 5000, with the starting rate equal to it and the starting mean -4 there, from logA = 0.  Step 0 sees
    r - f = 0 at that point and leaves its mean near -4; its optimiser (one iteration: one clipped step of 0.1 down the
    gradient) leaves the rate normalised to sum r, about 1 at that point.  Step 1's update then moves the mean there by
    about (r - f) / (1 / K_ii + f) = 1500, A lam_m is about 1360 at the optimiser's first closure call (exp overflows
    at 709.8; no other point is above 60) and the sum of the rate is not finite: status 1 at step k = 1.  Step k's m, V
    and moments are committed -- those of a chain(1) started from the state chain(k) leaves --, its record carries the
    status and the (logA, lambda0) of gpfit_fparam_lbfgs on the same moments, f, logA and lambda0 stay, and the steps
    behind it are skipped."""
    c = dict(case(100))
    for key, v in (("r", OVERFLOW_R), ("f", OVERFLOW_R), ("m", OVERFLOW_M)):
        c[key] = c[key].clone()
        c[key][5] = v
    n_steps, nfp = 4, OVERFLOW_NFP
    m, V, lm, lv, f, rec = chain(gp, c, c["m"], c["f"], 0.0, n_steps, nfp=nfp)
    print("records of the overflowing chain (info, ran, status):", [(x[9], x[10], x[6]) for x in rec])
    k = next((i for i, x in enumerate(rec) if x[6] != 0), None)
    assert k is not None and 1 <= k < n_steps - 1, rec          # a later step fails, and at least one is behind it
    assert all(x[9] == 0 and x[10] == 1 and x[6] == 0 for x in rec[:k]), rec
    assert rec[k][9] == 0 and rec[k][10] == 1 and int(rec[k][6]) >= 1, rec[k]
    assert all(x == [0.0] * 12 for x in rec[k + 1:]), rec
    # the state in front of step k, and that step alone from it
    mk, _, _, _, fk, reck = chain(gp, c, c["m"], c["f"], 0.0, k, nfp=nfp)
    assert all(same(p, q) for p, q in zip(reck, rec[:k]))
    logAk = reck[-1][0]
    assert logAk != 0.0                                          # the optimiser of the steps in front moved logA
    m1, V1, lm1, lv1, f1, rec1 = chain(gp, c, mk, fk, logAk, 1, nfp=nfp)
    assert same(rec1[0], rec[k]), (rec1[0], rec[k])
    for x, y in ((m, m1), (V, V1), (lm, lm1), (lv, lv1)):
        assert torch.equal(x, y)
    assert not torch.equal(m, mk)                                # step k's update is in
    assert torch.equal(f, fk) and torch.equal(f1, fk)            # and its rate is not
    _, out = fparam_lbfgs_raw(gp, lm, lv, c["r"], logAk, nfp)
    assert same(rec[k][:9], out), (rec[k], out)
    assert rec[k][7] == logAk                                    # the failing call's point: logA as step k - 1 left it
    fp = {"logA": torch.tensor(0.0, dtype=torch.float64)}
    with pytest.raises(ValueError, match=rf"closure has been called {int(out[6])} times in estep {k} iteration\.$"):
        gp._estep_chain_full_commit(rec, fp, f)
    assert float(fp["logA"]) == out[7] and same([float(fp["lambda0"])], [out[8]])


def test_two_calls_are_bit_equal(gp):
    c = case(640)
    one = chain(gp, c, c["m"], c["f"], math.log(0.5), 3)
    two = chain(gp, c, c["m"], c["f"], math.log(0.5), 3)
    for x, y in zip(one[:5], two[:5]):
        assert torch.equal(x, y)
    assert all(same(p, q) for p, q in zip(one[5], two[5]))


# ---------------------------------------------------------------------------------------------- varGP
def vargp_args(g, X, ntilde, f_params=None, **fit_kwargs):
    fit_parameters = {"ntilde": ntilde, "maxiter": int(g["maxiter"]), "nEstep": int(g["nEstep"]), "nMstep": int(g["nMstep"]),
                      "nFparamstep": int(g["nFparamstep"]), "kernfun": "acosker", "cellid": 0, "n_px_side": 8,
                      "display_hyper": False}
    fit_parameters.update(fit_kwargs)
    theta = {k: torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for k, v in zip(KEYS, g["theta0"])}
    f_params = f_params or {"logA": syn.F_PARAMS["logA"], "lambda0": syn.F_PARAMS["lambda0"]}
    return {"fit_parameters": fit_parameters, "xtilde": X[:ntilde].clone(), "hyperparams_tuple": (theta, LOWER, UPPER),
            "f_params": {k: torch.tensor(float(v), dtype=torch.float64) for k, v in f_params.items()}}


def run_vargp(gp, g, X, r, ntilde, **fit_kwargs):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return gp.varGP(X, r, **vargp_args(g, X, ntilde, **fit_kwargs))


def count_calls(gp, monkeypatch, name):
    calls = []
    inner = getattr(gp, name)

    def spy(*args, **kwargs):
        calls.append(1)
        return inner(*args, **kwargs)
    monkeypatch.setattr(gp, name, spy)
    return calls


def test_whole_fit_with_the_chain_on_and_off(gp, monkeypatch):
    """varGP on the full-rank fixture with ESTEP_CHAIN on against off and against the reference's fixture, within the
    bounds test_vargp_end_to_end_matches_reference asserts for it (track 1e-6, KL 1e-5, theta, logA and the prediction
    1e-4; on against off also 1e-4 for m_b and V_b).  Every EM iteration goes through _estep_chain_full when the switch
    is on, none when it is off, and none through the projected chain either way."""
    name = "g6_vargp_full_N128.npz"
    g = load_golden(name)
    X, r, N = T(g["X"]), T(g["r"]), int(g["N"])
    full_calls = count_calls(gp, monkeypatch, "_estep_chain_full")
    proj_calls = count_calls(gp, monkeypatch, "_estep_chain")
    monkeypatch.setattr(gp, "EIGVAL_TOL", float(g["tol"]))
    runs = {}
    for on in (True, False):
        monkeypatch.setattr(gp, "ESTEP_CHAIN", on)
        before = len(full_calls)
        fit, err = run_vargp(gp, g, X, r, N)
        assert not err["is_error"], err
        assert (len(full_calls) - before) == (int(g["maxiter"]) - 1 if on else 0)
        Rt = T(np.random.default_rng(5).poisson(0.7, (4, 6, 1)).astype(np.float64))
        with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, R_pred, _, _ = gp.test(T(g["Xstar"]), Rt, X_train=X, at_iteration=None, **fit)
        runs[on] = (fit, R_pred)
    assert len(proj_calls) == 0

    def summary(fit):
        vt = fit["values_track"]
        return {"logmarginal": vt["loss_track"]["logmarginal"].numpy(), "KL": vt["loss_track"]["KL"].numpy(),
                "theta": np.array([float(fit["hyperparams_tuple"][0][k]) for k in KEYS]),
                "logA": float(fit["f_params"]["logA"])}
    on, off = summary(runs[True][0]), summary(runs[False][0])
    assert runs[True][0]["B"].shape[1] == int(g["n_kept"]) == N
    d = {"track": relerr(on["logmarginal"], off["logmarginal"]), "KL": relerr(on["KL"], off["KL"]),
         "theta": float(np.abs(on["theta"] - off["theta"]).max()), "logA": abs(on["logA"] - off["logA"]),
         "prediction": relerr(runs[True][1].cpu().numpy(), runs[False][1].cpu().numpy()),
         "m_b": relerr(runs[True][0]["m_b"].cpu().numpy(), runs[False][0]["m_b"].cpu().numpy()),
         "V_b": relerr(runs[True][0]["V_b"].cpu().numpy(), runs[False][0]["V_b"].cpu().numpy())}
    ref = {"track": relerr(on["logmarginal"], g["logmarginal"]), "KL": relerr(on["KL"], g["KL"]),
           "theta": float(np.abs(on["theta"] - g["theta_final"]).max()), "logA": abs(on["logA"] - float(g["logA_final"])),
           "prediction": relerr(runs[True][1].cpu().numpy(), g["R_pred"])}
    print(f"{name}: chain on against off {d}; chain on against the fixture {ref}")
    for x in (d, ref):
        assert x["track"] < 1e-6 and x["KL"] < 1e-5 and x["theta"] < 1e-4 and x["logA"] < 1e-4, x
        assert x["prediction"] < 1e-4, x
    assert d["m_b"] < 1e-4 and d["V_b"] < 1e-4, d


def test_vargp_error_is_the_loops_error(gp, monkeypatch):
    """A NaN response in the full-rank regime (the inputs of g10_vargp_rollback_N128, every eigenvalue kept, the
    inducing set the training set): the same exception type and message and the same f_params with the chain on and
    off."""
    g = load_golden("g10_vargp_rollback_N128.npz")
    X, r, N = T(g["X"]), T(g["r"]), int(g["N"])
    r[3] = float("nan")
    monkeypatch.setattr(gp, "EIGVAL_TOL", 1e-14)
    calls = count_calls(gp, monkeypatch, "_estep_chain_full")
    out = {}
    for on in (True, False):
        monkeypatch.setattr(gp, "ESTEP_CHAIN", on)
        out[on] = run_vargp(gp, g, X, r, N, maxiter=4, nEstep=2, nMstep=1, nFparamstep=1)
    assert len(calls) == 1
    (fit, err), (fit_off, err_off) = out[True], out[False]
    assert err["is_error"] and err_off["is_error"]
    assert type(err["error"]) is type(err_off["error"]) and str(err["error"]) == str(err_off["error"])
    for k in ("logA", "lambda0"):
        x, y = float(fit["f_params"][k]), float(fit_off["f_params"][k])
        assert x == y or (math.isnan(x) and math.isnan(y)), (k, x, y)


def in_a_thread(fn):
    """fn() in a fresh host thread, joined with a bound: its result, or its exception re-raised here."""
    box = {}

    def body():
        try:
            with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                box["out"] = fn()
        except BaseException as err:
            box["err"] = err
    t = threading.Thread(target=body, daemon=True)
    t.start()
    t.join(JOIN_S)
    assert not t.is_alive(), "the fit thread is still running"
    if "err" in box:
        raise box["err"]
    return box["out"]


def test_vargp_cells_is_vargp_cell_by_cell(gp, monkeypatch):
    """Two cells on the full-rank fixture's stimuli (cell 0 is the fixture's): each fit issues its full-rank chains
    directly on its own workspace and has the bits of varGP on that cell alone; nothing went through the rendezvous."""
    g = load_golden("g6_vargp_full_N128.npz")
    X, N = T(g["X"]), int(g["N"])
    rng = np.random.default_rng(17)
    rs = [T(g["r"]), T(rng.poisson(np.maximum(g["r"].mean(), 0.2), g["r"].shape).astype(np.float64))]
    monkeypatch.setattr(gp, "EIGVAL_TOL", float(g["tol"]))
    calls = count_calls(gp, monkeypatch, "_estep_chain_full")
    kwargs = [vargp_args(g, X, N) for _ in rs]
    cells = in_a_thread(lambda: gp.varGP_cells(X, rs, copy.deepcopy(kwargs)))
    assert len(cells) == 2 and len(calls) == 2 * (int(g["maxiter"]) - 1)
    assert list(gp.varGP_cells.last_group_sizes) == []
    for i, r in enumerate(rs):
        fit1, err1 = in_a_thread(lambda: gp.varGP(X, r, **copy.deepcopy(kwargs[i])))
        fit, err = cells[i]
        assert not err1["is_error"] and not err["is_error"], (err, err1)
        for group in ("loss_track", "theta_track", "f_par_track"):
            for k, v in fit["values_track"][group].items():
                assert torch.equal(v, fit1["values_track"][group][k]), (i, group, k)
        for k in ("m_b", "V_b"):
            assert torch.equal(fit[k], fit1[k]), (i, k)
