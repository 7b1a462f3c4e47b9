"""gpfit_estep_chain (the E-steps between two kernel rebuilds as one device call) on the GPU: against itself step by
step, against the two calls a step stands for (gpfit_estep_projected + gpfit_fparam_lbfgs), its failure gating, and
varGP with the chain on and off."""
import contextlib
import ctypes
import functools
import io
import math
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden, relerr
from gaussian_processes_amd import _lib, synthetic as syn

pytestmark = pytest.mark.gpu
KEYS = syn.THETA_KEYS
LOWER, UPPER = syn.limits()
SHAPES = [(300, 128), (640, 385), (1000, 128)]   # one leaf + ragged rows; four leaves + ragged columns; many row slices
NFP = 10                # nFparamstep of the lab's fits
TOL_REF = 1e-6          # logA / lambda0 between the device's and the host's exp (tests/test_gpu_fparam_lbfgs.py)
TOL_UPDATE = 1e-10      # m, V and the moments (test_projected_estep_on_a_tight_context)


@pytest.fixture(scope="module")
def gp():
    from gaussian_processes_amd import utils
    return utils


def T(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).cuda()


@functools.lru_cache(maxsize=None)
def case(nt, nb):
    """Synthetic inputs built like test_projected_estep_on_a_tight_context; computed once per shape, never written."""
    from gaussian_processes_amd import utils as gp
    rng = np.random.default_rng(11)
    Mx = rng.standard_normal((nb, nb + 40))
    Ktb = T(Mx @ Mx.T / (nb + 40) + 0.05 * np.eye(nb))
    a = T(rng.standard_normal((nt, nb)) / np.sqrt(nb))
    m_b = T(0.2 * rng.standard_normal(nb))
    f = T(np.exp(0.3 * rng.standard_normal(nt)))
    r = T(rng.poisson(1.0, nt).astype(np.float64))
    Kvec = T(2.0 + rng.random(nt))
    Kb = gp.matmul(a, Ktb)
    Lb, _, _, info = gp.cholesky(Ktb)
    assert info == 0
    return {"a": a, "aL": gp.matmul(a, Lb), "L": Lb, "kv0": Kvec - torch.sum(Kb * a, 1), "m": m_b, "f": f, "r": r}


def chain(gp, c, m, f, logA0, n_steps, fixed=None, nfp=NFP, **state):
    return gp._estep_chain(c["r"], c["a"], c["aL"], c["L"], c["kv0"], m, f, logA0, n_steps, nfp, lambda0_fixed=fixed,
                           **state)


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


@pytest.mark.parametrize("fixed", [None, math.exp(-1.0)])
@pytest.mark.parametrize("nt,nb", SHAPES)
def test_chaining_is_exact(gp, nt, nb, fixed):
    """chain(3) against three chain(1), each fed the m, f and logA (slot 0 of its record) of the one before."""
    c = case(nt, nb)
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


def test_one_step_against_the_existing_pair(gp):
    """chain(1) against _estep_projected(kv0=) followed by gpfit_fparam_lbfgs.  The chain forms A = exp(logA) on the
    device, the pair takes the host's: where the two agree (record slot 11) every output has the pair's bits; where
    they differ in the last bit, the update agrees to rounding and the optimiser to the bound of
    tests/test_gpu_fparam_lbfgs.py with equal closure counts.  logA0 = 0 (exp is exactly 1 on both sides) must take the
    exact branch."""
    exact = total = 0
    for nt, nb in SHAPES:
        c = case(nt, nb)
        for fixed in (None, math.exp(-1.0)):
            for logA0 in (0.0, math.log(0.5), 0.3, -1.2, 0.77, -0.4321):
                what = (nt, nb, fixed, logA0)
                m1, V1, lm1, lv1, f1, rec = chain(gp, c, c["m"], c["f"], logA0, 1, fixed)
                fp = {"logA": torch.tensor(logA0, dtype=torch.float64)}
                m2, V2, lm2, lv2 = gp._estep_projected(c["r"], c["a"], c["aL"], c["L"], c["m"], fp, c["f"], kv0=c["kv0"])
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
    print(f"chain(1) against the pair: {exact} of {total} cases exact (the device's exp(logA0) equal to the host's)")


def test_non_finite_rate_stops_the_chain(gp):
    """One entry of the starting f is inf: W is not positive definite at step 0, nothing is committed by that step or
    by the two behind it, and every array comes back with the bits it went in with."""
    c = case(300, 128)
    rng = np.random.default_rng(3)
    f0 = c["f"].clone()
    f0[7] = float("inf")
    V0, lm0, lv0 = T(rng.standard_normal((128, 128))), T(rng.standard_normal(300)), T(rng.random(300))
    m, V, lm, lv, f, rec = chain(gp, c, c["m"], f0, math.log(0.5), 3, V=V0, lambda_m=lm0, lambda_var=lv0)
    assert rec[0][9] != 0 and rec[0][10] == 0, rec[0]
    assert rec[0][11] == pytest.approx(0.5, rel=1e-15) and rec[0][:9] == [0.0] * 9, rec[0]
    assert rec[1] == [0.0] * 12 and rec[2] == [0.0] * 12, rec
    for x, y in ((m, c["m"]), (V, V0), (lm, lm0), (lv, lv0), (f, f0)):
        assert torch.equal(x, y)
    fp = {"logA": torch.tensor(0.25, dtype=torch.float64)}
    with pytest.raises(torch.linalg.LinAlgError, match=rf"Estep: I \+ L\^T G L is not positive definite \(info={int(rec[0][9])}\)"):
        gp._estep_chain_commit(rec, fp)
    assert float(fp["logA"]) == 0.25 and "lambda0" not in fp    # what the host loop leaves when its first update fails


def overflow_inputs(seed):
    """Five training points with the responses of test_device_entry_overflow_matches_reference's generator
    (tests/test_gpu_fparam_lbfgs.py: inputs(5, seed, logA_true=1.0)) behind a 5 x 5 projection; lambda0 fixed and the
    start at logA = -3 as there."""
    rng = np.random.default_rng(seed)
    lam_m = rng.standard_normal(5) * 0.8
    lam_var = rng.uniform(0.02, 0.3, 5)
    A = math.exp(1.0)
    r = rng.poisson(np.exp(A * lam_m + 0.5 * A * A * lam_var - 1.0)).astype(np.float64)
    if r.sum() == 0:
        r[0] = 1.0
    rng = np.random.default_rng(1000 + seed)
    Mx = rng.standard_normal((5, 45))
    Ktb = Mx @ Mx.T / 45 + 0.05 * np.eye(5)
    a = np.eye(5) + 0.1 * rng.standard_normal((5, 5))
    return Ktb, a, np.linalg.solve(a, lam_m), np.exp(lam_m + 0.5 * lam_var - 1.0), r, lam_var


def test_optimiser_overflow_stops_the_chain(gp):
    """A step whose line search reaches a logA where exp overflows (seed 20 of overflow_inputs: the host instance of
    the optimiser fails in its 5th closure call on the moments behind the first update): the update of that step is
    committed, the record carries the status and the (logA, lambda0) of gpfit_fparam_lbfgs on the same moments, f stays,
    and the two steps behind it are skipped."""
    Ktb, a, m0, f0, r, kv0 = (T(x) for x in overflow_inputs(20))
    Lb, _, _, info = gp.cholesky(Ktb)
    assert info == 0
    c = {"a": a, "aL": gp.matmul(a, Lb), "L": Lb, "kv0": kv0, "r": r}
    fixed = math.exp(-1.0)
    m, V, lm, lv, f, rec = chain(gp, c, m0, f0, -3.0, 3, fixed, nfp=4)
    _, out = fparam_lbfgs_raw(gp, lm, lv, r, -3.0, 4, fixed)
    assert rec[0][9] == 0 and rec[0][10] == 1, rec[0]
    assert int(rec[0][6]) == int(out[6]) > 1, (rec[0], out)
    assert same(rec[0][7:9], out[7:9]) and same(rec[0][:9], out), (rec[0], out)
    assert rec[1] == [0.0] * 12 and rec[2] == [0.0] * 12, rec
    assert torch.equal(f, f0)
    fp = {"logA": torch.tensor(-3.0, dtype=torch.float64)}
    m2, V2, lm2, lv2 = gp._estep_projected(r, a, c["aL"], Lb, m0, fp, f0, kv0=kv0)
    if rec[0][11] == math.exp(-3.0):
        for x, y in ((m, m2), (V, V2), (lm, lm2), (lv, lv2)):
            assert torch.equal(x, y)
    with pytest.raises(ValueError, match=rf"closure has been called {int(out[6])} times in estep 0 iteration\."):
        gp._estep_chain_commit(rec, fp)
    assert float(fp["logA"]) == out[7] and same([float(fp["lambda0"])], [out[8]])


def test_two_calls_are_bit_equal(gp):
    c = case(640, 385)
    one = chain(gp, c, c["m"], c["f"], math.log(0.5), 3)
    two = chain(gp, c, c["m"], c["f"], math.log(0.5), 3)
    for x, y in zip(one[:5], two[:5]):
        assert torch.equal(x, y)
    assert all(same(p, q) for p, q in zip(one[5], two[5]))


def run_vargp(gp, g, X, r, ntilde, f_params=None, **fit_kwargs):
    fit_parameters = {"ntilde": ntilde, "maxiter": int(g["maxiter"]), "nEstep": int(g["nEstep"]), "nMstep": int(g["nMstep"]),
                      "nFparamstep": int(g["nFparamstep"]), "kernfun": "acosker", "cellid": 0, "n_px_side": 8,
                      "display_hyper": False}
    fit_parameters.update(fit_kwargs)
    theta = {k: torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for k, v in zip(KEYS, g["theta0"])}
    args = {"fit_parameters": fit_parameters, "xtilde": X[:ntilde].clone(), "hyperparams_tuple": (theta, LOWER, UPPER),
            "f_params": {"logA": torch.tensor(syn.F_PARAMS["logA"], dtype=torch.float64),
                         "lambda0": torch.tensor(syn.F_PARAMS["lambda0"], dtype=torch.float64)}}
    if f_params is not None:
        args["f_params"] = {k: torch.tensor(float(v), dtype=torch.float64) for k, v in f_params.items()}
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return gp.varGP(X, r, **args)


def count_chain_calls(gp, monkeypatch):
    calls = []
    inner = gp._estep_chain

    def spy(*args, **kwargs):
        calls.append(1)
        return inner(*args, **kwargs)
    monkeypatch.setattr(gp, "_estep_chain", spy)
    return calls


@pytest.mark.parametrize("name", ["g6_vargp_sparse_N128_nt64.npz", "g6_vargp_trunc_N128.npz"])
def test_whole_fits_with_the_chain_on_and_off(gp, monkeypatch, name):
    """varGP with ESTEP_CHAIN on against off and against the reference's fixture, within the bounds
    test_vargp_end_to_end_matches_reference asserts for the same fixture (tracks 1e-5, KL 1e-4, theta, logA and the
    prediction 1e-4; the prediction's bound also for m_b and V_b, which that test only reaches through it)."""
    g = load_golden(name)
    X, r = T(g["X"]), T(g["r"])
    ntilde = int(g["ntilde"]) if "ntilde" in g else int(g["N"])
    calls = count_chain_calls(gp, monkeypatch)
    monkeypatch.setattr(gp, "EIGVAL_TOL", float(g["tol"]))
    runs = {}
    for on in (True, False):
        monkeypatch.setattr(gp, "ESTEP_CHAIN", on)
        before = len(calls)
        fit, err = run_vargp(gp, g, X, r, ntilde)
        assert not err["is_error"], err
        assert (len(calls) - before) == (int(g["maxiter"]) - 1 if on else 0)
        Rt = T(np.random.default_rng(5).poisson(0.7, (4, 6, 1)).astype(np.float64))
        with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, R_pred, _, _ = gp.test(T(g["Xstar"]), Rt, X_train=X, at_iteration=None, **fit)
        runs[on] = (fit, R_pred)

    def summary(fit):
        vt = fit["values_track"]
        return {"kept": [int(v.shape[0]) for v in vt["variation_par_track"]["V_b"]],
                "logmarginal": vt["loss_track"]["logmarginal"].numpy(), "KL": vt["loss_track"]["KL"].numpy(),
                "theta": np.array([float(fit["hyperparams_tuple"][0][k]) for k in KEYS]),
                "logA": float(fit["f_params"]["logA"])}
    on, off = summary(runs[True][0]), summary(runs[False][0])
    assert on["kept"] == off["kept"] and runs[True][0]["B"].shape[1] == int(g["n_kept"])
    d = {"track": relerr(on["logmarginal"], off["logmarginal"]), "KL": relerr(on["KL"], off["KL"]),
         "theta": float(np.abs(on["theta"] - off["theta"]).max()), "logA": abs(on["logA"] - off["logA"]),
         "m_b": relerr(runs[True][0]["m_b"].cpu().numpy(), runs[False][0]["m_b"].cpu().numpy()),
         "V_b": relerr(runs[True][0]["V_b"].cpu().numpy(), runs[False][0]["V_b"].cpu().numpy())}
    ref = {"track": relerr(on["logmarginal"], g["logmarginal"]), "KL": relerr(on["KL"], g["KL"]),
           "theta": float(np.abs(on["theta"] - g["theta_final"]).max()), "logA": abs(on["logA"] - float(g["logA_final"])),
           "prediction": relerr(runs[True][1].cpu().numpy(), g["R_pred"])}
    print(f"{name}: chain on against off {d}; chain on against the fixture {ref}")
    assert d["track"] < 1e-5 and d["KL"] < 1e-4 and d["theta"] < 1e-4 and d["logA"] < 1e-4, d
    assert d["m_b"] < 1e-4 and d["V_b"] < 1e-4, d
    assert ref["track"] < 1e-5 and ref["KL"] < 1e-4 and ref["theta"] < 1e-4 and ref["logA"] < 1e-4, ref
    assert ref["prediction"] < 1e-4, ref


def test_vargp_error_is_the_loops_error(gp, monkeypatch):
    """A NaN response in the sparse regime (the pattern of test_vargp_error_matches_reference_block with
    n_tilde < N): the same exception type and message and the same f_params with the chain on and off."""
    g = load_golden("g10_vargp_rollback_N128.npz")
    X, r = T(g["X"]), T(g["r"])
    r[3] = float("nan")
    monkeypatch.setattr(gp, "EIGVAL_TOL", 1e-14)
    calls = count_chain_calls(gp, monkeypatch)
    out = {}
    for on in (True, False):
        monkeypatch.setattr(gp, "ESTEP_CHAIN", on)
        out[on] = run_vargp(gp, g, X, r, 64, maxiter=4, nEstep=2, nMstep=1, nFparamstep=1)
    assert len(calls) >= 1
    (fit, err), (fit_off, err_off) = out[True], out[False]
    assert err["is_error"] and err_off["is_error"]
    assert type(err["error"]) is type(err_off["error"]) and str(err["error"]) == str(err_off["error"])
    for k in ("logA", "lambda0"):
        x, y = float(fit["f_params"][k]), float(fit_off["f_params"][k])
        assert x == y or (math.isnan(x) and math.isnan(y)), (k, x, y)


def test_fixed_lambda0_keeps_the_host_loop(gp, monkeypatch):
    """f_params carrying loglambda0 with nEstep > 1: the loop evaluates the rate at the fixed lambda0 before every
    update (rate_now), the chain would hand on the optimiser's rate at the closed-form one -- so varGP keeps the loop
    whatever ESTEP_CHAIN says.  The switch changes nothing: the bounds of the 'lambda0' whole-fit case hold (the two
    runs are the same code: the differences are 0), and a chain fed the same way would not have met them."""
    g = load_golden("g6_vargp_sparse_N128_nt64.npz")
    assert int(g["nEstep"]) > 1
    X, r = T(g["X"]), T(g["r"])
    calls = count_chain_calls(gp, monkeypatch)
    monkeypatch.setattr(gp, "EIGVAL_TOL", float(g["tol"]))
    fits = {}
    for on in (True, False):
        monkeypatch.setattr(gp, "ESTEP_CHAIN", on)
        fit, err = run_vargp(gp, g, X, r, int(g["ntilde"]), f_params={"logA": syn.F_PARAMS["logA"], "loglambda0": -1.0})
        assert not err["is_error"], err
        fits[on] = fit
    assert len(calls) == 0
    on, off = fits[True], fits[False]
    track = lambda fit, k: fit["values_track"]["loss_track"][k].numpy()
    theta = lambda fit: np.array([float(fit["hyperparams_tuple"][0][k]) for k in KEYS])
    assert float(on["f_params"]["loglambda0"]) == -1.0
    d = {"track": relerr(track(on, "logmarginal"), track(off, "logmarginal")), "KL": relerr(track(on, "KL"), track(off, "KL")),
         "theta": float(np.abs(theta(on) - theta(off)).max()),
         "logA": abs(float(on["f_params"]["logA"]) - float(off["f_params"]["logA"])),
         "m_b": relerr(on["m_b"].cpu().numpy(), off["m_b"].cpu().numpy()),
         "V_b": relerr(on["V_b"].cpu().numpy(), off["V_b"].cpu().numpy())}
    print(f"loglambda0 fit, switch on against off: {d}")
    assert d["track"] < 1e-5 and d["KL"] < 1e-4 and d["theta"] < 1e-4 and d["logA"] < 1e-4, d
    assert d["m_b"] < 1e-4 and d["V_b"] < 1e-4, d
    # the reviewer's point, measured: one chained iteration in mode 1 from the same state is NOT the loop's
    c = case(300, 128)
    fixed = math.exp(-1.0)
    m2, V2, _, _, f2, rec = chain(gp, c, c["m"], c["f"], math.log(0.5), 2, fixed)
    m1, _, lm1, lv1, _, rec1 = chain(gp, c, c["m"], c["f"], math.log(0.5), 1, fixed)
    f_loop = gp.mean_f_given_lambda_moments({"logA": torch.tensor(rec1[0][0]), "lambda0": torch.tensor(fixed)}, lm1, lv1)
    m_loop, _, _, _, _, _ = chain(gp, c, m1, f_loop, rec1[0][0], 1, fixed)
    print(f"second update, chain against the loop's rate: m differs by {relerr(m2.cpu().numpy(), m_loop.cpu().numpy()):.2e}")
    assert relerr(m2.cpu().numpy(), m_loop.cpu().numpy()) > 1e-4


def test_vargp_optimiser_failure_at_a_later_step(gp, monkeypatch):
    """Responses scaled by 20 with one of 1000 more, from logA = -1.5: the first update and its optimiser run, the
    optimiser of the second fails in its first closure call (sum f not finite).  Through varGP's chain branch this is
    the status branch of _estep_chain_commit at step k = 1 > 0: the loop's ValueError with its step number, and logA /
    lambda0 as the loop leaves them (step 0's logA committed, then the failing call's point)."""
    g = load_golden("g6_vargp_sparse_N128_nt64.npz")
    X, r = T(g["X"]), T(g["r"]) * 20.0
    r[5] += 1000.0
    monkeypatch.setattr(gp, "EIGVAL_TOL", float(g["tol"]))
    calls = count_chain_calls(gp, monkeypatch)
    out = {}
    for on in (True, False):
        monkeypatch.setattr(gp, "ESTEP_CHAIN", on)
        out[on] = run_vargp(gp, g, X, r, 64, f_params={"logA": -1.5, "lambda0": -1.0}, maxiter=3, nEstep=4, nMstep=1,
                            nFparamstep=4)
    assert len(calls) == 1
    (fit, err), (fit_off, err_off) = out[True], out[False]
    assert err["is_error"] and err_off["is_error"]
    assert type(err["error"]) is ValueError is type(err_off["error"]) and str(err["error"]) == str(err_off["error"])
    assert "closure has been called 1 times in estep 1 iteration." in str(err["error"])
    for k in ("logA", "lambda0"):
        x, y = float(fit["f_params"][k]), float(fit_off["f_params"][k])
        assert x == y or (math.isnan(x) and math.isnan(y)), (k, x, y)
    assert float(fit["f_params"]["logA"]) != -1.5          # step 0's optimiser moved logA before step 1 failed
    for k in ("m_b", "V_b"):                              # and step 1's update is in, as in the loop
        assert relerr(fit[k].cpu().numpy(), fit_off[k].cpu().numpy()) < 1e-10, k
