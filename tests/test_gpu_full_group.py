"""gpfit_estep_chain_full_batch (the full-rank E-step chains of several independent units as one lock-step device call) on
the GPU: every unit inside a group against the same unit alone (gpfit_estep_chain_full, the group of one of the same
implementation), bit for bit; one step of a group against the un-chained calls it stands for; a failing unit stops alone;
the refusals; and varGP_cells in the full-rank regime -- chains and M-step closures as group calls -- against the same
fits run one after another, with FULL_RANK_GROUPS on and off, and in a wave mixed with a sparse and a failing fit."""
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
NFP = 10                  # nFparamstep of the lab's fits
# N and the units of its group: one leaf, ragged; np = 384: the uneven 256 + 128 block-wise split, ragged; n1 = 384, n2 = 256
GROUPS = [(100, 3), (300, 3), (640, 2)]
TOL_REF = 1e-6            # logA / lambda0 between the device's and the host's exp (tests/test_gpu_estep_chain_full.py)
TOL_UPDATE = 1e-10        # m, V and the moments (the same)
FIXED = math.exp(-1.0)
JOIN_S = 300              # a fit thread still alive after this is a deadlock: the test fails instead of hanging


@pytest.fixture(scope="module")
def gp():
    from gaussian_processes_amd import utils
    return utils


def T(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).cuda()


@functools.lru_cache(maxsize=None)
def case(n, seed):
    """Inputs built like case(n) of tests/test_gpu_estep_chain_full.py, from the given seed; computed once, never
    written."""
    rng = np.random.default_rng(seed)
    Mx = rng.standard_normal((n, n + 40))
    K = T(Mx @ Mx.T / (n + 40) + 0.05 * np.eye(n))
    f = T(np.exp(0.3 * rng.standard_normal(n)))
    r = T(rng.poisson(1.0, n).astype(np.float64))
    m = T(0.2 * rng.standard_normal(n))
    kv0 = T(1e-3 * rng.random(n))          # non-zero: the term is visible in lam_var
    return {"K": K, "kv0": kv0, "m": m, "f": f, "r": r}


def unit(c, logA0, fixed=None, **over):
    u = {"r": c["r"], "K_tilde": c["K"], "kv0": c["kv0"], "m": c["m"], "f_mean": c["f"], "logA0": logA0,
         "lambda0_fixed": fixed}
    u.update(over)
    return u


def single(gp, u, n_steps, nfp=NFP):
    """The unit alone: gpfit_estep_chain_full, the group of one."""
    return gp._estep_chain_full(n_steps=n_steps, n_fparam_steps=nfp, **u)


def same(x, y):
    """Lists of floats equal entry by entry, NaN equal to NaN."""
    return len(x) == len(y) and all(p == q or (math.isnan(p) and math.isnan(q)) for p, q in zip(x, y))


def bits(x, y):
    """Tensors equal bit for bit (a NaN equal to the same NaN)."""
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64))


def assert_bit_equal(got, want, what):
    for name, x, y in zip(("m", "V", "lam_m", "lam_var", "f"), got[:5], want[:5]):
        assert bits(x, y), (what, name)
    assert len(got[5]) == len(want[5])
    for k, (p, q) in enumerate(zip(got[5], want[5])):
        assert same(p, q), (what, k, p, q)


def ran(records):
    return all(rec[9] == 0 and rec[10] == 1 and rec[6] == 0 for rec in records)


@pytest.mark.parametrize("fixed", [None, FIXED])
@pytest.mark.parametrize("n_steps", [1, 3])
@pytest.mark.parametrize("n,nu", GROUPS)
def test_every_unit_has_the_bits_of_its_single_chain(gp, n, nu, n_steps, fixed):
    """A unit inside a group against the same unit alone."""
    units = [unit(case(n, 100 + i), math.log(0.5) + 0.1 * i, fixed) for i in range(nu)]
    group = gp._estep_chain_full_group(units, n_steps, NFP)
    assert len(group) == nu
    moved = False
    for i, u in enumerate(units):
        want = single(gp, u, n_steps)
        assert ran(want[5]), (i, want[5])
        assert_bit_equal(group[i], want, (n, i))
        assert not torch.equal(want[0], u["m"])             # the update is in
        moved = moved or want[5][-1][0] != u["logA0"]
    assert moved                                            # the optimisers moved: the steps really differ


def test_sixteen_units_and_a_group_of_one(gp):
    """Units inside a group of 16 against the same units alone, and the group of one through the batch entry point
    against the single entry point."""
    units = [unit(case(100, 200 + i), math.log(0.5) - 0.05 * i) for i in range(16)]
    group = gp._estep_chain_full_group(units, 3, NFP)
    for i in range(16):
        assert_bit_equal(group[i], single(gp, units[i], 3), ("16 units", i))
    one = gp._estep_chain_full_group(units[3:4], 3, NFP)
    assert_bit_equal(one[0], single(gp, units[3], 3), "one unit")
    assert_bit_equal(one[0], group[3], "one unit against the same unit in the group of 16")


def estep_raw(gp, c, logA):
    """gpfit_estep as varGP's host loop calls it."""
    n = c["K"].shape[0]
    m_new = torch.empty(n, dtype=torch.float64, device=c["m"].device)
    V_new = torch.empty((n, n), dtype=torch.float64, device=c["m"].device)
    rc = _lib.load().gpfit_estep(gp.get_engine(n, 1)._ctx, gp._stream(), c["K"].data_ptr(), c["K"].stride(0), n,
                                 c["r"].data_ptr(), c["m"].data_ptr(), c["f"].data_ptr(), logA, m_new.data_ptr(),
                                 V_new.data_ptr(), V_new.stride(0))
    assert rc == 0, (rc, _lib.last_error())
    return m_new, V_new


def fparam_lbfgs_raw(gp, lm, lv, r, logA0):
    n = lm.shape[0]
    f = torch.empty(n, dtype=torch.float64, device=lm.device)
    out = (ctypes.c_double * 9)()
    _lib.check(_lib.load().gpfit_fparam_lbfgs(gp.get_engine(n, 1)._ctx, gp._stream(), lm.data_ptr(), lv.data_ptr(), r.data_ptr(),
                                              n, logA0, 0, 0.0, NFP, NFP, 0.1, 1e-7, 1e-9, f.data_ptr(), out),
               "gpfit_fparam_lbfgs")
    return f, list(out)


def test_one_step_of_a_group_against_the_calls_it_stands_for(gp):
    """One step of three units at N = 300 against gpfit_estep, the loop's moments expression (lambda_m = m, lambda_var =
    kv0 + diag V) and gpfit_fparam_lbfgs, unit by unit.  The chain forms A = exp(logA) on the device, gpfit_estep takes the
    host's: where the two agree (record slot 11) every output has the bits of the three calls; where they differ in the
    last bits, the bounds of tests/test_gpu_estep_chain_full.py hold.  logA0 = 0 (exp is exactly 1 on both sides) must take
    the exact branch."""
    logAs = [0.0, math.log(0.5), 0.3]
    cs = [case(300, 600 + i) for i in range(3)]
    group = gp._estep_chain_full_group([unit(c, a) for c, a in zip(cs, logAs)], 1, NFP)
    exact = 0
    for i, (c, logA0, (m1, V1, lm1, lv1, f1, rec)) in enumerate(zip(cs, logAs, group)):
        m2, V2 = estep_raw(gp, c, logA0)
        lm2, lv2 = m2.clone(), c["kv0"] + torch.diagonal(V2)
        f2, out = fparam_lbfgs_raw(gp, lm2, lv2, c["r"], logA0)
        rec = rec[0]
        assert rec[9] == 0 and rec[10] == 1 and rec[6] == 0 and out[6] == 0, (i, rec, out)
        if rec[11] == math.exp(logA0):
            exact += 1
            for name, x, y in (("m", m1, m2), ("V", V1, V2), ("lam_m", lm1, lm2), ("lam_var", lv1, lv2), ("f", f1, f2)):
                assert torch.equal(x, y), (i, name)
            assert same(rec[:9], out), (i, rec, out)
            assert rec[0] != logA0                           # the optimiser moved
        else:
            assert logA0 != 0.0, i
            assert abs(rec[11] - math.exp(logA0)) <= 2 * math.ulp(math.exp(logA0)), (i, rec[11])
            for x, y in ((m1, m2), (V1, V2), (lm1, lm2), (lv1, lv2)):
                assert relerr(x.cpu().numpy(), y.cpu().numpy()) <= TOL_UPDATE, i
            for k in (0, 1):
                assert abs(rec[k] - out[k]) / max(1.0, abs(out[k])) <= TOL_REF, (i, k, rec[k], out[k])
            assert rec[4] == out[4], (i, rec, out)
    print(f"one step of a group of 3 at N = 300: {exact} of 3 units on the exact branch")
    assert group[0][5][0][11] == 1.0 and exact >= 1


def test_a_unit_whose_M_is_not_positive_definite_stops_alone(gp):
    """Unit 1 of three starts from a rate with one entry NaN: M = I + S K S is not positive definite at step 0, its record
    carries the info and nothing else, the records behind it are zero and its arrays come back with the bits they went in
    with; every unit inside the group has the bits of the same unit alone."""
    cs = [case(300, 300 + i) for i in range(3)]
    rng = np.random.default_rng(3)
    f_bad = cs[1]["f"].clone()
    f_bad[7] = float("nan")
    V0, lm0, lv0 = T(rng.standard_normal((300, 300))), T(rng.standard_normal(300)), T(rng.random(300))
    units = [unit(cs[0], math.log(0.5)),
             unit(cs[1], math.log(0.5), f_mean=f_bad, V=V0, lambda_m=lm0, lambda_var=lv0),
             unit(cs[2], math.log(0.4))]
    group = gp._estep_chain_full_group(units, 3, NFP)
    m, V, lm, lv, f, rec = group[1]
    assert rec[0][9] != 0 and rec[0][10] == 0, rec[0]
    assert rec[0][11] == pytest.approx(0.5, rel=1e-15) and rec[0][:9] == [0.0] * 9, rec[0]
    assert rec[1] == [0.0] * 12 and rec[2] == [0.0] * 12, rec
    for x, y in ((m, cs[1]["m"]), (V, V0), (lm, lm0), (lv, lv0), (f, f_bad)):
        assert bits(x, y)
    assert_bit_equal(group[1], single(gp, units[1], 3), "the failing unit in the group against the same unit alone")
    for i in (0, 2):
        want = single(gp, units[i], 3)
        assert ran(want[5]), (i, want[5])
        assert_bit_equal(group[i], want, i)


def test_a_unit_whose_optimiser_fails_stops_alone(gp):
    """kv0[3] = 1e6 in unit 1: the update of step 0 is committed, its moments carry lam_var[3] >= 1e6, so the first
    closure call of the optimiser meets sum f = inf (status 1); f stays and the two steps behind are skipped.  Units 0
    and 2 run their three steps; every unit inside the group has the bits of the same unit alone."""
    cs = [case(300, 400 + i) for i in range(3)]
    kv_bad = cs[1]["kv0"].clone()
    kv_bad[3] = 1.0e6
    units = [unit(cs[0], math.log(0.5)), unit(cs[1], math.log(0.5), kv0=kv_bad), unit(cs[2], math.log(0.6))]
    group = gp._estep_chain_full_group(units, 3, NFP)
    m, V, lm, lv, f, rec = group[1]
    assert rec[0][9] == 0 and rec[0][10] == 1 and int(rec[0][6]) == 1, rec[0]
    assert rec[1] == [0.0] * 12 and rec[2] == [0.0] * 12, rec
    assert torch.equal(f, cs[1]["f"]) and not torch.equal(m, cs[1]["m"]) and float(lv[3]) >= 1.0e6
    assert_bit_equal(group[1], single(gp, units[1], 3), "the failing unit in the group against the same unit alone")
    for i in (0, 2):
        want = single(gp, units[i], 3)
        assert ran(want[5]), (i, want[5])
        assert_bit_equal(group[i], want, i)


def test_refusals_enqueue_nothing(gp):
    """A repeated context, a context whose capacity is too small, a leading dimension of K below N, and two faults of which
    the earlier unit's is named: -3 with a message, and no output or record of any unit changes."""
    from gaussian_processes_amd.engine import GPFitEngine
    N = 300
    engines = gp._group_engines(3, N)
    small = GPFitEngine(100, 1)                              # round_up(300, 128) = 384 is above its capacity
    cs = [case(N, 500 + i) for i in range(3)]

    def requests():
        return [gp._chain_full_prepare(n_steps=2, n_fparam_steps=NFP, engine=e, **unit(c, math.log(0.5)))
                for c, e in zip(cs, engines)]

    def refused(ctxs, qs, word):
        for q in qs:                                         # outputs with known contents (V and the moments start empty)
            for k in ("V", "lam_m", "lam_var"):
                q[k].fill_(7.0)
        before = [{k: q[k].clone() for k in ("m", "f", "V", "lam_m", "lam_var")} for q in qs]
        rec = (ctypes.c_double * (12 * 2 * len(qs)))(*[7.0] * (12 * 2 * len(qs)))
        rc, rec = gp._chain_full_batch_raw(ctxs, qs, rec=rec)
        assert rc == -3, (word, rc)
        assert "gpfit_estep_chain_full_batch: " in _lib.last_error() and word in _lib.last_error(), (word, _lib.last_error())
        torch.cuda.synchronize()
        assert list(rec) == [7.0] * len(rec), word
        for q, b in zip(qs, before):
            for k, v in b.items():
                assert torch.equal(q[k], v), (word, k)

    ctxs = [e._ctx for e in engines]
    refused([ctxs[0], ctxs[1], ctxs[0]], requests(), "every unit needs a context of its own")
    refused([ctxs[0], small._ctx, ctxs[2]], requests(), "unit 1: problem larger than the context capacity")
    qs = requests()
    qs[2]["ldk"] = N - 1
    refused(ctxs, qs, "unit 2: bad argument: bad size or leading dimension")
    qs = requests()
    qs[0]["ldv"] = N - 1
    refused(ctxs, qs, "unit 0: bad argument: bad size or leading dimension")
    # two faults in one call -- unit 1's leading dimension, unit 2 on unit 0's context: the units are checked in order
    qs = requests()
    qs[1]["ldk"] = N - 1
    refused([ctxs[0], ctxs[1], ctxs[0]], qs, "unit 1: bad argument: bad size or leading dimension")
    # and the same three units are accepted as they are
    qs = requests()
    rc, _ = gp._chain_full_batch_raw(ctxs, qs)
    assert rc == 0, _lib.last_error()
    assert not torch.equal(qs[1]["m"], cs[1]["m"])
    small.close()


# ---------------------------------------------------------------------------------------------- varGP_cells
def vargp_args(g, X, ntilde, f_params=None, **fit_kwargs):
    fit_parameters = {"ntilde": ntilde, "maxiter": int(g["maxiter"]), "nEstep": int(g["nEstep"]), "nMstep": int(g["nMstep"]),
                      "nFparamstep": int(g["nFparamstep"]), "kernfun": "acosker", "cellid": 0, "n_px_side": 8,
                      "display_hyper": False}
    fit_parameters.update(fit_kwargs)
    theta = {k: torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for k, v in zip(KEYS, g["theta0"])}
    f_params = f_params or {"logA": syn.F_PARAMS["logA"], "lambda0": syn.F_PARAMS["lambda0"]}
    return {"fit_parameters": fit_parameters, "xtilde": X[:ntilde].clone(), "hyperparams_tuple": (theta, LOWER, UPPER),
            "f_params": {k: torch.tensor(float(v), dtype=torch.float64) for k, v in f_params.items()}}


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
    assert not t.is_alive(), "the fit thread is still running: a fit waits for one that will never arrive"
    if "err" in box:
        raise box["err"]
    return box["out"]


def assert_same_fit(a, b, what):
    (fit, err), (fit1, err1) = a, b
    assert err["is_error"] == err1["is_error"], what
    for group in ("loss_track", "theta_track", "f_par_track"):
        for k, v in fit["values_track"][group].items():
            assert torch.equal(v, fit1["values_track"][group][k]), (what, group, k)
    for k in ("m_b", "V_b"):
        assert torch.equal(fit[k], fit1[k]), (what, k)
    assert fit["f_params"].keys() == fit1["f_params"].keys()
    for k in fit["f_params"]:
        x, y = float(fit["f_params"][k]), float(fit1["f_params"][k])
        assert x == y or (math.isnan(x) and math.isnan(y)), (what, k, x, y)
    for k in KEYS:
        assert float(fit["hyperparams_tuple"][0][k]) == float(fit1["hyperparams_tuple"][0][k]), (what, k)


NEW_LISTS = ("last_full_group_sizes", "last_full_call_seconds", "last_full_closure_group_sizes",
             "last_full_closure_call_seconds")


def test_vargp_cells_is_vargp_cell_by_cell(gp, monkeypatch):
    """Three cells on the full-rank fixture's stimuli (cell 0 is the fixture's).  With FULL_RANK_GROUPS on every fit has
    the bits of varGP on that cell alone in a fresh thread, the chains went out as calls of 3 and closures shared calls,
    all counted in the full-rank lists only, and the fixture's cell meets the fixture within the bounds of
    tests/test_gpu_estep_chain_full.py::test_whole_fit_with_the_chain_on_and_off.  With the switch off: the same fits bit
    for bit, and nothing went through the rendezvous."""
    g = load_golden("g6_vargp_full_N128.npz")
    X, N = T(g["X"]), int(g["N"])
    rng = np.random.default_rng(17)
    rs = [T(g["r"])] + [T(rng.poisson(np.maximum(g["r"].mean(), 0.2), g["r"].shape).astype(np.float64)) for _ in range(2)]
    monkeypatch.setattr(gp, "EIGVAL_TOL", float(g["tol"]))
    kwargs = [vargp_args(g, X, N) for _ in rs]
    alone = [in_a_thread(lambda: gp.varGP(X, r, **copy.deepcopy(kwargs[i]))) for i, r in enumerate(rs)]
    assert not any(err["is_error"] for _, err in alone), [err for _, err in alone]
    assert all(fit["B"].shape[1] == N for fit, _ in alone)             # every eigenvalue kept

    monkeypatch.setattr(gp, "FULL_RANK_GROUPS", True)
    cells = in_a_thread(lambda: gp.varGP_cells(X, rs, copy.deepcopy(kwargs)))
    sizes, closure_sizes = list(gp.varGP_cells.last_full_group_sizes), list(gp.varGP_cells.last_full_closure_group_sizes)
    print(f"full-rank wave of 3: chain calls {sizes}, closure calls {closure_sizes}")
    assert len(cells) == 3 and 3 in sizes and sum(sizes) == 3 * (int(g["maxiter"]) - 1), sizes
    assert max(closure_sizes) >= 2, closure_sizes
    assert len(gp.varGP_cells.last_full_call_seconds) == len(sizes)
    assert len(gp.varGP_cells.last_full_closure_call_seconds) == len(closure_sizes)
    assert list(gp.varGP_cells.last_group_sizes) == [] and list(gp.varGP_cells.last_closure_group_sizes) == []
    for i in range(3):
        assert_same_fit(cells[i], alone[i], ("groups on", i))
    fit = cells[0][0]
    Rt = T(np.random.default_rng(5).poisson(0.7, (4, 6, 1)).astype(np.float64))
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, R_pred, _, _ = gp.test(T(g["Xstar"]), Rt, X_train=X, at_iteration=None, **fit)
    vt = fit["values_track"]
    d = {"track": relerr(vt["loss_track"]["logmarginal"].numpy(), g["logmarginal"]),
         "KL": relerr(vt["loss_track"]["KL"].numpy(), g["KL"]),
         "theta": float(np.abs(np.array([float(fit["hyperparams_tuple"][0][k]) for k in KEYS]) - g["theta_final"]).max()),
         "logA": abs(float(fit["f_params"]["logA"]) - float(g["logA_final"])),
         "prediction": relerr(R_pred.cpu().numpy(), g["R_pred"])}
    print(f"varGP_cells, the fixture's cell against the fixture: {d}")
    assert d["track"] < 1e-6 and d["KL"] < 1e-5 and d["theta"] < 1e-4 and d["logA"] < 1e-4 and d["prediction"] < 1e-4, d

    monkeypatch.setattr(gp, "FULL_RANK_GROUPS", False)
    cells_off = in_a_thread(lambda: gp.varGP_cells(X, rs, copy.deepcopy(kwargs)))
    for name in NEW_LISTS + ("last_group_sizes", "last_closure_group_sizes"):
        assert list(getattr(gp.varGP_cells, name)) == [], name
    for i in range(3):
        assert_same_fit(cells_off[i], alone[i], ("groups off", i))


def test_a_mixed_wave_ends_and_every_fit_is_its_own(gp, monkeypatch):
    """One wave of three on the full-rank fixture's stimuli: a full-rank fit, a sparse fit (ntilde = N / 2) and a full-rank
    fit with a NaN response.  The wave ends; the failing fit's error is varGP's alone (type and message); the two healthy
    fits have the bits of their own varGP, and the two regimes never shared a call."""
    g = load_golden("g6_vargp_full_N128.npz")
    X, N = T(g["X"]), int(g["N"])
    r0 = T(g["r"])
    r1 = T(np.random.default_rng(23).poisson(np.maximum(g["r"].mean(), 0.2), g["r"].shape).astype(np.float64))
    r_nan = r0.clone()
    r_nan[3] = float("nan")
    monkeypatch.setattr(gp, "EIGVAL_TOL", float(g["tol"]))
    monkeypatch.setattr(gp, "FULL_RANK_GROUPS", True)
    rs = [r0, r1, r_nan]
    kwargs = [vargp_args(g, X, N), vargp_args(g, X, N // 2), vargp_args(g, X, N)]
    cells = in_a_thread(lambda: gp.varGP_cells(X, rs, copy.deepcopy(kwargs)))
    v = gp.varGP_cells
    print(f"mixed wave: full-rank chain calls {v.last_full_group_sizes}, full-rank closure calls {v.last_full_closure_group_sizes}, "
          f"projected chain calls {v.last_group_sizes}, sparse closure calls {v.last_closure_group_sizes}")
    assert [err["is_error"] for _, err in cells] == [False, False, True], [err for _, err in cells]
    assert cells[0][0]["B"].shape[1] == N and cells[1][0]["B"].shape[0] == N // 2
    # the healthy full-rank fit chained every iteration; the sparse fit's chains and closures went out alone: the two
    # regimes never share a call
    assert sum(v.last_full_group_sizes) >= int(g["maxiter"]) - 1 and max(v.last_full_group_sizes) <= 2, v.last_full_group_sizes
    assert set(v.last_group_sizes) == {1} and len(v.last_group_sizes) == int(g["maxiter"]) - 1, v.last_group_sizes
    assert len(v.last_full_closure_group_sizes) > 0 and max(v.last_full_closure_group_sizes) <= 2
    assert set(v.last_closure_group_sizes) == {1}, v.last_closure_group_sizes
    for i in range(3):
        alone = in_a_thread(lambda: gp.varGP(X, rs[i], **copy.deepcopy(kwargs[i])))
        if i == 2:
            assert alone[1]["is_error"] and type(alone[1]["error"]) is type(cells[2][1]["error"])
            assert str(alone[1]["error"]) == str(cells[2][1]["error"])
        else:                                                # (the failing fit's tracks hold NaN: not comparable entry by entry)
            assert not alone[1]["is_error"], alone[1]
            assert_same_fit(cells[i], alone, i)
