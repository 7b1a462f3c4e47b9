"""gpfit_fit_eval_sparse_batch (the sparse M-step closures of several independent units as one device call) on the GPU:
every unit against gpfit_fit_eval_sparse on that unit alone, bit for bit; the reference; a failing unit stops alone; the
refusals; and varGP_cells, whose closures now meet like its chains, against the same fits run one after another."""
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
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu
KEYS = syn.THETA_KEYS
LOWER, UPPER = syn.limits()
N_PX = 8                # an 8 x 8 pixel grid
# (N, Ntilde, n_kept per unit): one leaf, ragged, three nb under one padded size; one recursion node (np2 = 384); the
# uneven split 256 + 128 with K = 640 >= 512, where the projections are cut into k slabs
SHAPES = [(200, 120, (70, 101, 120)), (300, 260, (130, 256, 200)), (600, 520, (300, 257, 384))]
# The slabs of a projection are min(splitk_for, what the context's scratch holds) (fit.hip: gemm_splitk), so a closure's
# bits depend on the capacity of the context it runs on -- for the single call as for a unit of a group.  Every
# comparison below therefore runs the single call on the context the unit had in the group; and the contexts of the
# third shape hold 1024 stimuli, so that all four split products (640 x 384 slabs) really are cut in two or more.
CAPACITY = {200: 200, 300: 300, 600: 1024}
# -2log2beta per unit: the first keeps every pixel, the others mask the corners of the grid, each a different number
LOGBETA = (-2.0 * math.log(1.2), 1.3, 1.9)
JOIN_S = 300            # a fit thread still alive after this is a deadlock: the test fails instead of hanging
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def gp():
    from gaussian_processes_amd import utils
    return utils


def T(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).cuda()


def tth(vec):
    return {k: torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for k, v in zip(KEYS, vec)}


def fparams(logA, lambda0):
    return {"logA": torch.tensor(float(logA), dtype=torch.float64), "lambda0": torch.tensor(float(lambda0), dtype=torch.float64)}


@functools.lru_cache(maxsize=None)
def stimuli(N, Nt):
    X = T(syn.stimuli(N, N_PX * N_PX, seed=N))
    return X, X[:Nt].contiguous()


@functools.lru_cache(maxsize=None)
def unit(N, Nt, nk, i, bad_V=False):
    """The arguments of _closure_sparse for unit i of a shape, from seeds: an orthonormal basis of nk columns, an SPD V_b
    (bad_V: one eigenvalue negative), a theta of its own.  Computed once, never written."""
    rng = np.random.default_rng(1000 * N + 10 * nk + i)
    X, xt = stimuli(N, Nt)
    B = T(np.linalg.qr(rng.standard_normal((Nt, nk)))[0])
    Q = np.linalg.qr(rng.standard_normal((nk, nk)))[0]
    ev = 0.05 + rng.random(nk)
    if bad_V:
        ev[nk // 2] = -0.1
    V_b = T((Q * ev) @ Q.T)
    V_b = ((V_b + V_b.T) * 0.5).contiguous()
    th = dict(syn.theta_eval())
    th["-2log2beta"] = LOGBETA[i % 3]
    th["eps_0x"] += 0.03 * i
    th["Amp"] *= 1.0 + 0.02 * i
    return {"theta": tth([th[k] for k in KEYS]), "lims": (LOWER, UPPER), "n_px_side": N_PX, "x": X, "xtilde": xt,
            "r": T(rng.poisson(0.7, N).astype(np.float64)), "B": B, "m_b": T(0.1 * rng.standard_normal(nk)), "V_b": V_b,
            "f_params": fparams(math.log(0.05) + 0.05 * i, -0.3 - 0.02 * i)}


def engines_for(gp, count, n):
    return gp._group_engines(count, CAPACITY.get(n, n), N_PX * N_PX, N_PX * N_PX)


def requests(gp, units, engines):
    return [gp._closure_sparse_prepare(engine=e, **u) for u, e in zip(units, engines)]


def batch(gp, units, engines=None, ctxs=None):
    """gpfit_fit_eval_sparse_batch on the units: (return code, out[16] per unit, rc per unit)."""
    engines = engines or engines_for(gp, len(units), max(units[0]["x"].shape[0], units[0]["xtilde"].shape[0]))
    qs = requests(gp, units, engines)
    rc, out, rcs = gp._closure_batch_raw(ctxs or [e._ctx for e in engines], qs)
    return rc, [list(out[16 * u:16 * u + 16]) for u in range(len(units))], [int(v) for v in rcs]


_SINGLES = {}


def single(gp, u, tag, eng):
    """gpfit_fit_eval_sparse on the unit alone, on the context `eng`: (rc, out[16]); computed once per (tag, context)."""
    key = (tag, eng._ctx.value if hasattr(eng._ctx, "value") else eng._ctx)
    if key not in _SINGLES:
        _SINGLES[key] = gp._closure_run_single(gp._closure_sparse_prepare(engine=eng, **u))
    return _SINGLES[key]


def same(x, y):
    """Lists of floats equal entry by entry, NaN equal to NaN."""
    return len(x) == len(y) and all(p == q or (math.isnan(p) and math.isnan(q)) for p, q in zip(x, y))


# ---------------------------------------------------------------------------------------------- the C entry point
@pytest.mark.parametrize("N,Nt,nks", SHAPES)
def test_every_unit_has_the_bits_of_its_single_closure(gp, N, Nt, nks):
    units = [unit(N, Nt, nk, i) for i, nk in enumerate(nks)]
    engines = engines_for(gp, 3, N)
    assert all(e.n_max >= CAPACITY[N] for e in engines)
    rc, outs, rcs = batch(gp, units, engines)
    assert rc == 0 and rcs == [0, 0, 0], (rc, rcs, _lib.last_error())
    for i, u in enumerate(units):
        rc1, want = single(gp, u, (N, Nt, nks[i], i), engines[i])
        assert rc1 == 0, (i, _lib.last_error())
        assert all(math.isfinite(v) for v in want), (i, want)
        assert same(outs[i], want), (N, Nt, nks, i, outs[i], want)
    assert len({o[0] for o in outs}) == 3, [o[0] for o in outs]          # the units really are different
    assert len({o[13] for o in outs}) == 3, [o[13] for o in outs]        # ... with different masked pixel counts


def test_sixteen_units_and_a_group_of_one(gp):
    N, Nt, _ = SHAPES[0]
    nks = [70 + (50 * i) // 15 for i in range(16)]            # 70 .. 120 under one padded size
    assert nks[0] == 70 and nks[-1] == 120
    units = [unit(N, Nt, nk, i) for i, nk in enumerate(nks)]
    engines = engines_for(gp, 16, N)
    rc, outs, rcs = batch(gp, units, engines)
    assert rc == 0 and rcs == [0] * 16, (rc, rcs, _lib.last_error())
    for i in (0, 5, 9, 15):
        rc1, want = single(gp, units[i], (N, Nt, nks[i], i), engines[i])
        assert rc1 == 0 and same(outs[i], want), ("16 units", i, outs[i], want)
    rc, one, rcs = batch(gp, units[3:4], engines[3:4])
    assert rc == 0 and rcs == [0]
    assert same(one[0], single(gp, units[3], (N, Nt, nks[3], 3), engines[3])[1]), "one unit against the single call"
    assert same(one[0], outs[3]), "one unit against the same unit in the group of 16"


def test_group_against_the_fixture_and_the_reference(gp):
    """g3_closure_sparse_N96_nt40 is the middle unit of three (the bounds of test_gpu_dropin.test_sparse_adjoint_closure);
    the other two, with theta and r perturbed, against oracle.mstep_closure_reference at the project's written bounds
    (1e-9 on the loss, 1e-6 on the gradients)."""
    g = load_golden("g3_closure_sparse_N96_nt40.npz")
    X, B, m_b, V_b = T(g["X"]), T(g["B"]), T(g["m_b"]), T(g["V_b"])
    xt = X[: int(g["ntilde"])].contiguous()
    n_px = int(g["n_px"])
    rng = np.random.default_rng(11)
    logA, lam0 = float(g["logA"]), float(g["lambda0"])
    thetas, rs = [], []
    for i in range(3):
        th = np.array(g["theta"], dtype=np.float64)
        r = np.array(g["r"], dtype=np.float64)
        if i != 1:
            th = th + 0.03 * (i + 1) * rng.standard_normal(6) * np.array([1, 0.3, 0.3, 1, 1, 1])
            r = rng.poisson(np.maximum(r.mean(), 0.2), r.shape).astype(np.float64)
        thetas.append(th)
        rs.append(r)
    units = [{"theta": tth(th), "lims": (LOWER, UPPER), "n_px_side": n_px, "x": X, "xtilde": xt, "r": T(r), "B": B, "m_b": m_b,
              "V_b": V_b, "f_params": fparams(logA, lam0)} for th, r in zip(thetas, rs)]
    engines = gp._group_engines(3, X.shape[0], X.shape[1], n_px * n_px)
    rc, outs, rcs = batch(gp, units, engines)
    assert rc == 0 and rcs == [0, 0, 0], (rc, rcs, _lib.last_error())
    d_loss = abs(outs[1][0] - float(g["loss"])) / abs(float(g["loss"]))
    d_grad = np.abs(np.array(outs[1][3:9]) - g["grad"]).max() / np.abs(g["grad"]).max()
    print(f"the fixture's unit in a group of three: loss {d_loss:.2e}, grad {d_grad:.2e}")
    assert d_loss <= 1e-10 and d_grad <= 1e-8, (d_loss, d_grad)
    for i in (0, 2):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref_loss, ref_grad = orc.mstep_closure_reference(dict(zip(KEYS, thetas[i])), LOWER, UPPER, n_px, X.cpu(), xt.cpu(),
                                                             torch.from_numpy(rs[i]), B.cpu(), m_b.cpu(), V_b.cpu(), logA, lam0,
                                                             tol=float(g["tol"]))
        b = np.array([float(ref_grad[k]) for k in KEYS])
        d_loss = abs(outs[i][0] - float(ref_loss)) / abs(float(ref_loss))
        d_grad = np.abs(np.array(outs[i][3:9]) - b).max() / np.abs(b).max()
        print(f"unit {i} against the reference formulation: loss {d_loss:.2e}, grad {d_grad:.2e}")
        assert d_loss <= 1e-9 and d_grad <= 1e-6, (i, d_loss, d_grad)


def outcome(fn):
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")
        try:
            return fn()
        except Exception as err:
            return err


def same_outcome(a, b):
    if isinstance(a, Exception) or isinstance(b, Exception):
        return type(a) is type(b) and str(a) == str(b)
    return same([a[0]] + [a[1][k] for k in KEYS], [b[0]] + [b[1][k] for k in KEYS])


def test_a_unit_whose_factorisation_fails_stops_alone(gp):
    N, Nt, _ = SHAPES[0]
    units = [unit(N, Nt, 101, 0), unit(N, Nt, 101, 1, bad_V=True), unit(N, Nt, 120, 2)]
    engines = engines_for(gp, 3, N)
    rc, outs, rcs = batch(gp, units, engines)
    assert rc == 0, _lib.last_error()
    assert rcs[1] > 0 and outs[1][15] != 0 and rcs[0] == 0 and rcs[2] == 0, (rcs, outs[1])
    assert rcs[1] == single(gp, units[1], "bad V", engines[1])[0]
    for i, tag in ((0, (N, Nt, 101, 0)), (2, (N, Nt, 120, 2))):
        assert same(outs[i], single(gp, units[i], tag, engines[i])[1]), i
    # through the Python layer: the failing unit takes the step-by-step formulation, alone
    group = outcome(lambda: gp._closure_sparse_group(units))
    assert not isinstance(group, Exception), group
    for i, u in enumerate(units):
        alone = outcome(lambda: gp._closure_sparse(**u))
        assert same_outcome(group[i], alone), (i, group[i], alone)
    assert not isinstance(group[0], Exception) and group[0][0] == outs[0][0]


def test_a_unit_outside_its_limits_gets_the_infinite_loss_alone(gp):
    N, Nt, _ = SHAPES[0]
    out_of_box = dict(unit(N, Nt, 101, 1))
    th = [float(v.detach()) for v in out_of_box["theta"].values()]
    th[1] = 1.5                                              # eps_0x above its upper limit of 1
    out_of_box["theta"] = tth(th)
    units = [unit(N, Nt, 101, 0), out_of_box, unit(N, Nt, 120, 2)]
    engines = engines_for(gp, 3, N)
    rc, outs, rcs = batch(gp, units, engines)
    assert rc == 0 and rcs == [0, -2, 0], (rc, rcs, _lib.last_error())
    assert outs[1][0] == math.inf and all(v == math.inf for v in outs[1][3:9]), outs[1]
    for i, tag in ((0, (N, Nt, 101, 0)), (2, (N, Nt, 120, 2))):
        assert same(outs[i], single(gp, units[i], tag, engines[i])[1]), i
    group = outcome(lambda: gp._closure_sparse_group(units))
    alone = outcome(lambda: gp._closure_sparse(**out_of_box))
    assert isinstance(alone, ValueError) and "eps_0x" in str(alone), alone
    assert same_outcome(group[1], alone), (group[1], alone)


def test_refusals_enqueue_nothing(gp):
    """17 units, a repeated context, mixed padded sizes, a null operand, n_kept > Ntilde and a context too small: a return
    value below 0 with a message naming the cause, and neither out_host nor rc_out changes."""
    N, Nt, nks = SHAPES[1]
    engines = engines_for(gp, 3, N)
    good = [unit(N, Nt, nk, i) for i, nk in enumerate(nks)]

    def raw(ctxs, qs):
        out = (ctypes.c_double * (16 * len(qs)))(*([SENTINEL] * (16 * len(qs))))
        rcs = (ctypes.c_int * len(qs))(*([77] * len(qs)))
        rc, _, _ = gp._closure_batch_raw(ctxs, qs, out, rcs)
        return rc, list(out), list(rcs)

    def refused(ctxs, qs, word):
        rc, out, rcs = raw(ctxs, qs)
        assert rc < 0, (word, rc)
        assert word in _lib.last_error(), (word, _lib.last_error())
        assert all(v == SENTINEL for v in out) and all(v == 77 for v in rcs), word

    ctxs = [e._ctx for e in engines]
    qs = requests(gp, good, engines)
    refused((ctxs * 6)[:17], (qs * 6)[:17], "units per call")
    refused([ctxs[0], ctxs[1], ctxs[0]], qs, "context of its own")
    refused(ctxs, requests(gp, [good[0], unit(N, Nt, 100, 1), good[2]], engines), "round_up(n_kept, 128)")
    qs = requests(gp, good, engines)
    qs[1]["m_b"] = None
    refused(ctxs, qs, "null")
    qs = requests(gp, good, engines)
    qs[2]["n_kept"] = Nt + 1
    refused(ctxs, qs, "n_kept")
    # two faults in one call -- unit 1's V_b narrower than n_kept, unit 2 on unit 0's context: the units are checked in order
    qs = requests(gp, good, engines)
    qs[1]["V_b"] = qs[1]["V_b"][:, :-1].contiguous()
    refused([ctxs[0], ctxs[1], ctxs[0]], qs, "gpfit_fit_eval_sparse_batch: unit 1: bad leading dimension")
    small = gp.GPFitEngine(128, N_PX * N_PX, N_PX * N_PX, device=engines[0].device)
    refused([ctxs[0], ctxs[1], small._ctx], requests(gp, good, engines), "capacity")
    # and the same three units are accepted as they are
    rc, out, rcs = raw(ctxs, requests(gp, good, engines))
    assert rc == 0 and rcs == [0, 0, 0], (_lib.last_error(), rcs)
    assert all(v != SENTINEL and math.isfinite(v) for v in out)


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


def test_vargp_cells_closures_meet_and_every_fit_is_vargp_alone(gp, monkeypatch):
    """Three cells in the sparse regime at the shape of g6_vargp_sparse_N128_nt64 (cell 0 is the fixture's): every fit has
    the bits of varGP on that cell alone, the closures went out as calls of up to 3 units -- as many unit-calls as the
    three fits make device calls alone -- the chains as before, and the fixture's cell meets the fixture within the
    bounds of test_vargp_end_to_end_matches_reference."""
    g = load_golden("g6_vargp_sparse_N128_nt64.npz")
    X, ntilde = T(g["X"]), int(g["ntilde"])
    rng = np.random.default_rng(17)
    rs = [T(g["r"])] + [T(rng.poisson(np.maximum(g["r"].mean(), 0.2), g["r"].shape).astype(np.float64)) for _ in range(2)]
    monkeypatch.setattr(gp, "EIGVAL_TOL", float(g["tol"]))
    kwargs = [vargp_args(g, X, ntilde) for _ in rs]
    cells = in_a_thread(lambda: gp.varGP_cells(X, rs, copy.deepcopy(kwargs)))
    sizes, closure_sizes = list(gp.varGP_cells.last_group_sizes), list(gp.varGP_cells.last_closure_group_sizes)
    assert len(gp.varGP_cells.last_closure_call_seconds) == len(closure_sizes)
    assert gp.varGP_cells.last_seconds_in_closure_call > 0.0
    assert len(cells) == 3 and 3 in sizes and sum(sizes) == 3 * (int(g["maxiter"]) - 1), sizes
    assert 3 in closure_sizes and all(1 <= n <= 3 for n in closure_sizes), closure_sizes
    # alone: count the device calls of _closure_sparse by wrapping its prepare step
    calls = [0]
    prepare = gp._closure_sparse_prepare

    def counting(*a, **k):
        calls[0] += 1
        return prepare(*a, **k)
    monkeypatch.setattr(gp, "_closure_sparse_prepare", counting)
    for i, r in enumerate(rs):
        alone = in_a_thread(lambda: gp.varGP(X, r, **copy.deepcopy(kwargs[i])))
        assert not alone[1]["is_error"], alone[1]
        assert_same_fit(cells[i], alone, i)
    monkeypatch.setattr(gp, "_closure_sparse_prepare", prepare)
    print(f"closure calls by units carried: {closure_sizes}; device calls of the three fits alone: {calls[0]}")
    assert calls[0] > 0 and sum(closure_sizes) == calls[0], (closure_sizes, calls[0])
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
    assert fit["B"].shape[1] == int(g["n_kept"])
    assert d["track"] < 1e-5 and d["KL"] < 1e-4 and d["theta"] < 1e-4 and d["logA"] < 1e-4 and d["prediction"] < 1e-4, d


def test_a_mixed_wave_ends_and_its_closures_still_meet(gp, monkeypatch):
    """The wave of four of test_gpu_estep_chain_group: two ordinary cells, one whose f_params carry loglambda0 (keeps its
    host loop and its own closure calls) and one with a NaN response.  The wave ends, the ordinary cells have the bits of
    their own varGP, and some closure call carried at least two units."""
    g = load_golden("g6_vargp_sparse_N128_nt64.npz")
    X, ntilde = T(g["X"]), int(g["ntilde"])
    rng = np.random.default_rng(23)
    r0 = T(g["r"])
    r1 = T(rng.poisson(np.maximum(g["r"].mean(), 0.2), g["r"].shape).astype(np.float64))
    r_nan = r0.clone()
    r_nan[3] = float("nan")
    monkeypatch.setattr(gp, "EIGVAL_TOL", float(g["tol"]))
    rs = [r0, r0, r_nan, r1]
    kwargs = [vargp_args(g, X, ntilde),
              vargp_args(g, X, ntilde, f_params={"logA": syn.F_PARAMS["logA"], "loglambda0": -1.0}),
              vargp_args(g, X, ntilde), vargp_args(g, X, ntilde)]
    cells = in_a_thread(lambda: gp.varGP_cells(X, rs, copy.deepcopy(kwargs)))
    closure_sizes = list(gp.varGP_cells.last_closure_group_sizes)
    print(f"closure calls with a loglambda0 fit and a failing fit in the wave: {closure_sizes}")
    assert [err["is_error"] for _, err in cells] == [False, False, True, False], [err for _, err in cells]
    assert max(closure_sizes) >= 2 and all(1 <= n <= 3 for n in closure_sizes), closure_sizes
    for i in (0, 3):
        alone = in_a_thread(lambda: gp.varGP(X, rs[i], **copy.deepcopy(kwargs[i])))
        assert_same_fit(cells[i], alone, i)
