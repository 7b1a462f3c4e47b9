"""gpfit_estep_chain_batch (the E-step chains of several independent units as one lock-step device call) on the GPU:
every unit inside a group against the same unit alone (gpfit_estep_chain, the group of one of the same implementation),
bit for bit; one step of a group against the un-chained calls it stands for; a failing unit stops alone; the refusals;
and varGP_cells against the same fits run one after another."""
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
NFP = 10                # nFparamstep of the lab's fits
# (N, nb per unit): one leaf, ragged rows, different nb under one padded size; one recursion node; the uneven split
# 256 + 128; many row slices
SHAPES = [(200, (70, 128, 101)), (300, (130, 256, 200)), (300, (300, 257, 384)), (1000, (128, 128))]
JOIN_S = 300            # a fit thread still alive after this is a deadlock: the test fails instead of hanging


@pytest.fixture(scope="module")
def gp():
    from gaussian_processes_amd import utils
    return utils


def T(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).cuda()


@functools.lru_cache(maxsize=None)
def case(nt, nb, seed):
    """The inputs of tests/test_gpu_estep_chain.py's case(), from the given seed; computed once, never written."""
    from gaussian_processes_amd import utils as gp
    rng = np.random.default_rng(seed)
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


def unit(c, logA0, fixed=None, **over):
    u = {"r": c["r"], "KKtilde_inv": c["a"], "aL": c["aL"], "L": c["L"], "kv0": c["kv0"], "m": c["m"], "f_mean": c["f"],
         "logA0": logA0, "lambda0_fixed": fixed}
    u.update(over)
    return u


def single(gp, u, n_steps, nfp=NFP):
    """The unit alone: gpfit_estep_chain, the group of one."""
    return gp._estep_chain(n_steps=n_steps, n_fparam_steps=nfp, **u)


def same(x, y):
    """Lists of floats equal entry by entry, NaN equal to NaN."""
    return len(x) == len(y) and all(p == q or (math.isnan(p) and math.isnan(q)) for p, q in zip(x, y))


def assert_bit_equal(got, want, what):
    for name, x, y in zip(("m", "V", "lam_m", "lam_var", "f"), got[:5], want[:5]):
        assert torch.equal(x, y), (what, name)
    assert len(got[5]) == len(want[5])
    for k, (p, q) in enumerate(zip(got[5], want[5])):
        assert same(p, q), (what, k, p, q)


@pytest.mark.parametrize("fixed", [None, math.exp(-1.0)])
@pytest.mark.parametrize("n_steps", [1, 3])
@pytest.mark.parametrize("nt,nbs", SHAPES)
def test_every_unit_has_the_bits_of_its_single_chain(gp, nt, nbs, n_steps, fixed):
    """A unit inside a group against the same unit alone."""
    units = [unit(case(nt, nb, 100 + i), math.log(0.5) + 0.1 * i, fixed) for i, nb in enumerate(nbs)]
    group = gp._estep_chain_group(units, n_steps, NFP)
    assert len(group) == len(units)
    moved = False
    for i, u in enumerate(units):
        want = single(gp, u, n_steps)
        assert all(rec[9] == 0 and rec[10] == 1 and rec[6] == 0 for rec in want[5]), (i, want[5])
        assert_bit_equal(group[i], want, (nt, nbs, i))
        moved = moved or want[5][-1][0] != u["logA0"]
    assert moved                                            # the optimisers moved: the steps really differ


def test_one_step_of_a_group_against_the_existing_pair(gp):
    """The group's own anchor in code the chain does not share: three units at N = 200 (nb = 70, 128, 101 under one padded
    size), one step, against _estep_projected(kv0=) followed by gpfit_fparam_lbfgs unit by unit (tests/
    test_gpu_estep_chain.py::test_one_step_against_the_existing_pair).  logA0 = 0 for all: exp is exactly 1 on the device
    and on the host, so this is the exact branch and every output and the optimiser's nine results have the pair's bits."""
    nt, nbs = SHAPES[0]
    assert (nt, nbs) == (200, (70, 128, 101))
    cs = [case(nt, nb, 600 + i) for i, nb in enumerate(nbs)]
    group = gp._estep_chain_group([unit(c, 0.0) for c in cs], 1, NFP)
    assert len(group) == 3
    for i, (c, (m1, V1, lm1, lv1, f1, rec)) in enumerate(zip(cs, group)):
        fp = {"logA": torch.tensor(0.0, dtype=torch.float64)}
        m2, V2, lm2, lv2 = gp._estep_projected(c["r"], c["a"], c["aL"], c["L"], c["m"], fp, c["f"], kv0=c["kv0"])
        n = lm2.shape[0]
        f2 = torch.empty(n, dtype=torch.float64, device=lm2.device)
        out = (ctypes.c_double * 9)()
        _lib.check(_lib.load().gpfit_fparam_lbfgs(gp.get_engine(n, 1)._ctx, gp._stream(), lm2.data_ptr(), lv2.data_ptr(),
                                                  c["r"].data_ptr(), n, 0.0, 0, 0.0, NFP, NFP, 0.1, 1e-7, 1e-9, f2.data_ptr(),
                                                  out), "gpfit_fparam_lbfgs")
        rec, out = rec[0], list(out)
        assert rec[9] == 0 and rec[10] == 1 and rec[6] == 0 and out[6] == 0, (i, rec, out)
        assert rec[11] == 1.0, (i, rec[11])
        for name, x, y in (("m", m1, m2), ("V", V1, V2), ("lam_m", lm1, lm2), ("lam_var", lv1, lv2), ("f", f1, f2)):
            assert torch.equal(x, y), (i, name)
        assert same(rec[:9], out), (i, rec, out)
        assert rec[0] != 0.0                                # the optimiser moved


def test_sixteen_units_and_a_group_of_one(gp):
    """Units inside a group of 16 against the same units alone, and the group of one through the batch entry point
    against the single entry point."""
    nbs = [70 + (58 * i) // 15 for i in range(16)]          # 70 .. 128 under one padded size
    assert nbs[0] == 70 and nbs[-1] == 128
    units = [unit(case(200, nb, 200 + i), math.log(0.5) - 0.05 * i) for i, nb in enumerate(nbs)]
    group = gp._estep_chain_group(units, 3, NFP)
    for i in (0, 5, 9, 15):
        assert_bit_equal(group[i], single(gp, units[i], 3), ("16 units", i))
    one = gp._estep_chain_group(units[3:4], 3, NFP)
    assert_bit_equal(one[0], single(gp, units[3], 3), "one unit")
    assert_bit_equal(one[0], group[3], "one unit against the same unit in the group of 16")


def test_a_unit_whose_W_is_not_positive_definite_stops_alone(gp):
    """Unit 1 of three starts from a rate with one entry inf (test_non_finite_rate_stops_the_chain): its record carries
    the info and nothing else, its arrays come back with the bits they went in with; every unit inside the group has the
    bits of the same unit alone."""
    cs = [case(200, 128, 300 + i) for i in range(3)]
    rng = np.random.default_rng(3)
    f_bad = cs[1]["f"].clone()
    f_bad[7] = float("inf")
    V0, lm0, lv0 = T(rng.standard_normal((128, 128))), T(rng.standard_normal(200)), T(rng.random(200))
    units = [unit(cs[0], math.log(0.5)),
             unit(cs[1], math.log(0.5), f_mean=f_bad, V=V0, lambda_m=lm0, lambda_var=lv0),
             unit(cs[2], math.log(0.4))]
    group = gp._estep_chain_group(units, 3, NFP)
    m, V, lm, lv, f, rec = group[1]
    assert rec[0][9] != 0 and rec[0][10] == 0, rec[0]
    assert rec[0][11] == pytest.approx(0.5, rel=1e-15) and rec[0][:9] == [0.0] * 9, rec[0]
    assert rec[1] == [0.0] * 12 and rec[2] == [0.0] * 12, rec
    for x, y in ((m, cs[1]["m"]), (V, V0), (lm, lm0), (lv, lv0), (f, f_bad)):
        assert torch.equal(x, y)
    assert_bit_equal(group[1], single(gp, units[1], 3), "the failing unit in the group against the same unit alone")
    for i in (0, 2):
        want = single(gp, units[i], 3)
        assert all(rec[9] == 0 and rec[10] == 1 and rec[6] == 0 for rec in want[5]), (i, want[5])
        assert_bit_equal(group[i], want, i)


def test_a_unit_whose_optimiser_fails_stops_alone(gp):
    """kv0[3] = 1e6 in unit 1: the update of step 0 is committed, its moments carry lam_var[3] >= 1e6, so the first
    closure call of the optimiser meets sum f = inf (status 1); f stays and the two steps behind are skipped.  Units 0
    and 2 run their three steps; every unit inside the group has the bits of the same unit alone."""
    cs = [case(200, 128, 400 + i) for i in range(3)]
    kv_bad = cs[1]["kv0"].clone()
    kv_bad[3] = 1.0e6
    units = [unit(cs[0], math.log(0.5)), unit(cs[1], math.log(0.5), kv0=kv_bad), unit(cs[2], math.log(0.6))]
    group = gp._estep_chain_group(units, 3, NFP)
    m, V, lm, lv, f, rec = group[1]
    assert rec[0][9] == 0 and rec[0][10] == 1 and int(rec[0][6]) == 1, rec[0]
    assert rec[1] == [0.0] * 12 and rec[2] == [0.0] * 12, rec
    assert torch.equal(f, cs[1]["f"]) and not torch.equal(m, cs[1]["m"]) and float(lv[3]) >= 1.0e6
    assert_bit_equal(group[1], single(gp, units[1], 3), "the failing unit in the group against the same unit alone")
    for i in (0, 2):
        want = single(gp, units[i], 3)
        assert all(rec[9] == 0 and rec[10] == 1 and rec[6] == 0 for rec in want[5]), (i, want[5])
        assert_bit_equal(group[i], want, i)


def test_refusals_enqueue_nothing(gp):
    """17 units, a repeated context, mixed padded sizes, a null unit pointer, and two faults of which the earlier unit's is
    named: -3 with a message, and no output of any unit changes."""
    engines = gp._group_engines(3, 200)
    cs = [case(200, 128, 500 + i) for i in range(3)]
    odd = case(200, 130, 503)                                # round_up(130, 128) = 256

    def requests(cases):
        return [gp._chain_prepare(n_steps=2, n_fparam_steps=NFP, engine=e, **unit(c, math.log(0.5)))
                for c, e in zip(cases, engines)]

    def refused(ctxs, qs, word):
        before = [{k: q[k].clone() for k in ("m", "f", "V", "lam_m", "lam_var") if q[k] is not None} for q in qs]
        for b in before:                                     # outputs with known contents (V and the moments start empty)
            for k in ("V", "lam_m", "lam_var"):
                b[k].fill_(7.0)
        for q, b in zip(qs, before):
            for k in ("V", "lam_m", "lam_var"):
                q[k].copy_(b[k])
        rc, _ = gp._chain_batch_raw(ctxs, qs)
        assert rc == -3, (word, rc)
        assert word in _lib.last_error(), (word, _lib.last_error())
        for q, b in zip(qs, before):
            for k, v in b.items():
                assert torch.equal(q[k], v), (word, k)

    ctxs = [e._ctx for e in engines]
    qs = requests(cs)
    refused((ctxs * 6)[:17], (qs * 6)[:17], "units per call")
    refused([ctxs[0], ctxs[1], ctxs[0]], qs, "context of its own")
    refused(ctxs, requests([cs[0], odd, cs[2]]), "round_up(nb, 128)")
    qs = requests(cs)
    qs[1]["m"] = None
    refused(ctxs, qs, "null")
    # two faults in one call -- unit 1's V narrower than nb, unit 2 on unit 0's context: the units are checked in order
    qs = requests(cs)
    qs[1]["V"] = torch.empty(128, 64, dtype=torch.float64, device="cuda")
    refused([ctxs[0], ctxs[1], ctxs[0]], qs, "unit 1: bad argument: bad size or leading dimension")
    # and the same three units are accepted as they are
    qs = requests(cs)
    rc, _ = gp._chain_batch_raw(ctxs, qs)
    assert rc == 0, _lib.last_error()
    assert not torch.equal(qs[1]["m"], cs[1]["m"])


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


def test_vargp_cells_is_vargp_cell_by_cell(gp, monkeypatch):
    """Three cells in the sparse regime at the shape of g6_vargp_sparse_N128_nt64 (cell 0 is the fixture's): every fit
    has the bits of varGP on that cell alone in a fresh thread, the chains went out as calls of 3, and the fixture's
    cell meets the fixture within the bounds of test_vargp_end_to_end_matches_reference."""
    g = load_golden("g6_vargp_sparse_N128_nt64.npz")
    X, ntilde = T(g["X"]), int(g["ntilde"])
    rng = np.random.default_rng(17)
    rs = [T(g["r"])] + [T(rng.poisson(np.maximum(g["r"].mean(), 0.2), g["r"].shape).astype(np.float64)) for _ in range(2)]
    monkeypatch.setattr(gp, "EIGVAL_TOL", float(g["tol"]))
    kwargs = [vargp_args(g, X, ntilde) for _ in rs]
    cells = in_a_thread(lambda: gp.varGP_cells(X, rs, copy.deepcopy(kwargs)))
    sizes = list(gp.varGP_cells.last_group_sizes)
    assert len(cells) == 3 and 3 in sizes and sum(sizes) == 3 * (int(g["maxiter"]) - 1), sizes
    for i, r in enumerate(rs):
        alone = in_a_thread(lambda: gp.varGP(X, r, **copy.deepcopy(kwargs[i])))
        assert not alone[1]["is_error"], alone[1]
        assert_same_fit(cells[i], alone, i)
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
    print(f"varGP_cells, the fixture's cell against the fixture: {d}; group sizes {sizes}")
    assert fit["B"].shape[1] == int(g["n_kept"])
    assert d["track"] < 1e-5 and d["KL"] < 1e-4 and d["theta"] < 1e-4 and d["logA"] < 1e-4 and d["prediction"] < 1e-4, d


def test_vargp_cells_with_fits_that_do_not_chain_or_fail(gp, monkeypatch):
    """One wave of four: two ordinary cells, one whose f_params carry loglambda0 (keeps its host loop: never arrives)
    and one with a NaN response (varGP returns an error dict).  Nobody waits for a fit that will not come: the wave
    ends, the two ordinary cells have the bits of their own varGP and shared their chain calls."""
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
    sizes = list(gp.varGP_cells.last_group_sizes)
    print(f"group sizes with a loglambda0 fit and a failing fit in the wave: {sizes}")
    assert [err["is_error"] for _, err in cells] == [False, False, True, False], [err for _, err in cells]
    assert max(sizes) >= 2 and all(1 <= n <= 3 for n in sizes), sizes
    for i in range(4):
        alone = in_a_thread(lambda: gp.varGP(X, rs[i], **copy.deepcopy(kwargs[i])))
        if i == 2:
            assert alone[1]["is_error"] and type(alone[1]["error"]) is type(cells[2][1]["error"])
            assert str(alone[1]["error"]) == str(cells[2][1]["error"])
        else:                                                # (the failing fit's tracks hold NaN: not comparable entry by entry)
            assert_same_fit(cells[i], alone, i)
