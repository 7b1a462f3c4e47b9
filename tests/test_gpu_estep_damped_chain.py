"""gpfit_estep_chain_damped / _batch (the damped E-steps between two kernel rebuilds as one device call, alone and in
groups) on the GPU: against itself step by step, against the calls a step stands for (gpfit_estep_projected_damped,
gpfit_fparam_lbfgs, utils.lambda_moments), against the numpy restatement of the loop
(estep_damped_chain_cases.loop), the fallback decided on the device for a V that is not positive definite, groups
against their units alone, and varGP / varGP_cells with the switch on and off.

Shapes (N, nb): (64, 64) one 128-leaf per chain, no recursion; (200, 130) padded to 256, ragged rows, both chains
recurse; (1000, 300) padded to 384, an odd tile count.  Inputs: estep_damped_cases.make_case(.., 1e4, "newton"), the
factors of K~ from utils.cholesky(K, want_inverse=True)."""
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

import estep_damped_cases as cases
import estep_damped_chain_cases as loops
from conftest import load_golden, relerr
from gaussian_processes_amd import _lib, synthetic as syn

pytestmark = pytest.mark.gpu
KEYS = syn.THETA_KEYS
LOWER, UPPER = syn.limits()
SHAPES = [(64, 64), (200, 130), (1000, 300)]
ALPHAS = [0.5, 0.05]
NFP = 10                # nFparamstep of the lab's fits
TOL_REF = 1e-6          # logA / lambda0 between the device's and the host's exp (tests/test_gpu_fparam_lbfgs.py)
TOL_UPDATE = 1e-10      # m, V and the moments (TOL_UPDATE of tests/test_gpu_estep_chain.py)
TOL_LOOP = 1e-9         # against the restatement (tests/test_gpu_estep_damped.py)
JOIN_S = 600


@pytest.fixture(scope="module")
def gp():
    from gaussian_processes_amd import utils
    return utils


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


@functools.lru_cache(maxsize=None)
def case(N, nb, seed=0):
    """The numpy case and its device operands; computed once per shape and seed, never written."""
    from gaussian_processes_amd import utils as gp
    c = cases.make_case(N, nb, 1e4, "newton", seed=seed)
    K, a = T(c["K"]), T(c["a"])
    L, Linv, _, info = gp.cholesky(K, want_inverse=True)
    assert info == 0
    kv0 = loops.kv0_of(N, seed)
    Kb = gp.matmul(a, K)
    d = {"np": c, "kv0_np": kv0, "r": T(c["r"]), "a": a, "aL": gp.matmul(a, L), "L": L, "Linv": Linv, "kv0": T(kv0),
         "m": T(c["m"]), "f": T(c["f"]), "V": T(c["V"]), "Vbad": T(loops.indefinite(c["V"])), "Kb": Kb,
         "Kvec": T(kv0) + torch.sum(Kb * a, 1)}
    return d


def chain(gp, c, m, V, f, logA0, n_steps, alpha, nfp=NFP, **state):
    return gp._estep_chain_damped(c["r"], c["a"], c["aL"], c["L"], c["Linv"], c["kv0"], V, m, f, logA0, alpha, n_steps, nfp,
                                  **state)


def unit(c, V=None, f=None, logA0=0.1):
    return {"r": c["r"], "KKtilde_inv": c["a"], "aL": c["aL"], "L": c["L"], "Linv": c["Linv"], "kv0": c["kv0"],
            "V": c["V"] if V is None else V, "m": c["m"], "f_mean": c["f"] if f is None else f, "logA0": logA0}


def fparam_lbfgs_raw(gp, lm, lv, r, logA0, max_iter):
    n = lm.shape[0]
    eng = gp.get_engine(n, 1)
    f = torch.empty(n, dtype=torch.float64, device=lm.device)
    out = (ctypes.c_double * 9)()
    _lib.check(_lib.load().gpfit_fparam_lbfgs(eng._ctx, gp._stream(), lm.data_ptr(), lv.data_ptr(), r.data_ptr(), n, logA0,
                                              0, 0.0, max_iter, max_iter, 0.1, 1e-7, 1e-9, f.data_ptr(), out),
               "gpfit_fparam_lbfgs")
    return f, list(out)


def same(x, y):
    """Lists of floats equal entry by entry, NaN equal to NaN."""
    return len(x) == len(y) and all(p == q or (math.isnan(p) and math.isnan(q)) for p, q in zip(x, y))


def same_result(x, y):
    return all(torch.equal(p, q) for p, q in zip(x[:5], y[:5])) and all(same(p, q) for p, q in zip(x[5], y[5]))


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("N,nb", SHAPES)
def test_chaining_is_exact(gp, N, nb, alpha):
    """chain(3) against three chain(1), each fed the m, V, f and logA (slot 0 of its record) of the one before."""
    c = case(N, nb)
    logA0 = 0.1
    m3, V3, lm3, lv3, f3, rec3 = chain(gp, c, c["m"], c["V"], c["f"], logA0, 3, alpha)
    m, V, f, logA = c["m"], c["V"], c["f"], logA0
    for k in range(3):
        m, V, lm, lv, f, rec = chain(gp, c, m, V, f, logA, 1, alpha)
        assert rec[0][9] == 0 and rec[0][10] == 1 and rec[0][6] == 0, (k, rec)
        assert same(rec[0], rec3[k]), (k, rec[0], rec3[k])
        logA = rec[0][0]
    assert logA != logA0                                  # the optimiser moved: the steps really differ
    for x, y in ((m, m3), (V, V3), (lm, lm3), (lv, lv3), (f, f3)):
        assert torch.equal(x, y)
    assert torch.equal(c["V"], T(c["np"]["V"])) and torch.equal(c["m"], T(c["np"]["m"]))     # the arguments are left alone


@pytest.mark.parametrize("N,nb", SHAPES)
def test_one_step_against_the_existing_calls(gp, N, nb):
    """chain(1) against _estep_projected_damped, gpfit_fparam_lbfgs on the chain's own moments, and utils.lambda_moments
    on the committed (m, V).  The chain forms A = exp(logA) on the device, the single call takes the host's: where the
    two agree (record slot 11) the update has the single call's bits; where they differ in the last bit it agrees to
    rounding.  logA0 = 0 (exp is exactly 1 on both sides) must take the exact branch.  The optimiser starts from logA0
    itself either way, so its nine results and the rate have the bits of gpfit_fparam_lbfgs on the returned moments."""
    c = case(N, nb)
    exact = total = 0
    for alpha in ALPHAS:
        for logA0 in (0.0, math.log(0.5), 0.3, -1.2, 0.77, -0.4321):
            what = (N, nb, alpha, logA0)
            m1, V1, lm1, lv1, f1, rec = chain(gp, c, c["m"], c["V"], c["f"], logA0, 1, alpha)
            fp = {"logA": torch.tensor(logA0, dtype=torch.float64)}
            m2, V2 = gp._estep_projected_damped(c["r"], c["a"], c["aL"], c["L"], c["Linv"], c["V"], c["m"], fp, c["f"], alpha)
            f2, out = fparam_lbfgs_raw(gp, lm1, lv1, c["r"], logA0, NFP)
            lm2, lv2 = gp.lambda_moments(None, None, c["a"], c["Kvec"], c["Kb"], None, m1, V1, None)
            rec = rec[0]
            assert rec[9] == 0 and rec[10] == 1 and rec[6] == 0 and out[6] == 0, (what, rec, out)
            total += 1
            if rec[11] == math.exp(logA0):
                exact += 1
                assert torch.equal(m1, m2) and torch.equal(V1, V2), what
            else:
                assert logA0 != 0.0, what
                assert abs(rec[11] - math.exp(logA0)) <= 2 * math.ulp(math.exp(logA0)), (what, rec[11])
                for x, y in ((m1, m2), (V1, V2)):
                    assert relerr(x.cpu().numpy(), y.cpu().numpy()) <= TOL_UPDATE, what
            assert same(rec[:9], out) and torch.equal(f1, f2), (what, rec, out)
            em, ev = relerr(lm1.cpu().numpy(), lm2.cpu().numpy()), relerr(lv1.cpu().numpy(), lv2.cpu().numpy())
            assert em <= TOL_UPDATE and ev <= TOL_UPDATE, (what, em, ev)
            assert torch.equal(V1, V1.T), what
    print(f"N {N} nb {nb}: chain(1) against the single call: {exact} of {total} cases exact (the device's exp(logA0) "
          f"equal to the host's)")


@functools.lru_cache(maxsize=None)
def restated(N, nb, alpha, bad):
    c = case(N, nb)
    V0 = loops.indefinite(c["np"]["V"]) if bad else None
    return loops.loop(c["np"], c["kv0_np"], alpha, 3, NFP, loops.cholesky_update, V=V0)


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("N,nb", SHAPES)
def test_three_steps_against_the_restatement(gp, N, nb, alpha):
    """(m, V) behind 3 steps against the CPU loop (cholesky_estep, the moments, gpfit_fparam_lbfgs_host) from the same
    start, each side with its own optimiser of nFparamstep steps; V exactly symmetric with a Cholesky factor."""
    c = case(N, nb)
    m, V, lm, lv, f, rec = chain(gp, c, c["m"], c["V"], c["f"], float(c["np"]["logA"]), 3, alpha)
    ref = restated(N, nb, alpha, False)
    assert [r_[10] for r_ in rec] == [1, 1, 1] and all(r_[9] == 0 and r_[6] == 0 for r_ in rec), rec
    em, ev = relerr(m.cpu().numpy(), ref[-1]["m"]), relerr(V.cpu().numpy(), ref[-1]["V"])
    dl = [abs(r_[0] - s["logA"]) for r_, s in zip(rec, ref)]
    print(f"N {N} nb {nb} alpha {alpha}: after 3 steps relerr m {em:.2e} V {ev:.2e}; |logA - logA_cpu| per step {dl}")
    assert em < TOL_LOOP and ev < TOL_LOOP, (em, ev, dl)
    assert torch.equal(V, V.T) and gp.cholesky(V)[3] == 0


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("N,nb", SHAPES)
def test_fallback_to_the_full_step_on_the_device(gp, N, nb, alpha):
    """V minus 2 lambda_max v v^T along its top eigenvector is indefinite: step 0 is committed as the full step (slot 10
    reads 2, its (m, V) those of _estep_projected at equal A: logA0 = 0), steps 1 and 2 are damped; chain(3) is
    chain(1) + chain(2) bit for bit; and a non-finite rate still stops the chain at step 0 with nothing written."""
    c = case(N, nb)
    logA0 = 0.0
    assert gp.cholesky(c["Vbad"])[3] != 0
    m3, V3, lm3, lv3, f3, rec3 = chain(gp, c, c["m"], c["Vbad"], c["f"], logA0, 3, alpha)
    assert [r_[10] for r_ in rec3] == [2, 1, 1] and all(r_[9] == 0 and r_[6] == 0 for r_ in rec3), rec3
    m1, V1, lm1, lv1, f1, rec1 = chain(gp, c, c["m"], c["Vbad"], c["f"], logA0, 1, alpha)
    assert rec1[0][10] == 2 and rec1[0][11] == 1.0 and same(rec1[0], rec3[0]), (rec1, rec3[0])
    fp = {"logA": torch.tensor(logA0, dtype=torch.float64)}
    mf, Vf = gp._estep_projected(c["r"], c["a"], c["aL"], c["L"], c["m"], fp, c["f"])
    em, ev = relerr(m1.cpu().numpy(), mf.cpu().numpy()), relerr(V1.cpu().numpy(), Vf.cpu().numpy())
    print(f"N {N} nb {nb}: fallback step against _estep_projected: relerr m {em:.2e} V {ev:.2e}; bits equal: m "
          f"{torch.equal(m1, mf)} V {torch.equal(V1, Vf)}")
    assert em <= TOL_UPDATE and ev <= TOL_UPDATE, (em, ev)
    assert bool(torch.isfinite(V1).all()) and torch.equal(V1, V1.T) and gp.cholesky(V1)[3] == 0
    two = chain(gp, c, m1, V1, f1, rec1[0][0], 2, alpha)
    assert [r_[10] for r_ in two[5]] == [1, 1]
    assert same_result((m3, V3, lm3, lv3, f3, rec3[1:]), two)
    # and against the restatement, whose first step is the full step too
    ref = restated(N, nb, alpha, True)
    m3r, V3r, *_ = chain(gp, c, c["m"], c["Vbad"], c["f"], float(c["np"]["logA"]), 3, alpha)
    em, ev = relerr(m3r.cpu().numpy(), ref[-1]["m"]), relerr(V3r.cpu().numpy(), ref[-1]["V"])
    print(f"N {N} nb {nb}: 3 steps from the indefinite V against the restatement: relerr m {em:.2e} V {ev:.2e}")
    assert [s["full"] for s in ref] == [True, False, False] and em < TOL_LOOP and ev < TOL_LOOP, (em, ev)
    # a non-finite rate: W1 fails whatever V is
    rng = np.random.default_rng(3)
    f0 = c["f"].clone()
    f0[7] = float("inf")
    lm0, lv0 = T(rng.standard_normal(N)), T(rng.random(N))
    for V0 in (c["Vbad"], c["V"]):
        m, V, lm, lv, f, rec = chain(gp, c, c["m"], V0, f0, logA0, 3, alpha, lambda_m=lm0, lambda_var=lv0)
        assert rec[0][9] != 0 and rec[0][10] == 0 and rec[0][:9] == [0.0] * 9, rec[0]
        assert rec[1] == [0.0] * 12 and rec[2] == [0.0] * 12, rec
        for x, y in ((m, c["m"]), (V, V0), (lm, lm0), (lv, lv0), (f, f0)):
            assert torch.equal(x, y)
        fp = {"logA": torch.tensor(0.25, dtype=torch.float64)}
        with pytest.raises(torch.linalg.LinAlgError, match=r"Estep: I \+ L\^T G L is not positive definite"):
            gp._estep_chain_damped_commit(rec, fp, 1, [0])


def test_three_units_of_different_size_one_falling_back(gp):
    """nb = 130, 200, 256 (all padded to 256) at N = 300, each with its own data; unit 1 carries the indefinite V.
    Every unit's arrays and records are those of the unit alone, bit for bit; a unit made to stop changes nothing in the
    others."""
    cs = [case(300, nb, seed=s) for s, nb in enumerate((130, 200, 256))]
    alpha = 0.5
    units = [unit(cs[0]), unit(cs[1], V=cs[1]["Vbad"]), unit(cs[2])]
    group = gp._estep_chain_damped_group(units, alpha, 3, NFP)
    assert [[r_[10] for r_ in g[5]] for g in group] == [[1, 1, 1], [2, 1, 1], [1, 1, 1]], [g[5] for g in group]
    alone = [chain(gp, c, c["m"], u["V"], c["f"], 0.1, 3, alpha) for c, u in zip(cs, units)]
    for i, (g, a) in enumerate(zip(group, alone)):
        assert same_result(g, a), i
        assert a[5][2][0] != 0.1
    f_inf = cs[0]["f"].clone()
    f_inf[5] = float("inf")
    stopped = gp._estep_chain_damped_group([unit(cs[0], f=f_inf)] + units[1:], alpha, 3, NFP)
    assert stopped[0][5][0][9] != 0 and stopped[0][5][0][10] == 0 and stopped[0][5][1] == [0.0] * 12
    assert torch.equal(stopped[0][0], cs[0]["m"]) and torch.equal(stopped[0][1], cs[0]["V"])
    for i in (1, 2):
        assert same_result(stopped[i], alone[i]), i


def test_sixteen_units(gp):
    """The largest group, 32 chains in the first recursion, at (64, 64) with each unit's own data; unit 11 carries the
    indefinite V.  Every unit against itself alone, bit for bit."""
    cs =[case(64, 64, seed=s) for s in range(16)]
    alpha = 0.05
    units = [unit(c, V=c["Vbad"] if i == 11 else None) for i, c in enumerate(cs)]
    group = gp._estep_chain_damped_group(units, alpha, 2, NFP)
    for i, (c, u, g) in enumerate(zip(cs, units, group)):
        assert [r_[10] for r_ in g[5]] == ([2, 1] if i == 11 else [1, 1]), (i, g[5])
        assert same_result(g, chain(gp, c, c["m"], u["V"], c["f"], 0.1, 2, alpha)), i


def test_raw_batch_refusals_write_nothing(gp):
    """Units of different alpha, or of different padded size, in one raw batch call: -3, nothing written."""
    c0, c1, c2 = case(300, 130, seed=0), case(300, 200, seed=1), case(300, 300, seed=0)
    engines = gp._group_engines(2, 300)

    def requests(ca, cb, alpha_b):
        return [gp._chain_damped_prepare(alpha=al, n_steps=2, n_fparam_steps=NFP, engine=e, **unit(c))
                for c, al, e in ((ca, 0.5, engines[0]), (cb, alpha_b, engines[1]))]

    for qs, why in ((requests(c0, c1, 0.05), "alpha"), (requests(c0, c2, 0.5), "differs from unit 0's")):
        before = [{k: q[k].clone() for k in ("m", "V", "f")} for q in qs]
        rec = (ctypes.c_double * (12 * 2 * 2))(*([-7.0] * 48))
        rc, _ = gp._chain_damped_batch_raw([e._ctx for e in engines], qs, rec=rec)
        assert rc == -3 and why in _lib.last_error() and "gpfit_estep_chain_damped_batch" in _lib.last_error()
        assert list(rec) == [-7.0] * 48
        torch.cuda.synchronize()
        for q, b in zip(qs, before):
            assert all(torch.equal(q[k], b[k]) for k in b)
        with pytest.raises(ValueError, match="share"):
            gp._request_run_group(qs)
    # and the same two sizes with one alpha run
    rc, _ = gp._chain_damped_batch_raw([e._ctx for e in engines], requests(c0, c1, 0.5))
    assert rc == 0


# ---- varGP with the switch
def run_vargp(gp, g, **extra_fit_parameters):
    N = int(g["N"])
    X, r = T(g["X"]), T(g["r"])
    ntilde = int(g["ntilde"]) if "ntilde" in g else N
    fit_parameters = {"ntilde": ntilde, "maxiter": int(g["maxiter"]), "nEstep": int(g["nEstep"]), "nMstep": int(g["nMstep"]),
                      "nFparamstep": int(g["nFparamstep"]), "kernfun": "acosker", "cellid": 0, "n_px_side": 8,
                      "display_hyper": False}
    fit_parameters.update(extra_fit_parameters)
    xtilde = X if ntilde == N else X[:ntilde].clone()
    theta = {k: torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for k, v in zip(KEYS, g["theta0"])}
    args = {"fit_parameters": fit_parameters, "xtilde": xtilde, "hyperparams_tuple": (theta, LOWER, UPPER),
            "f_params": {"logA": torch.tensor(syn.F_PARAMS["logA"], dtype=torch.float64),
                         "lambda0": torch.tensor(syn.F_PARAMS["lambda0"], dtype=torch.float64)}}
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fit, err = gp.varGP(X, r, **args)
    return fit, err, [str(w.message) for w in caught]


def spy(monkeypatch, gp, name, calls):
    inner = getattr(gp, name)

    def wrapper(*a, **kw):
        calls.append(name)
        return inner(*a, **kw)
    monkeypatch.setattr(gp, name, wrapper)


G6 = ["g6_vargp_sparse_N128_nt64.npz", "g6_vargp_full_N128.npz"]


@pytest.mark.parametrize("name", G6)
def test_whole_fits_with_the_damped_chain_on_and_off(gp, monkeypatch, name):
    """estep_alpha = 0.5 with the switch on against off (the host loop), within the project's whole-fit bounds
    (test_whole_fits_with_the_chain_on_and_off: tracks 1e-5; KL, theta, logA, m_b, V_b 1e-4) and with equal kept counts.
    On: every EM iteration issues exactly one _estep_chain_damped and no _estep_projected_damped; off: no chain call."""
    g = load_golden(name)
    monkeypatch.setattr(gp, "EIGVAL_TOL", float(g["tol"]))
    calls = []
    for fn in ("_estep_projected_damped", "_estep_chain_damped", "_estep_chain", "_estep_chain_full"):
        spy(monkeypatch, gp, fn, calls)
    runs = {}
    for on in (True, False):
        del calls[:]
        fit, err, _ = run_vargp(gp, g, estep_alpha=0.5, estep_damped_chain=on)
        assert not err["is_error"], err
        assert "_estep_chain" not in calls and "_estep_chain_full" not in calls
        if on:
            assert calls.count("_estep_chain_damped") == int(g["maxiter"]) - 1 and "_estep_projected_damped" not in calls, calls
        else:
            assert "_estep_chain_damped" not in calls and "_estep_projected_damped" in calls, calls
        runs[on] = fit
    # the module switch alone turns it on as well, and off is the default
    del calls[:]
    monkeypatch.setattr(gp, "DAMPED_CHAIN", True)
    fit_env, err, _ = run_vargp(gp, g, estep_alpha=0.5)
    assert not err["is_error"] and calls.count("_estep_chain_damped") == int(g["maxiter"]) - 1
    assert torch.equal(fit_env["m_b"], runs[True]["m_b"]) and torch.equal(fit_env["V_b"], runs[True]["V_b"])
    monkeypatch.setattr(gp, "DAMPED_CHAIN", False)
    del calls[:]
    fit_def, err, _ = run_vargp(gp, g, estep_alpha=0.5)
    assert not err["is_error"] and "_estep_chain_damped" not in calls
    assert torch.equal(fit_def["m_b"], runs[False]["m_b"]) and torch.equal(fit_def["V_b"], runs[False]["V_b"])

    def summary(fit):
        vt = fit["values_track"]
        return {"kept": [int(v.shape[0]) for v in vt["variation_par_track"]["V_b"]],
                "logmarginal": vt["loss_track"]["logmarginal"].numpy(), "KL": vt["loss_track"]["KL"].numpy(),
                "theta": np.array([float(fit["hyperparams_tuple"][0][k]) for k in KEYS]),
                "logA": float(fit["f_params"]["logA"])}
    on, off = summary(runs[True]), summary(runs[False])
    assert on["kept"] == off["kept"]
    assert runs[True]["estep_full_steps"] == runs[False]["estep_full_steps"]
    d = {"track": relerr(on["logmarginal"], off["logmarginal"]), "KL": relerr(on["KL"], off["KL"]),
         "theta": float(np.abs(on["theta"] - off["theta"]).max()), "logA": abs(on["logA"] - off["logA"]),
         "m_b": relerr(runs[True]["m_b"].cpu().numpy(), runs[False]["m_b"].cpu().numpy()),
         "V_b": relerr(runs[True]["V_b"].cpu().numpy(), runs[False]["V_b"].cpu().numpy())}
    print(f"{name}: damped chain on against off {d}; full steps {runs[True]['estep_full_steps']}")
    assert d["track"] < 1e-5 and d["KL"] < 1e-4 and d["theta"] < 1e-4 and d["logA"] < 1e-4, d
    assert d["m_b"] < 1e-4 and d["V_b"] < 1e-4, d


def test_vargp_counts_and_warns_for_a_full_step_of_the_chain(gp, monkeypatch):
    g = load_golden("g6_vargp_sparse_N128_nt64.npz")
    monkeypatch.setattr(gp, "EIGVAL_TOL", float(g["tol"]))
    inner = gp._estep_chain_damped
    flagged = []

    def once(*a, **kw):
        out = inner(*a, **kw)
        if not flagged:
            flagged.append(1)
            out[5][1][10] = 2.0
        return out
    monkeypatch.setattr(gp, "_estep_chain_damped", once)
    fit, err, caught = run_vargp(gp, g, estep_alpha=0.5, estep_damped_chain=True)
    assert not err["is_error"], err
    assert fit["estep_full_steps"] == 1
    texts = [w for w in caught if "full Newton step" in w]
    assert len(texts) == 1 and "in E-step 1 of iteration 1;" in texts[0], caught


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


def test_vargp_cells_groups_the_damped_chains_by_alpha(gp, monkeypatch):
    """Four damped cells on the stimuli of g6_vargp_sparse_N128_nt64, two step sizes with two cells each, the switch on:
    every (fit_model, err_dict) has the bits of its own varGP, and the chain calls went out two units at a time."""
    g = load_golden("g6_vargp_sparse_N128_nt64.npz")
    X, ntilde = T(g["X"]), int(g["ntilde"])
    rng = np.random.default_rng(17)
    rs = [T(g["r"])] + [T(rng.poisson(np.maximum(g["r"].mean(), 0.2), g["r"].shape).astype(np.float64)) for _ in range(3)]
    alphas = [0.5, 0.25, 0.5, 0.25]
    monkeypatch.setattr(gp, "EIGVAL_TOL", float(g["tol"]))

    def args(alpha):
        fit_parameters = {"ntilde": ntilde, "maxiter": int(g["maxiter"]), "nEstep": int(g["nEstep"]), "nMstep": int(g["nMstep"]),
                          "nFparamstep": int(g["nFparamstep"]), "kernfun": "acosker", "cellid": 0, "n_px_side": 8,
                          "display_hyper": False, "estep_alpha": alpha, "estep_damped_chain": True}
        theta = {k: torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for k, v in zip(KEYS, g["theta0"])}
        return {"fit_parameters": fit_parameters, "xtilde": X[:ntilde].clone(), "hyperparams_tuple": (theta, LOWER, UPPER),
                "f_params": {"logA": torch.tensor(syn.F_PARAMS["logA"], dtype=torch.float64),
                             "lambda0": torch.tensor(syn.F_PARAMS["lambda0"], dtype=torch.float64)}}
    kwargs = [args(al) for al in alphas]
    cells = in_a_thread(lambda: gp.varGP_cells(X, rs, copy.deepcopy(kwargs)))
    sizes = list(gp.varGP_cells.last_group_sizes)
    print(f"four damped cells, two step sizes: group sizes {sizes}")
    assert len(cells) == 4 and 2 in sizes and max(sizes) == 2 and sum(sizes) == 4 * (int(g["maxiter"]) - 1), sizes
    for i, r in enumerate(rs):
        (fit, err), (fit1, err1) = cells[i], in_a_thread(lambda: gp.varGP(X, r, **copy.deepcopy(kwargs[i])))
        assert not err["is_error"] and not err1["is_error"], (err, err1)
        for grp in ("loss_track", "theta_track", "f_par_track"):
            for k, v in fit["values_track"][grp].items():
                assert torch.equal(v, fit1["values_track"][grp][k]), (i, grp, k)
        for k in ("m_b", "V_b"):
            assert torch.equal(fit[k], fit1[k]), (i, k)
        assert fit["estep_full_steps"] == fit1["estep_full_steps"]
        for k in fit["f_params"]:
            assert torch.equal(fit["f_params"][k], fit1["f_params"][k]), (i, k)
