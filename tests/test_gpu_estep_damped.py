"""The damped E-step on the GPU: gpfit_estep_projected_damped (through utils._estep_projected_damped) against the numpy
restatement of the reference's Estep (estep_damped_cases.reference_estep, pinned to the real reference by
g11_estep_damped.npz in test_estep_damped_cpu.py) and against that fixture itself; its failure reporting; Estep with
alpha != 1; and varGP with fit_parameters['estep_alpha'].

Shapes (N, nb): (64, 64) one 128-leaf per chain, no recursion; (130, 130) a orthogonal and N = nb (the full-rank use),
padded to 256 so both chains recurse in lock step; (200, 130) N no multiple of 32 or 128 (ragged row slices);
(1000, 300) padded to 384, an odd tile count with unequal halves.  The bound 1e-9 is that of the project's E-step tests
(the Cholesky formulation itself sits at 5e-13 of the restatement on these cases in fp64, test_estep_damped_cpu.py)."""
import contextlib
import ctypes
import functools
import io
import warnings

import numpy as np
import pytest
import torch

import estep_damped_cases as cases
from conftest import load_golden, relerr
from gaussian_processes_amd import synthetic as syn

pytestmark = pytest.mark.gpu
KEYS = syn.THETA_KEYS
LOWER, UPPER = syn.limits()
TOL = 1e-9


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


@pytest.fixture(scope="module")
def gp():
    from gaussian_processes_amd import utils
    return utils


@functools.lru_cache(maxsize=None)
def _case(N, nb, cond, v_kind):
    return cases.make_case(N, nb, cond, v_kind)


@functools.lru_cache(maxsize=None)
def _reference(N, nb, cond, v_kind, alpha):
    c = _case(N, nb, cond, v_kind)
    return cases.reference_estep(c["r"], c["a"], c["m"], c["logA"], c["f"], c["K"], c["V"], alpha)


def _fp(c):
    return {"logA": torch.tensor(float(c["logA"]), dtype=torch.float64)}


def _damped(gp, c, alpha, V=None, f=None):
    """The device call on the arrays of a case, with the factor of K~ from the library's own Cholesky."""
    K, a = T(c["K"]), T(c["a"])
    L, Linv, _, info = gp.cholesky(K, want_inverse=True)
    assert info == 0
    return gp._estep_projected_damped(T(c["r"]), a, gp.matmul(a, L), L, Linv, T(c["V"] if V is None else V), T(c["m"]),
                                      _fp(c), T(c["f"] if f is None else f), alpha)


def _check(gp, m_new, V_new, m_ref, V_ref, what):
    em, ev = relerr(m_new.cpu().numpy(), m_ref), relerr(V_new.cpu().numpy(), V_ref)
    print(f"{what}: relerr m {em:.2e} V {ev:.2e}")
    assert em < TOL, f"{what}: m_new deviates by {em:.2e}"
    assert ev < TOL, f"{what}: V_new deviates by {ev:.2e}"
    assert torch.equal(V_new, V_new.T), what
    assert gp.cholesky(V_new)[3] == 0, f"{what}: V_new has no Cholesky factor"


@pytest.mark.parametrize("N,nb", cases.SHAPES)
def test_damped_call_matches_the_restatement(gp, N, nb):
    todo = [(cond, v_kind, alpha) for cond in (1e2, 1e4) for v_kind in cases.V_KINDS for alpha in cases.ALPHAS]
    todo.append((1e8, "newton", 0.5))
    for cond, v_kind, alpha in todo:
        m_new, V_new = _damped(gp, _case(N, nb, cond, v_kind), alpha)
        m_ref, V_ref = _reference(N, nb, cond, v_kind, alpha)
        _check(gp, m_new, V_new, m_ref, V_ref, f"N {N} nb {nb} cond {cond:g} V {v_kind} alpha {alpha}")


def test_damped_call_matches_the_reference_fixture(gp):
    g = load_golden("g11_estep_damped.npz")
    c = {k: g[k] for k in ("r", "a", "m", "f", "K", "V")}
    c["logA"] = float(g["logA"])
    for i, alpha in enumerate(g["alphas"]):
        m_new, V_new = _damped(gp, c, float(alpha))
        _check(gp, m_new, V_new, g[f"m_new_{i}"], g[f"V_new_{i}"], f"g11 alpha {alpha}")


@pytest.mark.parametrize("N,nb", cases.SHAPES)
def test_alpha_one_is_the_full_step(gp, N, nb):
    c = _case(N, nb, 1e4, "newton")
    K, a = T(c["K"]), T(c["a"])
    L = gp.cholesky(K)[0]
    m_full, V_full = gp._estep_projected(T(c["r"]), a, gp.matmul(a, L), L, T(c["m"]), _fp(c), T(c["f"]))
    m_new, V_new = _damped(gp, c, 1.0)
    _check(gp, m_new, V_new, m_full.cpu().numpy(), V_full.cpu().numpy(), f"N {N} nb {nb} alpha 1 against the full step")


def test_failures_name_the_matrix(gp):
    from gaussian_processes_amd import _lib
    N, nb = 1000, 300
    c = _case(N, nb, 1e2, "prior")
    # V with one negative eigenvalue whose eigenvector lives in rows 256 .. 299 only (the last tile of the padded matrix)
    rng = np.random.default_rng(3)
    Q1, _ = np.linalg.qr(rng.standard_normal((256, 256)))
    Q2, _ = np.linalg.qr(rng.standard_normal((44, 44)))
    Q = np.zeros((nb, nb))
    Q[:256, :256], Q[256:, 256:] = Q1, Q2
    d = np.linspace(1.0, 3.0, nb)
    d[270] = -0.5
    V_bad = (Q * d) @ Q.T
    V_bad = (V_bad + V_bad.T) / 2
    with pytest.raises(torch.linalg.LinAlgError, match=r"^Estep: V is not positive definite"):
        _damped(gp, c, 0.5, V=V_bad)
    assert "V is not positive definite" in _lib.last_error() and "gpfit_estep_projected_damped" in _lib.last_error()
    # a NaN rate: W1 = I + L^T G L fails, V is fine
    f_bad = c["f"].copy()
    f_bad[17] = np.nan
    with pytest.raises(torch.linalg.LinAlgError, match=r"I \+ L\^T G L is not positive definite"):
        _damped(gp, c, 0.5, f=f_bad)
    assert "I + L^T G L" in _lib.last_error()
    # and the context is fine afterwards
    m_new, V_new = _damped(gp, c, 0.5)
    _check(gp, m_new, V_new, *_reference(N, nb, 1e2, "prior", 0.5), "after the failures")


def test_raw_return_codes_tell_the_two_failures_apart(gp):
    from gaussian_processes_amd import _lib
    N, nb = 200, 130
    c = _case(N, nb, 1e2, "prior")
    K, a = T(c["K"]), T(c["a"])
    L, Linv, _, _ = gp.cholesky(K, want_inverse=True)
    aL = gp.matmul(a, L)
    r, m = T(c["r"]), T(c["m"])
    m_new = torch.empty(nb, dtype=torch.float64, device="cuda")
    V_new = torch.empty((nb, nb), dtype=torch.float64, device="cuda")
    eng = gp.get_engine(max(N, nb), 1)

    def call(V, f, ctx=None):
        info_v = ctypes.c_int(-7)
        rc = _lib.load().gpfit_estep_projected_damped(
            eng._ctx if ctx is None else ctx, gp._stream(), a.data_ptr(), a.stride(0), aL.data_ptr(), aL.stride(0),
            L.data_ptr(), L.stride(0), Linv.data_ptr(), Linv.stride(0), V.data_ptr(), V.stride(0), N, nb, r.data_ptr(),
            m.data_ptr(), f.data_ptr(), c["logA"], 0.5, m_new.data_ptr(), V_new.data_ptr(), V_new.stride(0),
            ctypes.byref(info_v))
        return rc, info_v.value

    assert call(T(c["V"]), T(c["f"])) == (0, 0)
    rc, info_v = call(T(c["V"] - 60.0 * np.eye(nb)), T(c["f"]))         # every eigenvalue of V negative
    assert rc > 0 and info_v == rc
    f_bad = c["f"].copy()
    f_bad[3] = np.nan
    rc, info_v = call(T(c["V"]), T(f_bad))
    assert rc > 0 and info_v == 0
    # a context too small for the problem refuses
    from gaussian_processes_amd.engine import GPFitEngine
    small = GPFitEngine(128, 1)
    try:
        rc, info_v = call(T(c["V"]), T(c["f"]), ctx=small._ctx)
        assert rc == -3 and info_v == -7 and "capacity" in _lib.last_error()
    finally:
        small.close()


def test_estep_with_a_step_size(gp):
    c = _case(200, 130, 1e4, "newton")
    m_raw, V_raw = _damped(gp, c, 0.5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")             # the provided branch does not warn
        m_new, V_new = gp.Estep(T(c["r"]), T(c["a"]), T(c["m"]), _fp(c), T(c["f"]), K_tilde=T(c["K"]), V=T(c["V"]), alpha=0.5)
    assert torch.equal(m_new, m_raw) and torch.equal(V_new, V_raw)
    _check(gp, m_new, V_new, *_reference(200, 130, 1e4, "newton", 0.5), "Estep alpha 0.5")


# ---- varGP with fit_parameters['estep_alpha']
def _run_vargp(gp, g, **extra_fit_parameters):
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
    old = gp.EIGVAL_TOL
    gp.EIGVAL_TOL = float(g["tol"])
    try:
        with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fit, err = gp.varGP(X, r, **args)
    finally:
        gp.EIGVAL_TOL = old
    return fit, err, [str(w.message) for w in caught]


def _spy(monkeypatch, gp, name, calls):
    inner = getattr(gp, name)

    def wrapper(*a, **kw):
        calls.append(name)
        return inner(*a, **kw)
    monkeypatch.setattr(gp, name, wrapper)


G6 = ["g6_vargp_full_N128.npz", "g6_vargp_sparse_N128_nt64.npz"]


@pytest.mark.parametrize("name", G6)
def test_vargp_with_damped_esteps(gp, monkeypatch, name):
    g = load_golden(name)
    calls = []
    for fn in ("_estep_projected_damped", "_estep_chain", "_estep_chain_full"):
        _spy(monkeypatch, gp, fn, calls)
    fit, err, _ = _run_vargp(gp, g, estep_alpha=0.5)
    assert not err["is_error"], err
    track = fit["values_track"]["loss_track"]["logmarginal"]
    assert bool(torch.isfinite(track).all()), track
    assert gp.cholesky(fit["V_b"])[3] == 0
    assert isinstance(fit["estep_full_steps"], int) and fit["estep_full_steps"] >= 0
    print(f"{name}: {calls.count('_estep_projected_damped')} damped updates, {fit['estep_full_steps']} full steps, "
          f"final log-marginal {float(track[-1]):.6f}")
    assert "_estep_projected_damped" in calls
    assert "_estep_chain" not in calls and "_estep_chain_full" not in calls


@pytest.mark.parametrize("name", G6)
def test_vargp_with_alpha_one_given_is_the_default_fit(gp, name):
    g = load_golden(name)
    fit0, err0, _ = _run_vargp(gp, g)
    fit1, err1, _ = _run_vargp(gp, g, estep_alpha=1)
    assert not err0["is_error"] and not err1["is_error"]
    assert torch.equal(fit0["m_b"], fit1["m_b"]) and torch.equal(fit0["V_b"], fit1["V_b"])
    for k in ("logmarginal", "loglikelihood", "KL"):
        assert torch.equal(fit0["values_track"]["loss_track"][k], fit1["values_track"]["loss_track"][k]), k
    assert "estep_full_steps" not in fit0 and "estep_full_steps" not in fit1


def test_vargp_takes_the_full_step_when_v_is_not_positive_definite(gp, monkeypatch):
    g = load_golden("g6_vargp_sparse_N128_nt64.npz")
    inner = gp._estep_projected_damped
    raised = []

    def once(*a, **kw):
        if not raised:
            raised.append(1)
            raise torch.linalg.LinAlgError("Estep: V is not positive definite: the damped update needs a positive "
                                           "definite V (info=1)")
        return inner(*a, **kw)
    monkeypatch.setattr(gp, "_estep_projected_damped", once)
    fit, err, caught = _run_vargp(gp, g, estep_alpha=0.5)
    assert not err["is_error"], err
    assert fit["estep_full_steps"] == 1
    assert sum("full Newton step" in w for w in caught) == 1, caught
    assert gp.cholesky(fit["V_b"])[3] == 0
