"""CPU-side checks of the damped E-step (gpfit_estep_projected_damped, utils.Estep with alpha != 1): the library builds
with it; header, ctypes table and library agree on the symbol; every argument check answers before the context or an
operand is read; the numpy restatement of the reference's Estep reproduces the fixture the real reference wrote; the
Cholesky formulation the device call implements agrees with that restatement and keeps V positive definite; and Estep's
own refusals come before any device is needed.  No call reaches a GPU here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import estep_damped_cases as cases
from conftest import ROOT, load_golden, relerr
from gaussian_processes_amd import _lib
from gaussian_processes_amd.build import build_library

NAME = "gpfit_estep_projected_damped"


@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _lib.load()


def test_symbol_is_declared_listed_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "gpfit_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", hdr), "not declared in the header"
    assert NAME in _lib.exported_symbols()
    assert hasattr(lib, NAME)


_POINTERS = ("a", "aL", "L", "Linv", "V", "r", "m", "f", "m_new", "V_new")
_LDS = ("lda", "ldal", "ldl", "ldli", "ldv_in", "ldv")


def _call(lib, ctx, N=200, nb=130, alpha=0.5, **kw):
    """The call with dummy (host) pointers: legal only for arguments the checks refuse before anything is dereferenced.
    kw: a pointer's name -> False for NULL, a leading dimension's name -> its value (default nb)."""
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ptr = {k: (p if kw.get(k, True) else None) for k in _POINTERS}
    ld = {k: kw.get(k, nb) for k in _LDS}
    info_v = ctypes.c_int(-7)
    rc = lib.gpfit_estep_projected_damped(ctx, None, ptr["a"], ld["lda"], ptr["aL"], ld["ldal"], ptr["L"], ld["ldl"],
                                          ptr["Linv"], ld["ldli"], ptr["V"], ld["ldv_in"], N, nb, ptr["r"], ptr["m"],
                                          ptr["f"], 0.1, alpha, ptr["m_new"], ptr["V_new"], ld["ldv"],
                                          ctypes.byref(info_v))
    return rc, lib.gpfit_last_error().decode(), info_v.value


def _fake_ctx():
    # a context pointer that is not a context: the answer must come from the arguments alone
    return ctypes.cast((ctypes.c_double * 8)(), ctypes.c_void_p)


def test_null_context_is_refused(lib):
    rc, msg, info_v = _call(lib, None)
    assert rc == -3 and NAME in msg and info_v == -7


@pytest.mark.parametrize("alpha", [0.0, -0.5, 1.5, math.nan, math.inf])
def test_alpha_outside_0_1_is_refused_before_the_context_is_read(lib, alpha):
    rc, msg, info_v = _call(lib, _fake_ctx(), alpha=alpha)
    assert rc == -3 and NAME in msg and "alpha" in msg and info_v == -7


@pytest.mark.parametrize("name", _POINTERS)
def test_null_operand_is_refused_before_the_context_is_read(lib, name):
    rc, msg, _ = _call(lib, _fake_ctx(), **{name: False})
    assert rc == -3 and NAME in msg


@pytest.mark.parametrize("name", _LDS)
def test_short_leading_dimension_is_refused_before_the_context_is_read(lib, name):
    rc, msg, _ = _call(lib, _fake_ctx(), **{name: 129})
    assert rc == -3 and NAME in msg


@pytest.mark.parametrize("N,nb", [(0, 130), (-1, 130), (200, 0), (200, -3)])
def test_non_positive_sizes_are_refused_before_the_context_is_read(lib, N, nb):
    rc, msg, _ = _call(lib, _fake_ctx(), N=N, nb=nb)
    assert rc == -3 and NAME in msg


# ---- the arithmetic
def test_restatement_reproduces_the_reference_fixture():
    g = load_golden("g11_estep_damped.npz")
    assert list(g["alphas"]) == list(cases.ALPHAS)
    for i, alpha in enumerate(g["alphas"]):
        m_new, V_new = cases.reference_estep(g["r"], g["a"], g["m"], float(g["logA"]), g["f"], g["K"], g["V"], float(alpha))
        em, ev = relerr(m_new, g[f"m_new_{i}"]), relerr(V_new, g[f"V_new_{i}"])
        print(f"alpha {alpha}: relerr m {em:.2e} V {ev:.2e}")
        assert em < 1e-12 and ev < 1e-12


@pytest.mark.parametrize("N,nb", [(64, 64), (200, 130), (1000, 300)])
@pytest.mark.parametrize("cond", cases.CONDS)
def test_cholesky_formulation_agrees_with_the_restatement(N, nb, cond):
    for v_kind in cases.V_KINDS:
        c = cases.make_case(N, nb, cond, v_kind)
        args = (c["r"], c["a"], c["m"], c["logA"], c["f"], c["K"], c["V"])
        for alpha in cases.ALPHAS:
            m_ref, V_ref = cases.reference_estep(*args, alpha)
            m_new, V_new = cases.cholesky_estep(*args, alpha)
            em, ev = relerr(m_new, m_ref), relerr(V_new, V_ref)
            print(f"N {N} nb {nb} cond {cond:g} V {v_kind} alpha {alpha}: relerr m {em:.2e} V {ev:.2e}")
            assert em < 1e-9 and ev < 1e-9
            np.linalg.cholesky(V_new)             # raises unless positive definite
            # the mean the device call forms, (1 - a) m + a m_full, is the same vector
            m_full, _ = cases.reference_estep(*args[:6], None, 1.0)
            assert relerr((1 - alpha) * c["m"] + alpha * m_full, m_ref) < 1e-9


def test_alpha_one_of_the_formulation_is_the_full_step():
    c = cases.make_case(200, 130, 1e4, "newton")
    args = (c["r"], c["a"], c["m"], c["logA"], c["f"], c["K"], c["V"])
    m_ref, V_ref = cases.reference_estep(*args, 1.0)
    m_new, V_new = cases.cholesky_estep(*args, 1.0)
    assert relerr(m_new, m_ref) < 1e-9 and relerr(V_new, V_ref) < 1e-9


# ---- Estep's own checks come before any device is needed
def _estep_args():
    c = cases.make_case(64, 64, 1e2, "prior")
    t = {k: torch.tensor(v, dtype=torch.float64) for k, v in c.items() if k != "logA"}
    return (t["r"], t["a"], t["m"], {"logA": torch.tensor(c["logA"], dtype=torch.float64)}, t["f"]), t


def test_estep_refuses_a_step_size_outside_0_1():
    from gaussian_processes_amd import utils as gp
    args, t = _estep_args()
    for alpha in (2, 0, -0.5, math.nan):
        with pytest.raises(ValueError, match="alpha"):
            gp.Estep(*args, K_tilde=t["K"], V=t["V"], alpha=alpha)


def test_estep_unprovided_branches_stay_not_implemented():
    from gaussian_processes_amd import utils as gp
    args, t = _estep_args()
    with pytest.warns(UserWarning), pytest.raises(NotImplementedError):
        gp.Estep(*args, K_tilde=t["K"], V=t["V"], update_V_inv=True)
    with pytest.warns(UserWarning), pytest.raises(NotImplementedError):
        gp.Estep(*args, K_tilde=t["K"], alpha=0.5)                     # the damped update needs V
    with pytest.warns(UserWarning), pytest.raises(NotImplementedError):
        gp.Estep(*args, V=t["V"], alpha=0.5)                           # and K_tilde
