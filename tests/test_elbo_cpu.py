"""CPU-side checks of the fused loss (gpfit_elbo, gpfit_elbo_batch, utils.elbo_terms), no GPU:

* the numpy fp64 restatement the GPU tests compare against (elbo_cases.elbo_reference) agrees with the same arithmetic in
  np.longdouble to 1e-10 relative on every term and on KL over SHAPES x CONDS x V_KINDS, and so does the elementwise form
  of the trace, sum_ij V_ij K~^-1_ij, which is what the device call evaluates (measured when this test was written: the
  worst term is tr(V K~^-1) at cond 1e8 with 1.3e-11, the log-determinants reach 4.4e-12, KL and loglik <= 5e-16): the
  reference alone stays 75x inside the 1e-9 of the GPU tests;
* header, ctypes table and library agree on the two symbols, and both refuse a null argument, n_units = 0 and 17 and a
  leading dimension below nb with -3 under their own name before any context is read;
* the loss has a request kind of its own with its own book and a key of (N, padded nb)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import elbo_cases as cases
from conftest import ROOT
from gaussian_processes_amd import _lib
from gaussian_processes_amd.build import build_library

NAMES = ("gpfit_elbo", "gpfit_elbo_batch")
TOL_REFERENCE = 1e-10


@functools.lru_cache(maxsize=None)
def _both(N, nb, cond, v_kind):
    c = cases.make_elbo_case(N, nb, cond, v_kind)
    return (cases.elbo_reference(c), cases.elbo_reference(c, elementwise=True), cases.elbo_reference_longdouble(c),
            cases.elbo_reference_longdouble(c, elementwise=True))


@pytest.mark.parametrize("N,nb", cases.SHAPES)
def test_the_restatement_agrees_with_extended_precision(N, nb):
    worst = {}
    for cond in cases.CONDS:
        for v_kind in cases.V_KINDS:
            ref, ref_el, ext, ext_el = _both(N, nb, cond, v_kind)
            for what, got, want in (("product", ref, ext), ("elementwise", ref_el, ext_el), ("elementwise vs product", ref_el, ext)):
                err = np.abs((got.astype(np.longdouble) - want) / want).astype(np.float64)
                for slot, e in zip(cases.SLOTS, err):
                    worst[what, slot] = max(worst.get((what, slot), 0.0), float(e))
                assert err.max() < TOL_REFERENCE, (N, nb, cond, v_kind, what, dict(zip(cases.SLOTS, err)))
    print(f"N {N} nb {nb}: worst relative deviation per term " +
          ", ".join(f"{w} {s} {e:.1e}" for (w, s), e in sorted(worst.items()) if e > 1e-13))


@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _lib.load()


def test_symbols_are_declared_listed_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "gpfit_mi355x.h")).read()
    assert re.search(r"#define\s+GPFIT_ELBO_MAX_UNITS\s+16\b", hdr)
    assert "utils.py:1243" in hdr and "utils.py:1318-1326" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in the header"
        assert name in _lib.exported_symbols() and hasattr(lib, name)


def _fake():
    """A pointer to eight doubles that is no context and no device array: legal only where the checks answer first."""
    return ctypes.cast((ctypes.c_double * 8)(), ctypes.c_void_p)


SENTINEL = -7.25


def _single(lib, ctx=True, nb=100, N=200, ld=None, known=0, null=None, out=True, info=True):
    p = {k: _fake() for k in ("m", "V", "K", "Kinv", "r", "f", "lam_m")}
    if null:
        p[null] = None
    ld = {"ldv": nb, "ldk": nb, "ldki": nb, **(ld or {})}
    o, i = (ctypes.c_double * 10)(*[SENTINEL] * 10), (ctypes.c_int * 2)(-7, -7)
    rc = lib.gpfit_elbo(_fake() if ctx else None, None, p["m"], p["V"], ld["ldv"], p["K"], ld["ldk"], p["Kinv"], ld["ldki"], nb,
                        known, 0.0, p["r"], p["f"], p["lam_m"], N, 0.1, -0.3, o if out else None, i if info else None)
    assert list(o) == [SENTINEL] * 10 and list(i) == [-7, -7], "a refused call wrote its outputs"
    return rc, lib.gpfit_last_error().decode()


def _batch(lib, n_units=2, nb=100, N=200, ld=None, known=0, null=None, null_table=None, null_ctx=False):
    nu = max(n_units, 1)
    ctxs = (ctypes.c_void_p * nu)(*[_fake() for _ in range(nu)])
    if null_ctx:
        ctxs[nu - 1] = None
    t = {k: (ctypes.c_void_p * nu)(*[_fake() for _ in range(nu)]) for k in ("m", "V", "K", "Kinv", "r", "f", "lam_m")}
    if null:
        t[null][nu - 1] = None
    ld = {"ldv": nb, "ldk": nb, "ldki": nb, **(ld or {})}
    lds = {k: (ctypes.c_int64 * nu)(*([nb] * (nu - 1) + [v])) for k, v in ld.items()}
    if null_table:
        (t if null_table in t else lds)[null_table] = None
    o, i = (ctypes.c_double * (10 * nu))(*[SENTINEL] * (10 * nu)), (ctypes.c_int * (2 * nu))(*[-7] * (2 * nu))
    rc = lib.gpfit_elbo_batch(ctxs, n_units, None, t["m"], t["V"], lds["ldv"], t["K"], lds["ldk"], t["Kinv"], lds["ldki"],
                              (ctypes.c_int64 * nu)(*[nb] * nu), (ctypes.c_int * nu)(*[known] * nu), _lib.darr([0.0] * nu),
                              t["r"], t["f"], t["lam_m"], N, _lib.darr([0.1] * nu), _lib.darr([-0.3] * nu), o, i)
    assert list(o) == [SENTINEL] * (10 * nu) and list(i) == [-7] * (2 * nu), "a refused call wrote its outputs"
    return rc, lib.gpfit_last_error().decode()


def test_the_single_call_refuses_bad_arguments_before_the_context_is_read(lib):
    for kw in ([dict(ctx=False)] + [dict(null=k) for k in ("m", "V", "K", "Kinv", "r", "f", "lam_m")] +
               [dict(out=False), dict(info=False), dict(nb=0), dict(nb=-3), dict(N=0)] +
               [dict(ld={k: 99}) for k in ("ldv", "ldk", "ldki")]):
        rc, msg = _single(lib, **kw)
        assert rc == -3 and msg.startswith("gpfit_elbo: "), (kw, rc, msg)
    rc, msg = _single(lib, ld={"ldv": 99})
    assert "leading dimension" in msg
    rc, msg = _single(lib, null="K")
    assert "logdet_K_known" in msg


def test_the_batch_call_refuses_bad_arguments_before_any_context_is_read(lib):
    for n_units in (0, 17, -1):
        rc, msg = _batch(lib, n_units=n_units)
        assert rc == -3 and msg.startswith("gpfit_elbo_batch: ") and "16" in msg, (n_units, msg)
    for kw in ([dict(null_ctx=True)] + [dict(null=k) for k in ("m", "V", "K", "Kinv", "r", "f", "lam_m")] +
               [dict(null_table=k) for k in ("m", "V", "Kinv", "r", "f", "lam_m", "ldv", "ldki", "K", "ldk")] +
               [dict(nb=0), dict(N=0)] + [dict(ld={k: 99}) for k in ("ldv", "ldk", "ldki")]):
        rc, msg = _batch(lib, **kw)
        assert rc == -3 and msg.startswith("gpfit_elbo_batch: "), (kw, rc, msg)
    rc, msg = _batch(lib, ld={"ldki": 99})
    assert "unit 1: " in msg and "leading dimension" in msg      # the faulty unit is named


def test_the_loss_is_a_request_kind_with_its_own_book_and_key():
    from gaussian_processes_amd import utils as gp

    class Stream:
        value = None

    class M:
        class device:
            index = 0

    def request(N, nb):
        return {"kind": "loss", "stream": Stream(), "N": N, "nb": nb, "m": M()}
    kind = gp._request_kind(request(1000, 300))
    assert kind.kind == "loss" and kind.entry == "gpfit_elbo_batch" and kind.book == "loss_" and kind.switch is None
    assert all(callable(f) for f in (kind.run_single, kind.batch, kind.unit, kind.key)) and "share" in kind.share
    assert kind is gp._REQUEST_KINDS["loss", None]
    assert [k for k in gp._REQUEST_KINDS.values() if k.book == "loss_"] == [kind], "no other record's book is loss_"
    assert gp._ChainRendezvous._book(request(1000, 300)) == "loss_"
    rv = gp._ChainRendezvous(1, None, None, None)
    assert rv.loss_group_sizes == [] and rv.loss_call_seconds == [] and rv.seconds_in_loss_call == 0.0
    assert isinstance(gp.varGP_cells.last_loss_group_sizes, list) and isinstance(gp.varGP_cells.last_loss_call_seconds, list)
    assert isinstance(gp.varGP_cells.last_seconds_in_loss_call, float)
    # the key: the kind, where the call runs, then (N, padded nb) -- nb 257, 300 and 384 share a call, 385 does not
    keys = [gp._request_bucket_key(request(1000, nb)) for nb in (257, 300, 384, 385)]
    assert keys[0][0] == "loss" and keys[0][-2:] == (1000, 384) and keys[0] == keys[1] == keys[2]
    assert keys[3][-2:] == (1000, 512) and gp._request_bucket_key(request(999, 300))[-2:] == (999, 384)
    # no chain or closure request shares a key with it, and a mixed list is refused before any call
    with pytest.raises(ValueError, match="share"):
        gp._request_run_group([request(1000, 300), request(1000, 385)])


def test_the_switch_is_read_from_the_environment_once():
    from gaussian_processes_amd import utils as gp
    assert isinstance(gp.FUSED_LOSS, bool)
    assert gp.FUSED_LOSS == (os.environ.get("GPFIT_FUSED_LOSS", "1") != "0")
    assert callable(gp.elbo_terms)
