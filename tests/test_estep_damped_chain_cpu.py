"""gpfit_estep_chain_damped / _batch without a GPU: the symbols are exported and bound, and the argument checks that need
no device answer -3 with a message before anything touches one; the request kind "chain_damped" and its bucket key; and
the numpy restatement of the n-step loop the call stands for (estep_damped_chain_cases.loop on
estep_damped_cases.cholesky_estep) against the same loop on the reference's own lines (reference_estep), to 1e-9 -- the
bound the project pins the formulation to (test_estep_damped_cpu.py, test_gpu_estep_damped.py)."""
import ctypes

import pytest

import estep_damped_cases as cases
import estep_damped_chain_cases as loops
from conftest import relerr
from gaussian_processes_amd import _lib, utils as gp

CAP = 1024   # GPFIT_ESTEP_CHAIN_MAX_STEPS of include/gpfit_mi355x.h
TOL = 1e-9


def call(ctx, n_steps, alpha=0.5):
    """The single entry point with null device pointers: every case here has to be refused before any of them is read."""
    rec = (ctypes.c_double * 12)()
    return _lib.load().gpfit_estep_chain_damped(ctx, None, None, 8, None, 8, None, 8, None, 8, 8, 8, None, None, None, None,
                                                None, 8, None, None, 0.0, alpha, 0, 0.0, n_steps, 4, 4, 0.1, 1e-7, 1e-9, rec)


def call_batch(n_units, n_steps, alpha=0.5):
    rec = (ctypes.c_double * (12 * 16))()
    return _lib.load().gpfit_estep_chain_damped_batch(None, n_units, None, None, None, None, None, None, None, None, None, 8,
                                                      None, None, None, None, None, None, None, None, None, None, alpha, 0,
                                                      None, n_steps, 4, 4, 0.1, 1e-7, 1e-9, rec)


def test_symbols_are_exported_and_bound():
    for name, nargs in (("gpfit_estep_chain_damped", 31), ("gpfit_estep_chain_damped_batch", 32)):
        assert name in _lib.exported_symbols()
        fn = getattr(_lib.load(), name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name


def test_null_context_is_refused():
    assert call(None, 1) == -3
    assert "gpfit_estep_chain_damped:" in _lib.last_error() and "bad argument" in _lib.last_error()
    assert call_batch(2, 1) == -3
    assert "gpfit_estep_chain_damped_batch:" in _lib.last_error() and "bad argument" in _lib.last_error()


def test_step_counts_outside_the_range_are_refused():
    assert call(None, 0) == -3 and "n_steps 0" in _lib.last_error()
    assert call(None, CAP + 1) == -3 and f"n_steps {CAP + 1}" in _lib.last_error()
    assert call(None, CAP) == -3 and "bad argument" in _lib.last_error()   # the cap itself passes the n_steps check
    assert call_batch(2, 0) == -3 and "n_steps 0" in _lib.last_error()
    assert call_batch(0, 1) == -3 and call_batch(17, 1) == -3 and "units per call" in _lib.last_error()


@pytest.mark.parametrize("alpha", [0.0, 1.5, float("nan"), -0.5, float("inf")])
def test_step_sizes_outside_the_range_are_refused(alpha):
    assert call(None, 1, alpha) == -3
    assert "gpfit_estep_chain_damped:" in _lib.last_error() and "alpha must lie in (0, 1]" in _lib.last_error()
    assert call_batch(2, 1, alpha) == -3
    assert "gpfit_estep_chain_damped_batch:" in _lib.last_error() and "alpha must lie in (0, 1]" in _lib.last_error()


# ---- the request kind
class Stream:
    value = None


class Dev:
    index = 0


class M:
    device = Dev()

    def __init__(self, ld):
        self.ld = ld

    def stride(self, i):
        return self.ld


def request(nb=200, alpha=0.5, kind="chain_damped"):
    return {"kind": kind, "stream": Stream(), "engine": None, "N": 300, "n_steps": 10, "nfp": 10, "lambda0_fixed": None,
            "nb": nb, "alpha": alpha, "a": M(nb), "V": M(nb)}


def test_the_request_kind_and_its_bucket_key():
    """The record is one of the table (tests/test_request_kinds_cpu.py pins the table as a whole) and is found by the
    lookup of every kind (_request_kind)."""
    kind = gp._request_kind(request())
    assert kind is gp._REQUEST_KINDS["chain_damped", None] and kind.kind == "chain_damped" and kind.regime is None
    assert kind.run_single is gp._chain_damped_run_single and kind.batch is gp._chain_damped_batch_raw
    assert kind.unit is gp._chain_result and kind.entry == "gpfit_estep_chain_damped_batch"
    assert kind.book == "" == gp._ChainRendezvous._book(request()) and kind.switch is None and "share" in kind.share
    key = gp._request_bucket_key
    assert key(request())[0] == "chain_damped"
    assert key(request())[1:] == gp._chain_bucket_key(request()) + (0.5,)        # the key of "chain" plus alpha
    assert key(request(alpha=0.5)) != key(request(alpha=0.05))                   # alpha alone separates
    assert key(request(nb=200)) != key(request(nb=300))                          # so does the padded size alone (256, 384)
    assert key(request(nb=130)) == key(request(nb=200))                          # 130 and 200 both pad to 256
    assert key(request()) != key(request(kind="chain"))                          # and never a call shared with "chain"
    # a mixed list is refused before any call goes out
    with pytest.raises(ValueError, match="gpfit_estep_chain_damped_batch.*share"):
        gp._request_run_group([request(alpha=0.5), request(alpha=0.05)])


def test_the_group_wrapper_refuses_0_and_17_units_under_its_own_name():
    for units in ([], [{}] * 17):
        with pytest.raises(ValueError, match="_estep_chain_damped_group: 1 .. 16 units per call"):
            gp._estep_chain_damped_group(units, 0.5, 2, 10)


def test_the_switch_is_off_by_default():
    import os
    if os.environ.get("GPFIT_DAMPED_CHAIN", "0") in ("", "0"):
        assert gp.DAMPED_CHAIN is False


def test_the_commit_warns_in_step_order_and_counts():
    import torch
    import warnings
    ok = [0.1, -1.0, 5.0, 4.0, 3.0, 2.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.1]
    full = ok[:10] + [2.0] + ok[11:]
    bad = [0.0] * 9 + [7.0, 0.0, 1.1]
    fp = {"logA": torch.tensor(0.0, dtype=torch.float64)}
    count = [0]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with pytest.raises(torch.linalg.LinAlgError, match=r"info=7"):
            gp._estep_chain_damped_commit([full, ok, full, bad, [0.0] * 12], fp, 4, count)
    texts = [str(w.message) for w in caught]
    assert count[0] == 2 and len(texts) == 2
    assert "E-step 0 of iteration 4" in texts[0] and "E-step 2 of iteration 4" in texts[1]
    assert all(t.startswith("varGP: V_b is not positive definite") and "full Newton step (alpha = 1)" in t for t in texts)
    assert float(fp["logA"]) == 0.1 and float(fp["lambda0"]) == -1.0


# ---- the restatement of the n-step loop
N, NB, ALPHA, STEPS, NFP = 200, 130, 0.5, 3, 10


@pytest.mark.parametrize("v_kind", ["given", "indefinite"])
def test_restated_loop_against_the_reference_lines(v_kind):
    c = cases.make_case(N, NB, 1e4, "newton")
    V0 = c["V"] if v_kind == "given" else loops.indefinite(c["V"])
    assert loops.is_posdef(V0) == (v_kind == "given")
    kv0 = loops.kv0_of(N)
    ours = loops.loop(c, kv0, ALPHA, STEPS, NFP, loops.cholesky_update, V=V0)
    ref = loops.loop(c, kv0, ALPHA, STEPS, NFP, loops.reference_update, V=V0)
    # the first update of the indefinite V is the full step (reference_estep at alpha = 1), every other one is damped
    assert [s["full"] for s in ours] == [s["full"] for s in ref] == [v_kind == "indefinite", False, False]
    assert ours[-1]["logA"] != c["logA"]                       # the optimiser moved: the steps really differ
    for k, (s, t) in enumerate(zip(ours, ref)):
        em, ev = relerr(s["m"], t["m"]), relerr(s["V"], t["V"])
        print(f"V {v_kind} step {k}: relerr m {em:.2e} V {ev:.2e} logA {s['logA']:.12f} / {t['logA']:.12f}")
        assert em < TOL and ev < TOL, (v_kind, k, em, ev)
        assert loops.is_posdef(s["V"])
