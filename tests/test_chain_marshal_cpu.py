"""The argument lists of the six E-step chain entry points (gpfit_estep_chain, _full, _damped and their _batch forms) as
utils builds them, without a GPU or the library: ``_lib.load`` is replaced by a stub that records what each entry point is
called with, and the recorded list is compared, position by position, with the parameter list of include/gpfit_mi355x.h
written out below.  Every tensor of a request has a pointer and a leading dimension of its own and every scalar a value of
its own, so an argument in the wrong place, or one field standing in for another, shows."""
import ctypes
import math

import pytest

from gaussian_processes_amd import _lib, utils as gp

LBFGS = {"lr": 0.1, "tol_grad": 1.e-7, "tol_change": 1.e-9}     # what a chain hands gpfit_fparam_lbfgs
N, N_STEPS, NFP = 300, 7, 9
NB = (200, 190)                                                  # both pad to 256
FIELDS = ("a", "aL", "L", "Linv", "K", "r", "kv0", "m", "f", "V", "lam_m", "lam_var")

# The parameters of include/gpfit_mi355x.h, in order.  (field, "ptr") / (field, "ld"): the device pointer / the leading
# dimension of that field of the request; in a batch call each is a table with one entry per unit, and so are nb, logA0
# and lambda0_fixed.
HEAD = {"chain": [("a", "ptr"), ("a", "ld"), ("aL", "ptr"), ("aL", "ld"), ("L", "ptr"), ("L", "ld"), "N", "nb"],
        "chain_full": [("K", "ptr"), ("K", "ld"), "N"],
        "chain_damped": [("a", "ptr"), ("a", "ld"), ("aL", "ptr"), ("aL", "ld"), ("L", "ptr"), ("L", "ld"), ("Linv", "ptr"),
                         ("Linv", "ld"), "N", "nb"]}
STATE = [("r", "ptr"), ("kv0", "ptr"), ("m", "ptr"), ("f", "ptr"), ("V", "ptr"), ("V", "ld"), ("lam_m", "ptr"),
         ("lam_var", "ptr"), "logA0"]
TAIL = ["lambda0_mode", "lambda0_fixed", "n_steps", "max_iter", "history_size", "lr", "tol_grad", "tol_change", "rec_host"]
PARAMS = {
    "gpfit_estep_chain": ["ctx", "stream"] + HEAD["chain"] + STATE + TAIL,
    "gpfit_estep_chain_full": ["ctx", "stream"] + HEAD["chain_full"] + STATE + TAIL,
    "gpfit_estep_chain_damped": ["ctx", "stream"] + HEAD["chain_damped"] + STATE + ["alpha"] + TAIL,
    "gpfit_estep_chain_batch": ["ctxs", "n_units", "stream"] + HEAD["chain"] + STATE + TAIL,
    "gpfit_estep_chain_full_batch": ["ctxs", "n_units", "stream"] + HEAD["chain_full"] + STATE + TAIL,
    "gpfit_estep_chain_damped_batch": ["ctxs", "n_units", "stream"] + HEAD["chain_damped"] + STATE + ["alpha"] + TAIL,
}
SINGLE = {"chain": "_chain_run_single", "chain_full": "_chain_full_run_single", "chain_damped": "_chain_damped_run_single"}
BATCH = {"chain": "_chain_batch_raw", "chain_full": "_chain_full_batch_raw", "chain_damped": "_chain_damped_batch_raw"}
ENTRY = {"chain": "gpfit_estep_chain", "chain_full": "gpfit_estep_chain_full", "chain_damped": "gpfit_estep_chain_damped"}
# the leading dimension that goes with a null pointer
DEFAULT_LD = {"chain": "nb", "chain_full": "N", "chain_damped": "nb"}


class Tensor:
    """What the marshal reads of a tensor: its pointer and its leading dimension."""

    def __init__(self, ptr, ld):
        self.ptr, self.ld = ptr, ld

    def data_ptr(self):
        return self.ptr

    def stride(self, i):
        assert i == 0
        return self.ld


class Engine:
    def __init__(self, u):
        self._ctx = ctypes.c_void_p(0x7000 + u)


def request(kind, u, lambda0_fixed=True, alpha=0.5):
    """Unit ``u`` of a call of ``kind``: a value of its own in every field (the fields of the other kinds included, so a
    marshal that reads a wrong one finds it)."""
    q = {"kind": kind, "engine": Engine(u), "stream": ctypes.c_void_p(0x5000), "N": N, "nb": NB[u], "alpha": alpha,
         "logA0": 0.25 + u, "lambda0_fixed": -1.5 - u if lambda0_fixed else None, "n_steps": N_STEPS, "nfp": NFP}
    for i, name in enumerate(FIELDS):
        q[name] = Tensor(0x100000 * (u + 1) + 0x100 * (i + 1), 1000 * (u + 1) + i)
    return q


class Library:
    """The six entry points: each checks its arguments against the declared signature, records them, numbers the
    records 0, 1, 2, ... and returns ``rc``."""

    def __init__(self, rc=0):
        self.rc, self.calls = rc, []
        for name in PARAMS:
            setattr(self, name, self._entry(name))

    def _entry(self, name):
        def entry(*args):
            argtypes = _lib._SIGS[name][1]
            assert len(args) == len(argtypes) == len(PARAMS[name]), name
            for i, (arg, argtype) in enumerate(zip(args, argtypes)):
                try:
                    argtype.from_param(arg)
                except (TypeError, ctypes.ArgumentError) as err:
                    raise AssertionError(f"{name}: argument {i} ({PARAMS[name][i]}) = {arg!r} is no {argtype}") from err
            self.calls.append((name, args))
            for i in range(len(args[-1])):
                args[-1][i] = float(i)
            return self.rc
        return entry

    def gpfit_last_error(self):
        return b"the stub's message"


@pytest.fixture
def lib(monkeypatch):
    stub = Library()
    monkeypatch.setattr(_lib, "load", lambda: stub)
    return stub


def plain(arg):
    """A recorded argument as Python values: a table as a list, a pointer as an integer or None."""
    if isinstance(arg, ctypes.Array):
        return list(arg)
    return arg.value if isinstance(arg, ctypes.c_void_p) else arg


def same(got, want):
    if isinstance(want, list):
        return isinstance(got, list) and len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    if isinstance(want, float) and math.isnan(want):
        return isinstance(got, float) and math.isnan(got)
    return type(got) is type(want) and got == want


def unit_value(kind, q, param):
    """What unit ``q`` contributes to ``param``."""
    if isinstance(param, tuple):
        field, what = param
        if what == "ptr":
            return None if q[field] is None else q[field].ptr
        override = {"K": "ldk", "V": "ldv"}[field] if kind == "chain_full" and field in ("K", "V") else None
        if override in q:
            return q[override]
        return q[DEFAULT_LD[kind]] if q[field] is None else q[field].ld
    if param == "lambda0_fixed":
        return q["lambda0_fixed"]
    return q[param]


def expected(kind, qs, batch, alpha=None):
    """The values the header's parameters take for the requests ``qs``, in order (rec_host apart)."""
    fixed = qs[0]["lambda0_fixed"] is not None
    want = []
    for param in PARAMS[ENTRY[kind] + ("_batch" if batch else "")][:-1]:
        if param == "ctx":
            want.append(qs[0]["engine"]._ctx.value)
        elif param == "ctxs":
            want.append([q["engine"]._ctx.value for q in qs])
        elif param == "n_units":
            want.append(len(qs))
        elif param == "stream":
            want.append(0x5000)
        elif param in ("N", "n_steps"):
            want.append(qs[0][param])
        elif param in ("max_iter", "history_size"):
            want.append(NFP)
        elif param in LBFGS:
            want.append(LBFGS[param])
        elif param == "lambda0_mode":
            want.append(1 if fixed else 0)
        elif param == "alpha":
            want.append(qs[0]["alpha"] if alpha is None else alpha)
        elif param == "lambda0_fixed":
            values = [q["lambda0_fixed"] if fixed else 0.0 for q in qs]
            want.append(values if batch else values[0])
        else:
            values = [unit_value(kind, q, param) for q in qs]
            want.append(values if batch else values[0])
    return want


def assert_call(lib, kind, qs, batch, rec=None, alpha=None):
    """The last recorded call is the kind's entry point with the header's arguments."""
    name, args = lib.calls[-1]
    assert name == ENTRY[kind] + ("_batch" if batch else "")
    want = expected(kind, qs, batch, alpha)
    for i, (arg, w) in enumerate(zip(args[:-1], want)):
        assert same(plain(arg), w), (name, i, PARAMS[name][i], plain(arg), w)
    assert len(args[-1]) == 12 * N_STEPS * len(qs) and (rec is None or args[-1] is rec)
    return args[-1]


def test_every_stub_field_is_distinct():
    qs = [request("chain_damped", u) for u in (0, 1)]
    ptrs = [q[f].ptr for q in qs for f in FIELDS]
    lds = [q[f].ld for q in qs for f in FIELDS]
    scalars = [N, N_STEPS, NFP, *NB] + [q[k] for q in qs for k in ("logA0", "lambda0_fixed")] + [0.5, *LBFGS.values()]
    assert len(set(ptrs)) == len(ptrs) and len(set(lds + scalars)) == len(lds + scalars)
    assert -(-NB[0] // 128) == -(-NB[1] // 128)


@pytest.mark.parametrize("kind", sorted(SINGLE))
@pytest.mark.parametrize("fixed", [True, False])
def test_the_single_call(lib, kind, fixed):
    q = request(kind, 1, lambda0_fixed=fixed)
    res = getattr(gp, SINGLE[kind])(q)
    assert len(lib.calls) == 1
    assert_call(lib, kind, [q], batch=False)
    # the request's state, and one 12-number record per step
    assert all(got is q[f] for got, f in zip(res[:5], ("m", "V", "lam_m", "lam_var", "f")))
    assert res[5] == [[float(12 * k + j) for j in range(12)] for k in range(N_STEPS)] and len(res) == 6


@pytest.mark.parametrize("kind", sorted(SINGLE))
def test_the_single_call_raises_under_its_own_name(lib, kind):
    lib.rc = -3
    with pytest.raises(_lib.GpfitError) as err:
        getattr(gp, SINGLE[kind])(request(kind, 0))
    assert str(err.value).startswith(ENTRY[kind] + " failed (rc=-3): the stub's message")
    assert lib.calls[-1][0] == ENTRY[kind]


@pytest.mark.parametrize("kind", sorted(BATCH))
@pytest.mark.parametrize("fixed", [True, False])
def test_the_batch_call(lib, kind, fixed):
    qs = [request(kind, u, lambda0_fixed=fixed) for u in (0, 1)]
    ctxs = [q["engine"]._ctx for q in qs]
    rc, rec = getattr(gp, BATCH[kind])(ctxs, qs)
    assert rc == 0 and len(lib.calls) == 1
    assert assert_call(lib, kind, qs, batch=True) is rec
    assert list(rec) == [float(i) for i in range(12 * N_STEPS * 2)]
    # contexts given as integers, the caller's array, a return code handed through unchecked; one unit is a batch too
    lib.rc, mine = -3, (ctypes.c_double * (12 * N_STEPS * 2))()
    rc, rec = getattr(gp, BATCH[kind])([c.value for c in ctxs], qs, mine)
    assert rc == -3 and rec is mine
    assert_call(lib, kind, qs, batch=True, rec=mine)
    rc, rec = getattr(gp, BATCH[kind])(ctxs[1:], qs[1:])
    assert_call(lib, kind, qs[1:], batch=True)
    # whether lambda0 is fixed is the first request's to say
    qs[1]["lambda0_fixed"] = -9.0
    getattr(gp, BATCH[kind])(ctxs, qs)
    assert_call(lib, kind, qs, batch=True)


@pytest.mark.parametrize("kind", sorted(BATCH))
def test_a_tensor_given_as_none_is_a_null_pointer_with_the_default_leading_dimension(lib, kind):
    qs = [request(kind, u) for u in (0, 1)]
    for field in HEAD[kind]:
        if isinstance(field, tuple):
            qs[1][field[0]] = None
    qs[1]["V"] = qs[0]["r"] = qs[1]["lam_var"] = None
    getattr(gp, BATCH[kind])([q["engine"]._ctx for q in qs], qs)
    assert_call(lib, kind, qs, batch=True)
    name, args = lib.calls[-1]
    lds = [plain(a)[1] for a, p in zip(args, PARAMS[name]) if isinstance(p, tuple) and p[1] == "ld"]
    assert lds and all(ld == (N if kind == "chain_full" else NB[1]) for ld in lds)


def test_ldk_and_ldv_replace_the_leading_dimensions_of_the_full_rank_batch(lib):
    qs = [request("chain_full", u) for u in (0, 1)]
    qs[0]["ldk"], qs[0]["ldv"] = 7777, 8888                 # beside a tensor: the override wins
    qs[1]["K"] = qs[1]["V"] = None
    qs[1]["ldv"] = 9999                                      # beside a null pointer too; K's falls back to N
    gp._chain_full_batch_raw([q["engine"]._ctx for q in qs], qs)
    assert_call(lib, "chain_full", qs, batch=True)
    name, args = lib.calls[-1]
    assert plain(args[PARAMS[name].index(("K", "ld"))]) == [7777, N]
    assert plain(args[PARAMS[name].index(("V", "ld"))]) == [8888, 9999]


def test_a_damped_batch_whose_units_disagree_on_alpha_has_none(lib):
    qs = [request("chain_damped", 0, alpha=0.5), request("chain_damped", 1, alpha=0.25)]
    gp._chain_damped_batch_raw([q["engine"]._ctx for q in qs], qs)
    assert_call(lib, "chain_damped", qs, batch=True, alpha=float("nan"))
    name, args = lib.calls[-1]
    assert math.isnan(args[PARAMS[name].index("alpha")])
    qs[1]["alpha"] = 0.5
    gp._chain_damped_batch_raw([q["engine"]._ctx for q in qs], qs)
    assert_call(lib, "chain_damped", qs, batch=True, alpha=0.5)
