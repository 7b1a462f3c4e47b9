"""What a varGP_cells wave needs for its full-rank fits to meet, without a GPU: gpfit_estep_chain_full_batch is exported and
declared with the header's argument list, its argument refusals that need no device, the bucket keys of the full-rank chain
and closure requests, and the rendezvous with both kinds waiting together (stub calls in place of the device calls).  Every
thread is joined with a bound."""
import ctypes
import os
import re
import threading

from conftest import ROOT
from gaussian_processes_amd import _lib, utils as gp

JOIN_S = 30
NAME = "gpfit_estep_chain_full_batch"


class Stream:
    def __init__(self, value=None):
        self.value = value


class Dev:
    def __init__(self, index=0):
        self.index = index


class M:
    def __init__(self, ld, dev=0):
        self.device, self.ld = Dev(dev), ld

    def stride(self, i):
        return self.ld


def chain_full(N=200, n_steps=10, nfp=10, fixed=None, stream=None, dev=0):
    return {"kind": "chain_full", "K": M(N, dev), "stream": Stream(stream), "N": N, "n_steps": n_steps, "nfp": nfp,
            "lambda0_fixed": fixed}


def chain(N=200, nb=200, n_steps=10, nfp=10, fixed=None, stream=None, dev=0):
    return {"kind": "chain", "a": M(nb, dev), "stream": Stream(stream), "N": N, "nb": nb, "n_steps": n_steps, "nfp": nfp,
            "lambda0_fixed": fixed}


def closure_full(N=200, ldx=64, ldv=200, rows=8, cols=8, cap=256, reuse_V=False, stream=None, dev=0):
    return {"kind": "closure", "regime": "full", "x": M(ldx, dev), "V": M(ldv, dev), "stream": Stream(stream), "N": N,
            "rows": rows, "cols": cols, "cap": cap, "reuse_V": reuse_V}


def sparse(N=200, Nt=200, n_kept=70, ldx=64, ldxt=64, rows=8, cols=8, stream=None, dev=0):
    return {"kind": "closure", "x": M(ldx, dev), "xt": M(ldxt, dev), "stream": Stream(stream), "N": N, "Nt": Nt,
            "n_kept": n_kept, "rows": rows, "cols": cols}


# ---------------------------------------------------------------------------------------------- the library
def test_symbol_is_exported_and_bound():
    assert NAME in _lib.exported_symbols()
    fn = getattr(_lib.load(), NAME)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 24


def test_lib_declares_the_entry_with_the_headers_argument_list():
    hdr = open(os.path.join(ROOT, "include", "gpfit_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
    assert m, "the header does not declare " + NAME
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    vp, i32, i64, f64, pd = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.POINTER(ctypes.c_double)

    def ctype(p):
        decl = p.rsplit(" ", 1)[0].replace(" *", "*")
        return {"int": i32, "int64_t": i64, "double": f64, "void*": vp, "gpfit_ctx* const*": vp, "const double* const*": vp,
                "double* const*": vp, "const int64_t*": vp, "const double*": pd, "double*": pd}[decl]
    res, args = _lib._SIGS[NAME]
    assert res is i32
    assert len(args) == len(params) == 24, (len(args), params)
    for have, p in zip(args, params):
        assert have is ctype(p), (p, have)
    names = [p.rsplit(" ", 1)[1].lstrip("*") for p in params]
    assert names == ["ctxs", "n_units", "stream", "K", "ldk", "N", "r", "kv0", "m", "f", "V", "ldv", "lam_m", "lam_var", "logA0",
                     "lambda0_mode", "lambda0_fixed", "n_steps", "max_iter", "history_size", "lr", "tol_grad", "tol_change",
                     "rec_host"]
    # the projected group's list without a / aL / L, their leading dimensions and nb, with K / ldk in their place
    mp = re.search(r"\bint\s+gpfit_estep_chain_batch\s*\((.*?)\)\s*;", hdr, flags=re.S)
    proj = [" ".join(p.split()).rsplit(" ", 1)[1].lstrip("*") for p in mp.group(1).split(",")]
    gone = ("a", "lda", "aL", "ldal", "L", "ldl", "nb")
    assert [n for n in names if n not in ("K", "ldk")] == [n for n in proj if n not in gone]
    assert re.search(r"#define\s+GPFIT_ESTEP_CHAIN_FULL_MAX_UNITS\s+16\b", hdr) and gp.MAX_CHAIN_UNITS == 16


def call(n_units, n_steps, null=None):
    """The entry point with tables of null unit pointers: every case here has to be refused before any of them is read."""
    nu = max(n_units, 1)
    tab = (ctypes.c_void_p * nu)()
    ld = (ctypes.c_int64 * nu)(*[8] * nu)
    logA0 = (ctypes.c_double * nu)()
    rec = (ctypes.c_double * (12 * nu))()
    args = {"ctxs": tab, "K": tab, "ldk": ld, "r": tab, "kv0": tab, "m": tab, "f": tab, "V": tab, "ldv": ld, "lam_m": tab,
            "lam_var": tab, "logA0": logA0, "rec_host": rec}
    if null is not None:
        args[null] = None
    a = args
    return getattr(_lib.load(), NAME)(a["ctxs"], n_units, None, a["K"], a["ldk"], 8, a["r"], a["kv0"], a["m"], a["f"], a["V"],
                                      a["ldv"], a["lam_m"], a["lam_var"], a["logA0"], 0, None, n_steps, 4, 4, 0.1, 1e-7, 1e-9,
                                      a["rec_host"])


def test_unit_counts_outside_the_range_are_refused():
    for n in (0, 17):
        assert call(n, 1) == -3
        assert NAME + ":" in _lib.last_error() and "1 .. 16 units per call" in _lib.last_error()


def test_step_counts_outside_the_range_are_refused():
    for n in (0, 1025):
        assert call(2, n) == -3
        assert NAME + ":" in _lib.last_error() and f"n_steps {n} is not within 1 .. 1024" in _lib.last_error()
    assert call(2, 1024) == -3 and "bad argument" in _lib.last_error()      # the cap itself passes the n_steps check


def test_null_pointers_are_refused():
    for null in ("ctxs", "K", "ldk", "r", "kv0", "m", "f", "V", "ldv", "lam_m", "lam_var", "logA0", "rec_host"):
        assert call(2, 1, null) == -3, null
        assert _lib.last_error() == NAME + ": bad argument", (null, _lib.last_error())
    # every table is there, the units' own pointers are null: the message names the unit
    assert call(2, 1) == -3
    assert _lib.last_error() == NAME + ": unit 0: bad argument: null context or operand"
    # lambda0_mode = 1 reads lambda0_fixed
    nu = 2
    tab, ld = (ctypes.c_void_p * nu)(), (ctypes.c_int64 * nu)(8, 8)
    rc = getattr(_lib.load(), NAME)(tab, nu, None, tab, ld, 8, tab, tab, tab, tab, tab, ld, tab, tab, (ctypes.c_double * nu)(), 1,
                                    None, 1, 4, 4, 0.1, 1e-7, 1e-9, (ctypes.c_double * 24)())
    assert rc == -3 and _lib.last_error() == NAME + ": bad argument"


def test_the_single_call_is_refused_in_the_same_words():
    rec = (ctypes.c_double * 12)()
    rc = _lib.load().gpfit_estep_chain_full(None, None, None, 8, 8, None, None, None, None, None, 8, None, None, 0.0, 0, 0.0, 1,
                                            4, 4, 0.1, 1e-7, 1e-9, rec)
    assert rc == -3 and _lib.last_error() == "gpfit_estep_chain_full: bad argument: null context or operand"


# ---------------------------------------------------------------------------------------------- the bucket keys
def test_the_bucket_keys_are_what_a_group_call_shares():
    k = gp._request_bucket_key
    c = closure_full
    assert k(c()) == k(c()) and k(c(reuse_V=True)) == k(c(reuse_V=True))
    assert k(c(reuse_V=False)) != k(c(reuse_V=True))       # one flag per call: first closures of an M-step and later ones
    assert k(c()) != k(c(N=201))
    assert k(c()) != k(c(ldx=72)) and k(c()) != k(c(ldv=208)) and k(c()) != k(c(rows=4, cols=16))
    assert k(c()) != k(c(cap=1024)) and k(c()) != k(c(stream=5)) and k(c()) != k(c(dev=1))
    assert k(c())[:2] == ("closure", "full") and k(c())[1:] == gp._closure_bucket_key(c())
    assert k(c()) != k(sparse()) and "full" not in k(sparse())
    q = chain_full
    assert k(q()) == k(q()) == ("chain_full", 0, None, 200, 10, 10, False)
    assert k(q(fixed=0.3)) == k(q(fixed=0.5)) != k(q())
    assert k(q()) != k(q(N=201)) and k(q()) != k(q(n_steps=11)) and k(q()) != k(q(nfp=9))
    assert k(q()) != k(q(stream=5)) and k(q()) != k(q(dev=1))
    # a full-rank chain never shares a call with a projected one, whatever the sizes
    for N in (128, 200):
        assert k(q(N=N)) != k(chain(N=N, nb=N)) and k(chain(N=N, nb=N))[0] == "chain"


# ---------------------------------------------------------------------------------------------- the rendezvous
def wave(reqs, single, group, key=None):
    rv = gp._ChainRendezvous(len(reqs), single, group, key or gp._request_bucket_key)
    out = [None] * len(reqs)

    def party(i):
        rv.enter()
        try:
            out[i] = rv.call(reqs[i])
        except BaseException as err:
            out[i] = err
        finally:
            rv.leave()
    threads = [threading.Thread(target=party, args=(i,), daemon=True) for i in range(len(reqs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_S)
    assert not any(t.is_alive() for t in threads), "a party is still waiting"
    return rv, out


def test_full_rank_chains_and_closures_waiting_together_go_out_as_their_own_calls():
    """Two full-rank chains, three full-rank closures (two first ones of their M-step, one later), one sparse closure and
    one projected chain wait together: one call per kind and key, the full-rank ones counted in the new lists only."""
    calls, lock = [], threading.Lock()

    def single(q):
        with lock:
            calls.append(("single", [q["name"]]))
        return ("single", q["name"])

    def group(qs):
        with lock:
            calls.append(("group", sorted(q["name"] for q in qs)))
        return [("group", q["name"]) for q in qs]
    reqs = [dict(chain_full(), name="f0"), dict(chain_full(), name="f1"), dict(closure_full(), name="c0"),
            dict(closure_full(), name="c1"), dict(closure_full(reuse_V=True), name="c2"), dict(sparse(), name="s0"),
            dict(chain(nb=70), name="p0")]
    rv, out = wave(reqs, single, group)
    assert out == [("group", "f0"), ("group", "f1"), ("group", "c0"), ("group", "c1"), ("single", "c2"), ("single", "s0"),
                   ("single", "p0")], out
    assert sorted(calls, key=lambda c: c[1]) == [("group", ["c0", "c1"]), ("single", ["c2"]), ("group", ["f0", "f1"]),
                                                 ("single", ["p0"]), ("single", ["s0"])], calls
    assert rv.full_group_sizes == [2] and sorted(rv.full_closure_group_sizes) == [1, 2]
    assert rv.group_sizes == [1] and rv.closure_group_sizes == [1]
    assert len(rv.full_call_seconds) == 1 and len(rv.full_closure_call_seconds) == 2
    assert len(rv.call_seconds) == 1 and len(rv.closure_call_seconds) == 1
    assert rv.seconds_in_full_call > 0.0 and rv.seconds_in_full_closure_call > 0.0


def test_a_wave_of_full_rank_requests_leaves_the_other_counters_alone():
    reqs = [dict(chain_full(), name="f0"), dict(chain_full(), name="f1"), dict(closure_full(), name="c0")]
    rv, out = wave(reqs, lambda q: q["name"], lambda qs: [q["name"] for q in qs])
    assert out == ["f0", "f1", "c0"]
    assert rv.full_group_sizes == [2] and rv.full_closure_group_sizes == [1]
    assert rv.group_sizes == [] and rv.closure_group_sizes == [] and rv.call_seconds == [] and rv.closure_call_seconds == []
    assert rv.seconds_in_call == 0.0 and rv.seconds_in_closure_call == 0.0
    # and a request without a kind is counted where it was
    rv, out = wave([{"name": "x"}, {"name": "y"}], lambda q: q["name"], lambda qs: [q["name"] for q in qs], key=lambda q: 0)
    assert out == ["x", "y"] and rv.group_sizes == [2] and rv.full_group_sizes == [] and rv.full_closure_group_sizes == []


def test_a_failing_group_is_raised_in_its_participants_only():
    def group(qs):
        if qs[0]["kind"] == "chain_full":
            raise RuntimeError("the chain call failed")
        return [q["name"] for q in qs]
    reqs = [dict(chain_full(), name="f0"), dict(chain_full(), name="f1"), dict(closure_full(), name="c0"),
            dict(closure_full(), name="c1")]
    rv, out = wave(reqs, lambda q: q["name"], group)
    assert isinstance(out[0], RuntimeError) and isinstance(out[1], RuntimeError) and out[2:] == ["c0", "c1"], out
    assert rv.full_group_sizes == [2] and rv.full_closure_group_sizes == [2]
    # a unit's own exception in the group's result list is raised in that fit alone
    err = ValueError("unit 1 alone")
    rv, out = wave(reqs[2:], lambda q: q["name"], lambda qs: ["c0", err])
    assert out == ["c0", err]


def test_the_dispatchers_send_each_kind_to_its_own_call(monkeypatch):
    seen = []
    names = {("chain_full", None): "chain_full", ("closure", "full"): "closure_full", ("chain", None): "chain"}
    for key, name in names.items():
        monkeypatch.setitem(gp._REQUEST_KINDS, key, gp._REQUEST_KINDS[key]._replace(
            run_single=lambda q, name=name: seen.append((name + " single", q["name"])) or name + " single",
            batch=lambda ctxs, qs, name=name: seen.append((name + " group", [q["name"] for q in qs])) or (0, name + " group"),
            unit=lambda q, u, out: out))
    eng = type("Engine", (), {"_ctx": 0})()
    f0, f1 = dict(chain_full(), name="f0", engine=eng), dict(chain_full(), name="f1", engine=eng)
    c0, c1 = dict(closure_full(), name="c0", engine=eng), dict(closure_full(), name="c1", engine=eng)
    p0 = dict(chain(), name="p0", engine=eng)
    assert gp._request_run_single(f0) == "chain_full single" and gp._request_run_single(c0) == "closure_full single"
    assert gp._request_run_single(p0) == "chain single"
    assert gp._request_run_group([f0, f1]) == ["chain_full group"] * 2
    assert gp._request_run_group([c0, c1]) == ["closure_full group"] * 2
    assert gp._request_run_group([p0, p0]) == ["chain group"] * 2
    assert seen == [("chain_full single", "f0"), ("closure_full single", "c0"), ("chain single", "p0"),
                    ("chain_full group", ["f0", "f1"]), ("closure_full group", ["c0", "c1"]),
                    ("chain group", ["p0", "p0"])]
    try:
        gp._request_run_group([c0, dict(sparse(), name="s0", engine=eng)])
    except ValueError as err:
        assert "share" in str(err)
    else:
        raise AssertionError("a call with both regimes was not refused")
    assert len(seen) == 6


def test_the_switch_and_the_counters_exist():
    assert gp.FULL_RANK_GROUPS is True or os.environ.get("GPFIT_FULL_RANK_GROUPS") == "0"
    for name in ("last_full_group_sizes", "last_full_call_seconds", "last_full_closure_group_sizes",
                 "last_full_closure_call_seconds"):
        assert isinstance(getattr(gp.varGP_cells, name), list)
