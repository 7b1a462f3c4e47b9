"""What a varGP_cells wave needs for its truncated-rank M-step closures to meet, without a GPU: the truncated request's
bucket key, the ctypes declaration of gpfit_fit_eval_projected_batch against the header's argument list, and the
rendezvous with truncated and sparse closure requests waiting together (stub calls in place of the device calls).  Every
thread is joined with a bound."""
import ctypes
import os
import re
import threading

from conftest import ROOT
from gaussian_processes_amd import _lib, utils as gp

JOIN_S = 30


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


class Engine:
    _ctx = 0


def trunc(N=200, n_kept=70, ldx=64, rows=8, cols=8, stream=None, dev=0, cap=256):
    return {"kind": "closure", "regime": "truncated", "x": M(ldx, dev), "stream": Stream(stream), "N": N, "n_kept": n_kept,
            "rows": rows, "cols": cols, "cap": cap}


def sparse(N=200, Nt=200, n_kept=70, ldx=64, ldxt=64, rows=8, cols=8, stream=None, dev=0):
    return {"kind": "closure", "x": M(ldx, dev), "xt": M(ldxt, dev), "stream": Stream(stream), "N": N, "Nt": Nt,
            "n_kept": n_kept, "rows": rows, "cols": cols}


def test_the_truncated_bucket_key_is_what_a_group_call_shares():
    k = gp._closure_bucket_key
    q = trunc
    assert k(q(n_kept=70)) == k(q(n_kept=128)) == k(q(n_kept=101))          # one padded size
    assert k(q(n_kept=128)) != k(q(n_kept=129))
    assert k(q()) != k(q(N=201))
    assert k(q()) != k(q(ldx=72))
    assert k(q()) != k(q(rows=4, cols=16))
    assert k(q()) != k(q(stream=5)) and k(q()) != k(q(dev=1))
    assert k(q()) != k(q(cap=1024))        # the slab counts and the lift's route depend on the workspace's capacity
    # the regime is in the key: a truncated and a sparse request with otherwise equal fields never share a call
    assert k(q()) != k(sparse()) and "truncated" in k(q()) and "truncated" not in k(sparse())
    assert gp._request_bucket_key(q())[0] == "closure" and gp._request_bucket_key(q())[1:] == k(q())
    # a request without the field keeps the sparse key, content for content
    s = sparse(Nt=120)
    assert k(s) == (0, None, 200, 120, 64, 64, 8, 8, 128)
    assert gp._request_bucket_key(s) == ("closure",) + k(s)


def test_lib_declares_the_entry_with_the_headers_argument_list():
    hdr = open(os.path.join(ROOT, "include", "gpfit_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+gpfit_fit_eval_projected_batch\s*\((.*?)\)\s*;", hdr, flags=re.S)
    assert m, "the header does not declare gpfit_fit_eval_projected_batch"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    vp, i32, i64, pd = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_double)

    def ctype(p):
        decl = p.rsplit(" ", 1)[0].replace(" *", "*")
        return {"int": i32, "int64_t": i64, "void*": vp, "gpfit_ctx* const*": vp, "const double* const*": vp,
                "const int64_t*": vp, "const double*": pd, "double*": pd, "int*": ctypes.POINTER(i32)}[decl]
    res, args = _lib._SIGS["gpfit_fit_eval_projected_batch"]
    assert res is i32
    assert len(args) == len(params) == 22, (len(args), params)
    for have, p in zip(args, params):
        assert have is ctype(p), (p, have)
    names = [p.rsplit(" ", 1)[1].lstrip("*") for p in params]
    assert names == ["ctxs", "n_units", "stream", "theta", "lower", "upper", "n_rows", "n_cols", "X", "ldx", "N", "r", "B", "ldb",
                     "n_kept", "m_b", "V_b", "ldvb", "logA", "lambda0", "out_host", "rc_out"]
    # the sparse entry's list without Xtilde / ldxt / Ntilde
    ms = re.search(r"\bint\s+gpfit_fit_eval_sparse_batch\s*\((.*?)\)\s*;", hdr, flags=re.S)
    sparse_params = [" ".join(p.split()) for p in ms.group(1).split(",")]
    assert params == [p for p in sparse_params if p.rsplit(" ", 1)[1].lstrip("*") not in ("Xtilde", "ldxt", "Ntilde")]
    assert re.search(r"#define\s+GPFIT_FIT_EVAL_PROJECTED_MAX_UNITS\s+16\b", hdr) and gp.MAX_CHAIN_UNITS == 16


def test_truncated_and_sparse_closures_waiting_together_go_out_as_separate_calls():
    """Two truncated and two sparse requests and one chain wait at a rendezvous keyed by _request_bucket_key: one call per
    regime, both counted as closure calls."""
    calls, lock = [], threading.Lock()

    def single(q):
        with lock:
            calls.append(("single", [q["name"]], {q.get("regime", "sparse") if q["kind"] == "closure" else "chain"}))
        return ("single", q["name"])

    def group(qs):
        with lock:
            calls.append(("group", sorted(q["name"] for q in qs), {q.get("regime", "sparse") for q in qs}))
        return [("group", q["name"]) for q in qs]
    chain = {"kind": "chain", "a": M(70), "stream": Stream(), "N": 200, "nb": 70, "n_steps": 10, "nfp": 10, "lambda0_fixed": None}
    reqs = [dict(trunc(n_kept=70), name="t0"), dict(trunc(n_kept=120), name="t1"), dict(sparse(n_kept=70), name="s0"),
            dict(sparse(n_kept=120), name="s1"), dict(chain, name="c0")]
    rv = gp._ChainRendezvous(len(reqs), single, group, gp._request_bucket_key)
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
    assert out == [("group", "t0"), ("group", "t1"), ("group", "s0"), ("group", "s1"), ("single", "c0")], out
    assert sorted(calls, key=lambda c: c[1]) == [("single", ["c0"], {"chain"}), ("group", ["s0", "s1"], {"sparse"}),
                                                 ("group", ["t0", "t1"], {"truncated"})], calls
    assert sorted(rv.closure_group_sizes) == [2, 2] and rv.group_sizes == [1]
    assert len(rv.closure_call_seconds) == 2


def test_the_dispatchers_send_a_request_to_its_regimes_call(monkeypatch):
    """_request_run_single / _request_run_group take the truncated kind's record for a request with that regime field; a
    mixed list is refused."""
    seen = []
    kind = gp._REQUEST_KINDS["closure", "truncated"]
    monkeypatch.setitem(gp._REQUEST_KINDS, ("closure", "truncated"), kind._replace(
        run_single=lambda q: seen.append(("single", q["name"])) or (0, [0.0] * 16),
        batch=lambda ctxs, qs: seen.append(("group", [q["name"] for q in qs])) or (0, [0.0] * 16 * len(qs), [0] * len(qs))))
    sparse_kind = gp._REQUEST_KINDS["closure", None]
    monkeypatch.setitem(gp._REQUEST_KINDS, ("closure", None), sparse_kind._replace(
        run_single=lambda q: seen.append(("sparse single", q["name"])), batch=lambda ctxs, qs: seen.append("sparse group")))
    t0, t1 = dict(trunc(), name="t0", engine=Engine()), dict(trunc(n_kept=100), name="t1", engine=Engine())
    assert gp._request_run_single(t0)[0] == 0 and len(gp._request_run_group([t0, t1])) == 2
    assert seen == [("single", "t0"), ("group", ["t0", "t1"])]
    try:
        gp._request_run_group([t0, dict(sparse(), name="s0", engine=Engine())])
    except ValueError as err:
        assert "share" in str(err)
    else:
        raise AssertionError("a call with both regimes was not refused")
    assert seen == [("single", "t0"), ("group", ["t0", "t1"])]
