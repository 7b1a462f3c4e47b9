"""What a varGP_cells wave needs for its M-step closures to meet, without a GPU: the rendezvous with two kinds of request
(stub calls in place of the device calls), the closure bucket key, and the ctypes declaration of
gpfit_fit_eval_sparse_batch against the header's argument list.  Every thread is joined with a bound."""
import ctypes
import os
import re
import threading

from conftest import ROOT
from gaussian_processes_amd import _lib, utils as gp

JOIN_S = 30


def run_parties(bodies):
    """One thread per body; returns what each returned or raised."""
    out = [None] * len(bodies)

    def work(i):
        try:
            out[i] = ("ok", bodies[i]())
        except BaseException as err:
            out[i] = ("raised", err)
    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(len(bodies))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_S)
    assert not any(t.is_alive() for t in threads), "a party is still waiting"
    return out


class Stubs:
    """single / group that record (how, kinds, names) per call and answer (how, kind, name) per request."""

    def __init__(self, fail=None):
        self.calls, self.fail, self.lock = [], fail, threading.Lock()

    def single(self, q):
        with self.lock:
            self.calls.append(("single", {q["kind"]}, [q["name"]]))
        return ("single", q["kind"], q["name"])

    def group(self, qs):
        with self.lock:
            self.calls.append(("group", {q["kind"] for q in qs}, sorted(q["name"] for q in qs)))
        if self.fail is not None and all(q["kind"] == self.fail[0] for q in qs) and any(q["name"] in self.fail[1] for q in qs):
            raise RuntimeError("the closure group call failed")
        return [("group", q["kind"], q["name"]) for q in qs]


def key(q):
    return (q["kind"], q["bucket"])


def fit(rv, name, closures_per_mstep, bucket="A"):
    """A fit of len(closures_per_mstep) EM iterations: a chain, then that many closures (its line searches)."""
    def body():
        rv.enter()
        got = []
        try:
            for n_closures in closures_per_mstep:
                got.append(rv.call({"kind": "chain", "name": name, "bucket": bucket}))
                for _ in range(n_closures):
                    got.append(rv.call({"kind": "closure", "name": name, "bucket": bucket}))
            return got
        finally:
            rv.leave()
    return body


def test_fits_with_different_numbers_of_closures_between_two_chains():
    """x asks 3 closures per M-step, y 1, z 2: whenever all live fits wait, each kind goes out as its own call -- a closure
    never waits for the next EM iteration of a fit that is already at its chain -- and nothing deadlocks."""
    stubs = Stubs()
    rv = gp._ChainRendezvous(3, stubs.single, stubs.group, key)
    plan = {"x": [3, 3], "y": [1, 1], "z": [2, 2]}
    out = run_parties([fit(rv, n, p) for n, p in plan.items()])
    for (n, p), (how, res) in zip(plan.items(), out):
        assert how == "ok", res
        kinds = [k for _, k, _ in res]
        want = []
        for c in p:
            want += ["chain"] + ["closure"] * c
        assert kinds == want and all(name == n for _, _, name in res), (n, res)
    assert all(len(kinds) == 1 for _, kinds, _ in stubs.calls), stubs.calls          # kinds never share a call
    assert sum(rv.closure_group_sizes) == 2 * (3 + 1 + 2) and sum(rv.group_sizes) == 2 * 3
    # the first closure call carried all three fits; then y is at its next chain while x and z still search
    assert rv.closure_group_sizes[0] == 3 and 2 in rv.closure_group_sizes and 1 in rv.closure_group_sizes
    assert rv.group_sizes[0] == 3
    assert len(rv.closure_call_seconds) == len(rv.closure_group_sizes) and len(rv.call_seconds) == len(rv.group_sizes)
    assert rv.seconds_in_closure_call > 0.0 and rv.seconds_in_call > 0.0


def test_a_round_with_both_kinds_issues_one_call_per_kind():
    stubs = Stubs()
    rv = gp._ChainRendezvous(4, stubs.single, stubs.group, key)

    def once(name, kind):
        def body():
            rv.enter()
            try:
                return rv.call({"kind": kind, "name": name, "bucket": "A"})
            finally:
                rv.leave()
        return body
    out = run_parties([once("a", "closure"), once("b", "closure"), once("c", "chain"), once("d", "chain")])
    assert [res for _, res in out] == [("group", "closure", "a"), ("group", "closure", "b"), ("group", "chain", "c"),
                                       ("group", "chain", "d")]
    assert sorted(stubs.calls, key=lambda c: c[2]) == [("group", {"closure"}, ["a", "b"]), ("group", {"chain"}, ["c", "d"])]
    assert rv.closure_group_sizes == [2] and rv.group_sizes == [2]


def test_a_fit_that_leaves_releases_fits_waiting_with_either_kind():
    """w withdraws after the others have handed in a closure (x) and a chain (y): both calls go out when it leaves."""
    stubs = Stubs()
    rv = gp._ChainRendezvous(3, stubs.single, stubs.group, key)
    both_wait = threading.Event()

    def waiter(name, kind):
        def body():
            rv.enter()
            try:
                return rv.call({"kind": kind, "name": name, "bucket": "A"})
            finally:
                rv.leave()
        return body

    def leaver():
        rv.enter()
        try:
            while True:                      # its turn comes round only when the others wait or have not started
                with rv.cond:
                    if len(rv.waiting) == 2:
                        break
                rv.turn.release()
                both_wait.wait(0.001)
                rv.turn.acquire()
            return "left"
        finally:
            rv.leave()
    out = run_parties([waiter("x", "closure"), waiter("y", "chain"), leaver])
    assert out == [("ok", ("single", "closure", "x")), ("ok", ("single", "chain", "y")), ("ok", "left")]
    assert rv.closure_group_sizes == [1] and rv.group_sizes == [1]


def test_a_failing_closure_group_is_raised_in_its_participants_only():
    stubs = Stubs(fail=("closure", {"a1"}))
    rv = gp._ChainRendezvous(5, stubs.single, stubs.group, key)
    names = [("a0", "closure", "A"), ("a1", "closure", "A"), ("b0", "closure", "B"), ("c0", "chain", "A"), ("c1", "chain", "A")]

    def once(name, kind, bucket):
        def body():
            rv.enter()
            try:
                return rv.call({"kind": kind, "name": name, "bucket": bucket})
            finally:
                rv.leave()
        return body
    out = run_parties([once(*n) for n in names])
    for (n, kind, b), (how, res) in zip(names, out):
        if b == "A" and kind == "closure":
            assert how == "raised" and isinstance(res, RuntimeError) and "closure group call failed" in str(res), (n, res)
        else:
            assert how == "ok" and res == ("single" if n == "b0" else "group", kind, n), (n, res)
    assert sorted(rv.closure_group_sizes) == [1, 2] and rv.group_sizes == [2]


def test_requests_without_a_kind_are_counted_as_chain_calls():
    stubs_calls = []
    rv = gp._ChainRendezvous(1, lambda q: stubs_calls.append(q) or "one", lambda qs: ["g"] * len(qs), lambda q: 0)
    rv.enter()
    assert rv.call({"name": "plain"}) == "one"
    rv.leave()
    assert rv.group_sizes == [1] and rv.closure_group_sizes == []


def test_the_closure_bucket_key_is_what_a_group_call_shares():
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

    def q(N=200, Nt=120, n_kept=70, ldx=64, ldxt=64, rows=8, cols=8, stream=None, dev=0):
        return {"kind": "closure", "x": M(ldx, dev), "xt": M(ldxt, dev), "stream": Stream(stream), "N": N, "Nt": Nt,
                "n_kept": n_kept, "rows": rows, "cols": cols}
    k = gp._closure_bucket_key
    assert k(q(n_kept=70)) == k(q(n_kept=128)) == k(q(n_kept=101))          # one padded size
    assert k(q(n_kept=128)) != k(q(n_kept=129))
    assert k(q()) != k(q(N=201)) and k(q()) != k(q(Nt=121))
    assert k(q()) != k(q(ldx=72)) and k(q()) != k(q(ldxt=72))
    assert k(q()) != k(q(rows=4, cols=16))
    assert k(q()) != k(q(stream=5)) and k(q()) != k(q(dev=1))
    # the rendezvous' key carries the kind in front: a closure and a chain never share a bucket
    chain = {"kind": "chain", "a": M(70), "stream": Stream(), "N": 200, "nb": 70, "n_steps": 10, "nfp": 10, "lambda0_fixed": None}
    assert gp._request_bucket_key(q())[0] == "closure" and gp._request_bucket_key(chain)[0] == "chain"
    assert gp._request_bucket_key(q())[1:] == k(q()) and gp._request_bucket_key(chain)[1:] == gp._chain_bucket_key(chain)


def test_lib_declares_the_entry_with_the_headers_argument_list():
    hdr = open(os.path.join(ROOT, "include", "gpfit_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+gpfit_fit_eval_sparse_batch\s*\((.*?)\)\s*;", hdr, flags=re.S)
    assert m, "the header does not declare gpfit_fit_eval_sparse_batch"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    vp, i32, i64, pd = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_double)

    def ctype(p):
        decl = p.rsplit(" ", 1)[0].replace(" *", "*")
        return {"int": i32, "int64_t": i64, "void*": vp, "gpfit_ctx* const*": vp, "const double* const*": vp,
                "const int64_t*": vp, "const double*": pd, "double*": pd, "int*": ctypes.POINTER(i32)}[decl]
    res, args = _lib._SIGS["gpfit_fit_eval_sparse_batch"]
    assert res is i32
    assert len(args) == len(params) == 25, (len(args), params)
    for have, p in zip(args, params):
        assert have is ctype(p), (p, have)
    names = [p.rsplit(" ", 1)[1].lstrip("*") for p in params]
    assert names == ["ctxs", "n_units", "stream", "theta", "lower", "upper", "n_rows", "n_cols", "X", "ldx", "N", "Xtilde", "ldxt",
                     "Ntilde", "r", "B", "ldb", "n_kept", "m_b", "V_b", "ldvb", "logA", "lambda0", "out_host", "rc_out"]
    assert re.search(r"#define\s+GPFIT_FIT_EVAL_SPARSE_MAX_UNITS\s+16\b", hdr) and gp.MAX_CHAIN_UNITS == 16
