"""The rendezvous of varGP_cells (utils._ChainRendezvous) without a GPU: stub chain functions in place of the device
calls.  Every thread is joined with a bound; a thread still alive afterwards fails the test."""
import threading

import pytest

from gaussian_processes_amd import utils as gp

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
    """single / group that record what they were asked and answer (tag, name) per request."""

    def __init__(self, fail_group=None):
        self.calls = []
        self.fail_group = fail_group
        self.lock = threading.Lock()

    def single(self, q):
        with self.lock:
            self.calls.append(("single", [q["name"]]))
        return ("single", q["name"])

    def group(self, qs):
        with self.lock:
            self.calls.append(("group", sorted(q["name"] for q in qs)))
        if self.fail_group is not None and any(q["name"] in self.fail_group for q in qs):
            raise RuntimeError("the group call failed")
        return [("group", q["name"]) for q in qs]


def key(q):
    return q["bucket"]


def party(rv, name, bucket, rounds=1):
    def body():
        rv.enter()
        try:
            return [rv.call({"name": name, "bucket": bucket}) for _ in range(rounds)]
        finally:
            rv.leave()
    return body


def test_two_buckets_and_a_singleton():
    stubs = Stubs()
    rv = gp._ChainRendezvous(6, stubs.single, stubs.group, key)
    names = [("a0", "A"), ("a1", "A"), ("a2", "A"), ("b0", "B"), ("b1", "B"), ("c0", "C")]
    out = run_parties([party(rv, n, b, rounds=2) for n, b in names])
    for (n, b), (how, res) in zip(names, out):
        assert how == "ok"
        assert res == [("single" if b == "C" else "group", n)] * 2
    per_round = [("group", ["a0", "a1", "a2"]), ("group", ["b0", "b1"]), ("single", ["c0"])]
    assert sorted(stubs.calls) == sorted(per_round * 2)
    assert sorted(rv.group_sizes) == [1, 1, 2, 2, 3, 3]


def test_a_bucket_larger_than_max_units_is_split():
    stubs = Stubs()
    rv = gp._ChainRendezvous(5, stubs.single, stubs.group, key, max_units=2)
    out = run_parties([party(rv, f"u{i}", "A") for i in range(5)])
    assert all(how == "ok" for how, _ in out)
    assert sorted(rv.group_sizes) == [1, 2, 2]


def test_a_party_that_leaves_early_is_not_waited_for():
    stubs = Stubs()
    rv = gp._ChainRendezvous(3, stubs.single, stubs.group, key)
    gone = threading.Event()

    def leaver():
        rv.enter()
        rv.leave()          # a fit that keeps its host loop: it never asks
        gone.set()
        return "left"

    def stayer(name):
        def body():
            gone.wait(JOIN_S)
            rv.enter()
            try:
                return [rv.call({"name": name, "bucket": "A"}) for _ in range(3)]
            finally:
                rv.leave()
        return body
    out = run_parties([leaver, stayer("x"), stayer("y")])
    assert out[0] == ("ok", "left")
    assert out[1] == ("ok", [("group", "x")] * 3) and out[2] == ("ok", [("group", "y")] * 3)
    assert rv.group_sizes == [2, 2, 2]


def test_a_party_that_ends_while_the_others_wait_releases_them():
    """y asks once and ends; x asks three times: its second and third requests go out alone, as single calls."""
    stubs = Stubs()
    rv = gp._ChainRendezvous(2, stubs.single, stubs.group, key)
    out = run_parties([party(rv, "x", "A", rounds=3), party(rv, "y", "A", rounds=1)])
    assert out[0] == ("ok", [("group", "x"), ("single", "x"), ("single", "x")])
    assert out[1] == ("ok", [("group", "y")])
    assert rv.group_sizes == [2, 1, 1]


def test_a_party_that_raises_is_not_waited_for():
    stubs = Stubs()
    rv = gp._ChainRendezvous(3, stubs.single, stubs.group, key)

    def raiser():
        rv.enter()
        try:
            rv.call({"name": "z", "bucket": "A"})
            raise ValueError("the fit failed between two chains")
        finally:
            rv.leave()
    out = run_parties([raiser, party(rv, "x", "A", rounds=2), party(rv, "y", "A", rounds=2)])
    assert out[0][0] == "raised" and isinstance(out[0][1], ValueError)
    assert out[1] == ("ok", [("group", "x")] * 2) and out[2] == ("ok", [("group", "y")] * 2)
    assert rv.group_sizes == [3, 2]


def test_a_failing_group_call_is_raised_in_every_participant_and_in_nobody_else():
    stubs = Stubs(fail_group={"a1"})
    rv = gp._ChainRendezvous(5, stubs.single, stubs.group, key)
    names = [("a0", "A"), ("a1", "A"), ("b0", "B"), ("b1", "B"), ("c0", "C")]
    out = run_parties([party(rv, n, b) for n, b in names])
    for (n, b), (how, res) in zip(names, out):
        if b == "A":
            assert how == "raised" and isinstance(res, RuntimeError) and "the group call failed" in str(res), (n, res)
        else:
            assert how == "ok" and res == [("single" if b == "C" else "group", n)], (n, res)
    assert sorted(rv.group_sizes) == [1, 2, 2]


def test_only_one_party_runs_between_two_calls():
    stubs = Stubs()
    rv = gp._ChainRendezvous(4, stubs.single, stubs.group, key)
    running, overlaps, lock = [0], [0], threading.Lock()

    def work():
        with lock:
            running[0] += 1
            overlaps[0] += running[0] > 1
        for _ in range(200):
            pass
        with lock:
            running[0] -= 1

    def turn_party(name, rounds, withdraws=False):
        def body():
            rv.enter()
            got = []
            try:
                if withdraws:
                    return "left"
                for _ in range(rounds):
                    work()
                    got.append(rv.call({"name": name, "bucket": "A"}))
                work()
                return got
            finally:
                rv.leave()
        return body
    out = run_parties([turn_party("x", 3), turn_party("y", 3), turn_party("z", 1), turn_party("w", 0, withdraws=True)])
    assert out[0] == ("ok", [("group", "x")] * 3) and out[1] == ("ok", [("group", "y")] * 3)
    assert out[2] == ("ok", [("group", "z")]) and out[3] == ("ok", "left")
    assert overlaps[0] == 0
    assert rv.group_sizes == [3, 2, 2]


def test_the_bucket_key_is_what_a_group_call_shares():
    class Stream:
        value = None

    class Dev:
        index = 0

    class A:
        device = Dev()

    def q(N, nb, n_steps=10, nfp=10, fixed=None):
        return {"a": A(), "stream": Stream(), "N": N, "nb": nb, "n_steps": n_steps, "nfp": nfp, "lambda0_fixed": fixed}
    k = gp._chain_bucket_key
    assert k(q(200, 70)) == k(q(200, 128)) == k(q(200, 101))          # one padded size
    assert k(q(200, 128)) != k(q(200, 129))
    assert k(q(200, 128)) != k(q(201, 128))
    assert k(q(200, 128)) != k(q(200, 128, n_steps=9)) and k(q(200, 128)) != k(q(200, 128, nfp=4))
    assert k(q(200, 128)) != k(q(200, 128, fixed=0.3)) and k(q(200, 128, fixed=0.5)) == k(q(200, 128, fixed=0.3))


def test_vargp_cells_checks_its_arguments_before_it_starts_a_thread():
    before = threading.active_count()
    with pytest.raises(ValueError, match="one kwargs dict per response vector"):
        gp.varGP_cells(None, [1, 2], [{}])
    with pytest.raises(ValueError, match="max_units"):
        gp.varGP_cells(None, [1], [{}], max_units=17)
    assert threading.active_count() == before
