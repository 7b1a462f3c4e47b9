"""The table of request kinds behind varGP_cells, without a GPU: its nine records, the bucket keys and books of hand-built
requests of every kind, the refusal of mixed lists before any call goes out (stub batch calls), and the unit bounds of the
*_group wrappers."""
import itertools

import pytest

from gaussian_processes_amd import utils as gp


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


class Engine:
    _ctx = 0
    n_max = 256


N = 200
BOOKS = {("chain", None): "", ("chain_full", None): "full_", ("chain_damped", None): "", ("closure", None): "closure_",
         ("closure", "truncated"): "closure_", ("closure", "full"): "full_closure_", ("loss", None): "loss_",
         ("sweeps", None): "basis_", ("sign", None): "basis_"}
ALL_BOOKS = ("", "closure_", "full_", "full_closure_", "loss_", "basis_")


def request(kind, regime):
    """A request of the kind with the fields its key reads: every field that two kinds share has one value."""
    q = {"kind": kind, "stream": Stream(), "engine": Engine(), "N": N, "n_steps": 10, "nfp": 10, "lambda0_fixed": None,
         "nb": N, "a": M(N), "K": M(N), "x": M(64), "xt": M(64), "V": M(N), "Nt": N, "n_kept": N, "rows": 8, "cols": 8,
         "cap": 256, "reuse_V": False, "alpha": 0.5, "k": 32, "flags": 2, "its0": 0, "c": [1.5, 1.2], "S": M(32), "m": M(N)}
    if regime is not None:
        q["regime"] = regime
    return q


REQUESTS = {key: request(*key) for key in BOOKS}


def test_the_table_has_exactly_the_nine_kinds_and_every_record_is_complete():
    assert set(gp._REQUEST_KINDS) == set(BOOKS) and len(gp._REQUEST_KINDS) == 9
    for key, kind in gp._REQUEST_KINDS.items():
        assert (kind.kind, kind.regime) == key and len(kind) == 10 and gp._request_kind(REQUESTS[key]) is kind
        assert kind.book in gp._ALL_BOOKS and kind.switch in (None, "FULL_RANK_GROUPS", "BASIS_GROUPS")
        assert kind.switch is None or isinstance(getattr(gp, kind.switch), bool)
        assert all(callable(f) for f in (kind.run_single, kind.batch, kind.unit, kind.key)), key
        assert kind.entry.startswith("gpfit_") and kind.entry.endswith("_batch") and "share" in kind.share, key
    assert len({kind.entry for kind in gp._REQUEST_KINDS.values()}) == 9
    switched = {name: {key for key, kind in gp._REQUEST_KINDS.items() if kind.switch == name}
                for name in ("FULL_RANK_GROUPS", "BASIS_GROUPS")}
    assert switched["FULL_RANK_GROUPS"] == {("chain_full", None), ("closure", "full")}
    assert switched["BASIS_GROUPS"] == {("sweeps", None), ("sign", None)}
    # a request with nothing but its kind is found too
    assert gp._request_kind({"kind": "sweeps"}) is gp._REQUEST_KINDS["sweeps", None]


def test_a_key_begins_with_the_kind_and_keys_of_different_kinds_differ():
    keys = {key: gp._request_bucket_key(q) for key, q in REQUESTS.items()}
    for (kind, regime), k in keys.items():
        assert k[0] == kind and k == gp._request_bucket_key(request(kind, regime))
        if kind == "closure":
            assert k[1:] == gp._closure_bucket_key(REQUESTS[kind, regime])
            assert (k[1] == regime) if regime else (k[1] not in ("truncated", "full"))
    assert len(set(keys.values())) == 9


def test_the_book_of_each_kind_and_of_a_request_without_one():
    assert gp._ALL_BOOKS == ALL_BOOKS
    assert {kind.book for kind in gp._REQUEST_KINDS.values()} == set(gp._ALL_BOOKS)
    for key, q in REQUESTS.items():
        assert gp._REQUEST_KINDS[key].book == BOOKS[key] == gp._ChainRendezvous._book(q)
    assert gp._ChainRendezvous._book({"name": "x"}) == "" and gp._ChainRendezvous._book("not a dict") == ""
    rv = gp._ChainRendezvous(1, None, None, None)
    for book in ALL_BOOKS:
        assert getattr(rv, book + "group_sizes") == [] and getattr(rv, book + "call_seconds") == []
        assert getattr(rv, "seconds_in_" + book + "call") == 0.0
        assert isinstance(getattr(gp.varGP_cells, "last_" + book + "group_sizes"), list)
        assert isinstance(getattr(gp.varGP_cells, "last_" + book + "call_seconds"), list)
        assert isinstance(getattr(gp.varGP_cells, "last_seconds_in_" + book + "call"), float)


def test_every_mixed_pair_is_refused_before_any_call(monkeypatch):
    called = []
    for key, kind in list(gp._REQUEST_KINDS.items()):
        monkeypatch.setitem(gp._REQUEST_KINDS, key, kind._replace(
            run_single=lambda q, key=key: called.append(("single", key)),
            batch=lambda ctxs, qs, key=key: called.append(("batch", key)) or (0, None),
            unit=lambda q, u, out, key=key: key))
    for a, b in itertools.permutations(REQUESTS, 2):
        with pytest.raises(ValueError, match="share") as err:
            gp._request_run_group([REQUESTS[a], REQUESTS[b]])
        assert gp._REQUEST_KINDS[a].entry in str(err.value)        # named after the kind actually called
    assert called == []
    # and two requests of one kind and bucket go to that kind's batch call, once
    for key in REQUESTS:
        assert gp._request_run_group([REQUESTS[key], request(*key)]) == [key, key]
    assert called == [("batch", key) for key in REQUESTS]


@pytest.mark.parametrize("name, extra", [("_estep_chain_group", (2, 10)), ("_estep_chain_full_group", (2, 10)),
                                         ("_closure_sparse_group", ()), ("_closure_projected_group", ())])
def test_the_group_wrappers_refuse_0_and_17_units_under_their_own_name(name, extra):
    for units in ([], [{}] * 17):
        with pytest.raises(ValueError, match=name + ": 1 .. 16 units per call"):
            getattr(gp, name)(units, *extra)
