"""The cases of the group pool-scoring tests (predict_group_cases) and the host logic of ``score_pool_cells``, checked on
the CPU.

Cases: every K~_b is well conditioned, every reference variance positive, and each unit's re-associated form (numpy
fp64) agrees with its long-double moments to 1e-12, as test_predict_cases_cpu.py asks of the single cases; the units
fall into the buckets the case list states.

Host logic, with the device calls replaced by recording stand-ins (the pattern of test_sign_chain_cpu.py /
test_request_kinds_cpu.py): the cells are sorted into buckets and cut into calls of at most ``max_units``, the results
come back in the caller's order, the switch sends every cell through the single call, an exception stays with its cell."""
import numpy as np
import pytest
import torch

import predict_cases as cases
import predict_group_cases as groups
from gaussian_processes_amd import utils as gp

GROUP_IDS = [g[0] for g in groups.GROUPS]


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("group", groups.GROUPS, ids=GROUP_IDS)
def test_units_are_sound_and_their_forms_agree(group):
    name, P, shapes = group
    for c, (mu_ref, s2_ref), (nt, k, kept) in zip(groups.make_group(group), groups.group_reference(group), shapes):
        assert c["xstar"].shape == (P, 64) and c["xtilde"].shape == (nt, 64) and c["K"].shape == (k, k)
        assert c["C"].shape == (kept, kept) and int(c["mask"].sum()) == kept == c["d"]
        assert all(r.stop - r.start != nt for r in groups.reference_rows(c))
        cond = np.linalg.cond(c["K"])
        mu, s2 = groups.moments_reassociated(c)
        e = (cases.err(mu, mu_ref), cases.err(s2, s2_ref))
        print(f"{name} {(nt, k, kept)}: cond(K~_b) = {cond:.2e}, sigma2_ref in [{float(s2_ref.min()):.3f}, "
              f"{float(s2_ref.max()):.3f}], re-associated vs long double mu {e[0]:.2e} sigma2 {e[1]:.2e}")
        assert cond <= 1e5
        assert mu_ref.shape == (P,) and np.all(s2_ref > 0)
        assert np.linalg.eigvalsh(c["V"]).min() > 0
        if c["B"] is not None:
            assert np.max(np.abs(c["B"].T @ c["B"] - np.eye(k))) <= 1e-13
        else:
            assert k == nt
        assert e[0] <= 1e-12 and e[1] <= 1e-12


@pytest.mark.parametrize("group", groups.GROUPS, ids=GROUP_IDS)
def test_buckets_are_what_the_case_list_says(group):
    units = groups.make_group(group)
    assert [groups.bucket(c) for c in units] == groups.BUCKETS[group[0]]
    assert [gp._pool_bucket_key(c["d"], c["nt"], c["k"], c["B"] is not None) for c in units] == groups.BUCKETS[group[0]]
    assert all(c["P"] == group[1] for c in units)


def test_units_of_a_group_differ_where_the_call_has_tables():
    units = groups.make_group(groups.PROJECTED3)
    assert len({c["theta"]["sigma_0"] for c in units}) == 3 and len({c["logA"] for c in units}) == 3
    assert len({c["lambda0"] for c in units}) == 3 and len({c["d"] for c in units}) == 3
    assert len({(c["nt"], c["k"]) for c in units}) == 3
    assert all(c["xstar"] is units[0]["xstar"] for c in units)          # one pool


# ------------------------------------------------------------------ score_pool_cells with the device calls replaced
def cells_of(group):
    """The cells of a group as score_pool_cells takes them (host tensors: nothing here reaches a device); a cell is told
    from the others by its lambda0."""
    out = []
    for c in groups.make_group(group):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
        folded = {"S": torch.zeros(c["k"], c["k"]), "w": torch.zeros(c["k"]), "B": None if c["B"] is None else t(c["B"]),
                  "k": c["k"]}
        out.append({"xtilde": t(c["xtilde"][:, c["mask"]]), "C": t(c["C"]), "theta": c["theta"], "folded": folded,
                    "f_params": {"logA": torch.tensor(c["logA"]), "lambda0": torch.tensor(c["lambda0"])}, "mask": t(c["mask"])})
    return out


class Recorder:
    """Stand-ins for the two device calls of score_pool_cells and for the sum: every row a call writes is filled with the
    unit's lambda0 (utility: ten times that), and the calls are recorded."""

    def __init__(self, monkeypatch, fail=None):
        self.calls, self.fail = [], fail
        monkeypatch.setattr(gp, "_device", lambda: torch.device("cpu"))
        monkeypatch.setattr(gp, "_score_pool_group", self.group)
        monkeypatch.setattr(gp, "_score_pool_single", self.single)
        monkeypatch.setattr(gp, "_utility_sum", self.total)

    def write(self, unit, rows):
        lam = float(unit["f_params"]["lambda0"])
        if self.fail is not None and lam == self.fail:
            raise RuntimeError(f"cell with lambda0 {lam} cannot be scored")
        for row in rows[:3]:
            row.fill_(lam)
        if rows[3] is not None:
            rows[3].fill_(10 * lam)

    def group(self, units, r_masked, chunk_rows, out=None):
        self.calls.append(("group", [float(u["f_params"]["lambda0"]) for u in units], chunk_rows))
        assert len({gp._pool_cell_key(u) for u in units}) == 1 and all(u["xstar"] is units[0]["xstar"] for u in units)
        for u, rows in zip(units, out):
            self.write(u, rows)

    def single(self, unit, r_masked, chunk_rows, out):
        self.calls.append(("single", [float(unit["f_params"]["lambda0"])], chunk_rows))
        self.write(unit, out)

    def total(self, U, weights=None):
        self.calls.append(("sum", tuple(U.shape), weights))
        return U.sum(0)


COUNTS = torch.arange(0, 100, dtype=torch.float64)


def test_buckets_calls_and_the_callers_order(monkeypatch):
    rec = Recorder(monkeypatch)
    cells = cells_of(groups.MIXED)
    lam = [float(c["f_params"]["lambda0"]) for c in cells]
    order = [3, 0, 4, 1, 2]                     # the caller's order mixes the buckets
    xstar = torch.from_numpy(np.array(groups.pool(130)))
    out = gp.score_pool_cells(xstar, [cells[i] for i in order], r_masked=COUNTS, chunk_rows=128)
    assert gp.last_pool_group_sizes == [1, 3, 1]          # buckets in the order of their first cell
    assert [c[1] for c in rec.calls[:3]] == [[lam[3]], [lam[0], lam[1], lam[2]], [lam[4]]]
    assert all(c[0] == "group" and c[2] == 128 for c in rec.calls[:3]) and rec.calls[3][:2] == ("sum", (5, 130))
    for key in ("mu", "sigma2", "rate"):
        assert out[key].shape == (5, 130)
        assert torch.equal(out[key][:, 0], torch.tensor([lam[i] for i in order], dtype=torch.float64))
    assert torch.equal(out["utility"][:, 7], torch.tensor([10 * lam[i] for i in order], dtype=torch.float64))
    assert out["population_utility"].shape == (130,) and out["errors"] == [None] * 5


def test_mixed_in_its_own_order_is_three_one_one(monkeypatch):
    Recorder(monkeypatch)
    xstar = torch.from_numpy(np.array(groups.pool(130)))
    out = gp.score_pool_cells(xstar, cells_of(groups.MIXED))
    assert gp.last_pool_group_sizes == [3, 1, 1]
    assert out["utility"] is None and out["population_utility"] is None


def test_max_units_cuts_a_bucket(monkeypatch):
    rec = Recorder(monkeypatch)
    xstar = torch.from_numpy(np.array(groups.pool(130)))
    gp.score_pool_cells(xstar, cells_of(groups.PROJECTED3), max_units=2)
    assert gp.last_pool_group_sizes == [2, 1] and [len(c[1]) for c in rec.calls] == [2, 1]
    gp.score_pool_cells(xstar, cells_of(groups.SIXTEEN) + cells_of(groups.SIXTEEN)[:3])
    assert gp.last_pool_group_sizes == [16, 3]
    with pytest.raises(ValueError):
        gp.score_pool_cells(xstar, cells_of(groups.PROJECTED3), max_units=17)
    with pytest.raises(ValueError):
        gp.score_pool_cells(xstar, cells_of(groups.PROJECTED3), chunk_rows=100)


def test_the_switch_routes_every_cell_to_the_single_call(monkeypatch):
    rec = Recorder(monkeypatch)
    monkeypatch.setattr(gp, "POOL_GROUPS", False)
    xstar = torch.from_numpy(np.array(groups.pool(130)))
    cells = cells_of(groups.MIXED)
    out = gp.score_pool_cells(xstar, cells, r_masked=COUNTS)
    assert gp.last_pool_group_sizes == [1] * 5
    assert [c[0] for c in rec.calls] == ["single"] * 5 + ["sum"]
    assert torch.equal(out["mu"][:, 3], torch.tensor([float(c["f_params"]["lambda0"]) for c in cells], dtype=torch.float64))


@pytest.mark.parametrize("grouped", [True, False], ids=["groups", "single"])
def test_an_exception_stays_with_its_cell(monkeypatch, grouped):
    cells = cells_of(groups.MIXED)
    lam = [float(c["f_params"]["lambda0"]) for c in cells]
    rec = Recorder(monkeypatch, fail=lam[1])               # a member of the bucket of three
    monkeypatch.setattr(gp, "POOL_GROUPS", grouped)
    xstar = torch.from_numpy(np.array(groups.pool(130)))
    out = gp.score_pool_cells(xstar, cells, r_masked=COUNTS)
    assert [e is None for e in out["errors"]] == [True, False, True, True, True]
    assert isinstance(out["errors"][1], RuntimeError) and "cannot be scored" in str(out["errors"][1])
    assert bool(torch.isnan(out["mu"][1]).all()) and bool(torch.isnan(out["utility"][1]).all())
    for i in (0, 2, 3, 4):
        assert bool((out["mu"][i] == lam[i]).all()) and bool((out["utility"][i] == 10 * lam[i]).all())
    assert sum(gp.last_pool_group_sizes) == 4              # the calls that scored a cell
    assert rec.calls[-1][0] == "sum"


def test_group_refuses_bad_lists_before_any_call(monkeypatch):
    monkeypatch.setattr(gp, "_device", lambda: torch.device("cpu"))
    called = []
    monkeypatch.setattr(gp, "_score_pool_batch_raw", lambda *a, **k: called.append("batch"))
    monkeypatch.setattr(gp, "_group_engines", lambda *a, **k: called.append("engines"))
    xstar = torch.from_numpy(np.array(groups.pool(130)))
    units = [dict(c, xstar=xstar) for c in cells_of(groups.MIXED)]
    with pytest.raises(ValueError, match="1 .. 16 units"):
        gp._score_pool_group([], COUNTS, 0)
    with pytest.raises(ValueError, match="1 .. 16 units"):
        gp._score_pool_group(units[:1] * 17, COUNTS, 0)
    with pytest.raises(ValueError, match="chunk_rows"):
        gp._score_pool_group(units[:3], COUNTS, 100)
    with pytest.raises(ValueError, match="share"):
        gp._score_pool_group(units[:4], COUNTS, 0)          # a projected and an identity unit
    with pytest.raises(ValueError, match="share"):
        gp._score_pool_group([units[0], dict(units[1], xstar=xstar[:100])], COUNTS, 0)
    assert called == []
