"""Greedy selection on the device (gpfit_select_batch through utils.select_batch / select_round, and the C call itself)
against the long-double recurrence of select_cases.greedy_reference.

The device, the numpy fp64 transcription and the reference all start from the same fp64 covariance and means
(select_cases.*_inputs), so what is compared is the selection alone.  Equal picks may be demanded because every step of
every case separates its pick from the runner-up by a relative gap of at least 1e-6 (test_select_cases_cpu.py; the exact
copy of the duplicate pool is the one deliberate tie, decided by the lowest index).  The conditional variances may err at
most ten times as much as the fp64 transcription (both against long double, relative to the largest initial variance,
floored at 1e-15): the same recurrence, another summation order.

Shapes: 130 rows with 8 picks (identity basis and projected), 300 rows with 128 picks (the sum over earlier picks then
runs to the end of one 128-thread stride), 5 rows with 8 picks (exhaustion), 3 and 16 units."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import predict_cases as cases
import predict_group_cases as groups
import select_cases as sel

pytestmark = pytest.mark.gpu
LD = np.longdouble
SENTINEL = -777


def T(a):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()      # a copy: shared inputs are read-only


def bits(t):
    return t.detach().cpu().numpy().view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def gp():
    from gaussian_processes_amd import utils
    return utils


@pytest.fixture(scope="module")
def lib():
    from gaussian_processes_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def counts():
    return torch.from_numpy(sel.COUNTS).cuda()


def link(A):
    """A = 1 exactly (logA = 0) through the host module; other gains go through the C call, which takes A itself."""
    assert A == 1.0
    return {"logA": torch.tensor(0.0, dtype=torch.float64), "lambda0": torch.tensor(sel.LAMBDA0, dtype=torch.float64)}


def raw(lib, Sigmas, mus, As, weights, counts, n_select, fill=0.0, n_units=None):
    """gpfit_select_batch itself: (rc, picked, utility, sigma2 [n][M], work [n][n_select][M]); work starts as ``fill``,
    picked as the sentinel."""
    n = len(Sigmas)
    M = Sigmas[0].shape[0]
    rows = max(1, min(n_select, 128))
    work = torch.full((n, rows, M), fill, dtype=torch.float64, device="cuda")
    s2 = torch.full((n, M), float(SENTINEL), dtype=torch.float64, device="cuda")
    picked = torch.full((rows,), SENTINEL, dtype=torch.int32, device="cuda")
    utility = torch.full((rows,), float(SENTINEL), dtype=torch.float64, device="cuda")
    ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])   # noqa: E731
    darr = lambda v: (ctypes.c_double * n)(*[float(x) for x in v])         # noqa: E731
    rc = lib.gpfit_select_batch(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), n if n_units is None else n_units,
                                ptrs(Sigmas), (ctypes.c_int64 * n)(*[S.stride(0) for S in Sigmas]), M, ptrs(mus), darr(As),
                                darr([sel.LAMBDA0] * n), None if weights is None else darr(weights), counts.data_ptr(),
                                counts.numel(), n_select, ptrs(list(work)), ptrs(list(s2)), picked.data_ptr(), utility.data_ptr())
    torch.cuda.synchronize()
    return rc, picked, utility, s2, work


def variance_error(s2, ref_s2, Sigma):
    return float(np.max(np.abs(np.asarray(s2, dtype=LD) - ref_s2)) / np.max(np.diag(Sigma)))


# ------------------------------------------------------------------ 1. one pick is the argmax of today's score
@functools.lru_cache(maxsize=None)
def _unit(shape):
    from gaussian_processes_amd import utils as gp
    c = cases.make_case(*shape)
    mask = torch.from_numpy(c["mask"]).cuda()
    u = {k: T(c[k]) for k in ("C", "K", "Kinv", "m", "V")}
    u["xs"], u["xt"] = T(c["xstar"])[:, mask].contiguous(), T(c["xtilde"])[:, mask].contiguous()
    B = gp._mark_identity(torch.eye(c["nt"], dtype=torch.float64, device="cuda")) if c["B"] is None else T(c["B"])
    u["theta"] = c["theta"]
    u["folded"] = gp.fold_posterior(u["K"], u["Kinv"], u["m"], u["V"], B)
    return u


@pytest.mark.parametrize("shape", [cases.CASES[1], cases.PROJECTED], ids=lambda s: "P{}-nt{}-k{}-px{}".format(*s))
def test_one_pick_is_the_argmax_of_score_pool(gp, counts, shape):
    u = _unit(shape)
    args = (u["xs"], u["xt"], u["C"], u["theta"], u["folded"])
    score = gp.score_pool(*args, link(1.0), r_masked=counts)
    Sigma = gp.pool_covariance(*args)
    out = gp.select_batch([Sigma], [score["mu"]], [link(1.0)], counts, 1)
    best = int(score["utility"].argmax())
    assert out["picked"].dtype == torch.int64 and out["picked"].tolist() == [best]
    assert same_bits(out["utility"], score["utility"][best:best + 1])


# ------------------------------------------------------------------ 2. picks and conditional variances
@pytest.mark.parametrize("name", sorted(sel.SINGLE))
def test_picks_and_conditional_variances_follow_the_reference(lib, counts, name):
    _, A, n_select = sel.SINGLE[name]
    Sigma, mu = sel.single_inputs(name)
    ref = sel.single_reference(name)
    f64 = sel.greedy_f64([Sigma], [mu], [A], [sel.LAMBDA0], None, n_select)
    rc, picked, utility, s2, _ = raw(lib, [T(Sigma)], [T(mu)], [A], None, counts, n_select)
    assert rc == 0
    e_dev = variance_error(s2[0].cpu().numpy(), ref["sigma2"][0], Sigma)
    e_f64 = variance_error(f64["sigma2"][0], ref["sigma2"][0], Sigma)
    e_u = float(np.max(np.abs(utility.cpu().numpy() - np.array(ref["utility"])) / np.abs(np.array(ref["utility"]))))
    print(f"\n{name}: sigma2_cond e_dev {e_dev:.2e} e_f64 {e_f64:.2e}; utility of the picks, relative {e_u:.2e}; "
          f"smallest gap {min(ref['gap']):.2e}")
    assert picked.tolist() == ref["picked"]
    assert e_dev <= 10 * max(e_f64, 1e-15)


# ------------------------------------------------------------------ 3. duplicates
def test_a_copy_and_a_near_copy_take_one_slot_each(gp, lib, counts):
    Sigma, mu = sel.duplicate_inputs()
    ref = sel.duplicate_reference()
    rc, picked, _, _, _ = raw(lib, [T(Sigma)], [T(mu)], [1.0], None, counts, 8)
    picked = picked.tolist()
    assert rc == 0 and picked == ref["picked"]
    assert picked[0] == 20 and 21 not in picked                    # the exact copy ties; the lowest index wins
    assert (46 in picked) + (47 in picked) == 1                    # the near-copy pair yields one pick
    # the top 8 of the same scores hold both pairs: what the examples pick without --batch-aware
    U = gp.nd_utility(T(np.diag(Sigma).copy()), T(mu) + sel.LAMBDA0, counts)
    top = torch.topk(U, 8).indices.tolist()
    print(f"\ntop-8 {sorted(top)} greedy {picked}")
    assert {20, 21, 46, 47} <= set(top)


def test_the_tie_of_an_exact_copy_survives_the_device_covariance(gp, counts):
    """End to end on the duplicate pool: identical rows get identical bits from gpfit_pool_covariance and from
    gpfit_score_pool, so the copy ties on the device too and pool order decides."""
    c = sel.duplicate_case()
    u = _unit(sel.DUPLICATE_SHAPE)
    xs = T(c["xstar"])[:, torch.from_numpy(c["mask"]).cuda()].contiguous()
    cell = {"xtilde": u["xt"], "C": u["C"], "theta": u["theta"], "folded": u["folded"], "f_params": link(1.0)}
    out = gp.select_round(xs, [cell], 8, counts)
    assert out["picked"].tolist() == sel.duplicate_reference()["picked"]
    util = out["scores"]["population_utility"]
    assert same_bits(util[20:21], util[21:22])


# ------------------------------------------------------------------ 4. exhaustion and rows without a finite utility
def test_exhaustion_is_decided_on_the_device(lib, counts):
    Sigma, mu = sel.single_inputs("identity130")
    S5, m5 = np.ascontiguousarray(Sigma[:5, :5]), mu[:5]
    ref = sel.greedy_reference([S5], [m5], [1.0], [sel.LAMBDA0], None, 8)
    rc, picked, utility, s2, _ = raw(lib, [T(S5)], [T(m5)], [1.0], None, counts, 8)
    assert rc == 0 and picked.tolist() == ref["picked"] and picked.tolist()[5:] == [-1, -1, -1]
    u = utility.cpu().numpy()
    assert np.all(np.isfinite(u[:5])) and np.all(np.isnan(u[5:]))
    # conditioned on all five, then left alone
    f64 = sel.greedy_f64([S5], [m5], [1.0], [sel.LAMBDA0], None, 8)
    e_f64 = variance_error(f64["sigma2"][0], ref["sigma2"][0], S5)
    assert variance_error(s2[0].cpu().numpy(), ref["sigma2"][0], S5) <= 10 * max(e_f64, 1e-15)


def test_a_row_without_a_finite_utility_is_never_picked(lib, counts):
    Sigma, mu = sel.single_inputs("identity130")
    dead = np.array(Sigma[:40, :40])
    dead[7, :] = 0.0
    dead[:, 7] = 0.0
    ref = sel.greedy_reference([dead], [mu[:40]], [1.0], [sel.LAMBDA0], None, 8)
    rc, picked, utility, s2, _ = raw(lib, [T(dead)], [T(mu[:40])], [1.0], None, counts, 8)
    assert rc == 0 and 7 not in picked.tolist() and picked.tolist() == ref["picked"]
    assert bool(torch.isfinite(utility).all()) and float(s2[0][7]) == 0.0
    # nothing finite at all: -1 from the first step on, the call ends clean
    rc, picked, utility, _, _ = raw(lib, [torch.zeros(6, 6, dtype=torch.float64, device="cuda")], [T(mu[:6])], [1.0], None, counts, 3)
    assert rc == 0 and picked.tolist() == [-1, -1, -1] and bool(torch.isnan(utility).all())


# ------------------------------------------------------------------ 5. several units with weights
@pytest.mark.parametrize("name", sorted(sel.UNITS))
def test_units_with_weights_follow_the_reference(lib, counts, name):
    _, weights, n_select = sel.UNITS[name]
    inp = sel.unit_inputs(name)
    n = len(inp)
    As = [sel.unit_A(u) for u in range(n)]
    ref = sel.unit_reference(name)
    f64 = sel.greedy_f64([S for S, _ in inp], [m for _, m in inp], As, [sel.LAMBDA0] * n, weights, n_select)
    rc, picked, _, s2, _ = raw(lib, [T(S) for S, _ in inp], [T(m) for _, m in inp], As, weights, counts, n_select)
    assert rc == 0 and picked.tolist() == ref["picked"]
    e_dev = max(variance_error(s2[u].cpu().numpy(), ref["sigma2"][u], inp[u][0]) for u in range(n))
    e_f64 = max(variance_error(f64["sigma2"][u], ref["sigma2"][u], inp[u][0]) for u in range(n))
    print(f"\n{name}: sigma2_cond e_dev {e_dev:.2e} e_f64 {e_f64:.2e}; smallest gap {min(ref['gap']):.2e}")
    assert e_dev <= 10 * max(e_f64, 1e-15)


def test_one_unit_with_weight_one_has_the_bits_of_no_weights(lib, counts):
    Sigma, mu = sel.single_inputs("projected130")
    a = raw(lib, [T(Sigma)], [T(mu)], [0.5], None, counts, 8)
    b = raw(lib, [T(Sigma)], [T(mu)], [0.5], [1.0], counts, 8)
    assert a[1].tolist() == b[1].tolist() and same_bits(a[2], b[2]) and same_bits(a[3], b[3])


# ------------------------------------------------------------------ 6. repeatability
def test_work_content_and_repeats_do_not_change_a_bit(lib, counts):
    Sigma, mu = sel.single_inputs("identity300")
    args = ([T(Sigma)], [T(mu)], [1.0], None, counts, 128)
    zeros = raw(lib, *args, fill=0.0)
    nans = raw(lib, *args, fill=float("nan"))
    again = raw(lib, *args, fill=0.0)
    for other in (nans, again):
        assert other[0] == 0 and other[1].tolist() == zeros[1].tolist()
        assert same_bits(other[2], zeros[2]) and same_bits(other[3], zeros[3]) and same_bits(other[4], zeros[4])
    assert not torch.isnan(nans[4]).any()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_picked_untouched(lib, counts):
    from gaussian_processes_amd import _lib
    Sigma, mu = sel.single_inputs("identity130")
    S, m = T(Sigma), T(mu)
    for n_select, n_units, why in ((0, None, "n_select"), (129, None, "n_select"), (8, 0, "units"), (8, 17, "units")):
        rc, picked, utility, s2, _ = raw(lib, [S], [m], [1.0], None, counts, n_select, n_units=n_units)
        assert rc == -3 and why in _lib.last_error(), (n_select, n_units, _lib.last_error())
        assert bool((picked == SENTINEL).all()) and bool((utility == SENTINEL).all()) and bool((s2 == SENTINEL).all())


# ------------------------------------------------------------------ 8. select_round
def _cells(name):
    from gaussian_processes_amd import utils as gp
    group = {g[0]: g for g in groups.GROUPS}[name]
    pool = T(np.array(groups.pool(group[1])))
    out = []
    for c in groups.make_group(group):
        mask = torch.from_numpy(c["mask"]).cuda()
        dev = {k: T(c[k]) for k in ("C", "K", "Kinv", "m", "V")}
        B = gp._mark_identity(torch.eye(c["nt"], dtype=torch.float64, device="cuda")) if c["B"] is None else T(c["B"])
        out.append({"xtilde": T(c["xtilde"])[:, mask].contiguous(), "C": dev["C"], "theta": c["theta"], "mask": mask,
                    "folded": gp.fold_posterior(dev["K"], dev["Kinv"], dev["m"], dev["V"], B), "f_params": link(1.0)})
    return pool, out


@pytest.mark.parametrize("n_cells", [1, 3])
def test_select_round_returns_pool_indices(gp, counts, n_cells):
    pool, cells = _cells("PROJECTED3")
    cells = cells[:n_cells]
    weights = None if n_cells == 1 else [1.0, 0.5, 2.0]
    P = pool.shape[0]
    out = gp.select_round(pool, cells, 8, counts, weights=weights, shortlist=64)
    picked = out["picked"].tolist()
    keep = out["shortlist"]
    assert len(set(picked)) == 8 and all(0 <= i < P for i in picked)
    assert keep.numel() == 64 and bool((keep[1:] > keep[:-1]).all()) and set(picked) <= set(keep.tolist())
    # the shortlist is the 64 rows of largest population utility
    total = out["scores"]["population_utility"]
    assert set(keep.tolist()) == set(torch.topk(total, 64).indices.tolist())
    # select_batch on the hand-built shortlist
    rows = pool[keep].contiguous()
    Sigmas = [gp.pool_covariance(rows, c["xtilde"], c["C"], c["theta"], c["folded"], c["mask"]) for c in cells]
    mus = [out["scores"]["mu"][u][keep] for u in range(n_cells)]
    hand = gp.select_batch(Sigmas, mus, [c["f_params"] for c in cells], counts, 8, weights)
    assert keep[hand["picked"]].tolist() == picked and same_bits(hand["utility"], out["utility"])
    # the first pick is the best image of the plain score
    assert picked[0] == int(total.argmax())
    # shortlist >= P: the whole pool
    whole = gp.select_round(pool, cells, 8, counts, weights=weights, shortlist=4096)
    assert whole["shortlist"].tolist() == list(range(P)) and whole["picked"][0] == picked[0]
    with pytest.raises(ValueError, match="shortlist"):
        gp.select_round(pool, cells, 8, counts, shortlist=gp.POOL_ROWS + 1)
