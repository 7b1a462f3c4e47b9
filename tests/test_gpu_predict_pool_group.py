"""Scoring one stimulus pool for several cells in one device call (gpfit_score_pool_batch through utils._score_pool_group
and utils.score_pool_cells) and the utility of the population (gpfit_utility_sum).

The property everything rests on: for every unit the group call has the bits of the single call (utils.score_pool) on that
unit alone -- whatever the other units, their number, their order, chunk_rows, or the workspaces' capacities.  Accuracy is
therefore the single call's; it is checked once more on the new shapes by the rule of
test_gpu_predict_pool.test_moments_are_as_accurate_as_todays_composition, unchanged: the error against the long-double
restatement of lambda_moments_star may be at most ten times that of lambda_moments_star on the same inputs (relative to
max |.|, floored at 1e-15), which measures the composition, not the code under test.

Shapes: predict_group_cases (PROJECTED3, IDENTITY3, SIXTEEN, MIXED), the smallest at which the group mechanisms can fail.
IDENTITY3's second unit has as many inducing images as the pool has rows; acosker symmetrises a square kernel matrix, so
its references (lambda_moments_star, the long-double form) are evaluated over the two halves of the pool."""
import contextlib
import ctypes
import functools
import io
import warnings

import numpy as np
import pytest
import torch

import predict_cases as cases
import predict_group_cases as groups
from gaussian_processes_amd import synthetic as syn

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
WORK_MATRICES = (b"Abuf", b"Tbuf", b"Wbuf", b"Zbuf", b"Cos", b"TmpV")
KEYS = ("mu", "sigma2", "rate", "utility")
LOWER, UPPER = syn.limits()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


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
    return torch.arange(0, 100, dtype=torch.float64).cuda()


@functools.lru_cache(maxsize=None)
def _pool(P):
    return T(np.array(groups.pool(P)))       # (a copy: the shared array is read-only)


@functools.lru_cache(maxsize=None)
def _units(name):
    """The units of a group on the device (shared between the tests, never written): per unit the arguments of
    score_pool by name -- the pool of whole images, the unit's mask -- and what the references need."""
    from gaussian_processes_amd import utils as gp
    group = {g[0]: g for g in groups.GROUPS}[name]
    out = []
    for c in groups.make_group(group):
        mask = torch.from_numpy(c["mask"]).cuda()
        dev = {k: T(c[k]) for k in ("C", "K", "Kinv", "m", "V")}
        B = gp._mark_identity(torch.eye(c["nt"], dtype=torch.float64, device="cuda")) if c["B"] is None else T(c["B"])
        out.append({"xstar": _pool(c["P"]), "xtilde": T(c["xtilde"])[:, mask].contiguous(), "C": dev["C"], "theta": c["theta"],
                    "folded": gp.fold_posterior(dev["K"], dev["Kinv"], dev["m"], dev["V"], B), "mask": mask,
                    "f_params": {"logA": torch.tensor(c["logA"], dtype=torch.float64),
                                 "lambda0": torch.tensor(c["lambda0"], dtype=torch.float64)},
                    "_ref": dict(dev, B=B)})
    return out


def unit_args(u):
    return {k: v for k, v in u.items() if not k.startswith("_")}


@functools.lru_cache(maxsize=None)
def _single(name):
    """score_pool on every unit of a group alone (computed once, never written)."""
    from gaussian_processes_amd import utils as gp
    r = torch.arange(0, 100, dtype=torch.float64).cuda()
    return [gp.score_pool(u["xstar"], u["xtilde"], u["C"], u["theta"], u["folded"], u["f_params"], r_masked=r, mask=u["mask"])
            for u in _units(name)]


def assert_units_equal(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for key in KEYS:
            assert not torch.isnan(g[key]).any(), (what, i, key)
            assert same_bits(g[key], w[key]), (what, i, key)


# ------------------------------------------------------------------ 1. bit identity with the single call
@pytest.mark.parametrize("name", ["PROJECTED3", "IDENTITY3", "SIXTEEN"])
def test_every_unit_has_the_bits_of_the_single_call(gp, counts, name):
    units = [unit_args(u) for u in _units(name)]
    got = gp._score_pool_group(units, counts, 0)
    assert all(g[key].shape == (units[0]["xstar"].shape[0],) for g in got for key in KEYS)
    assert_units_equal(got, _single(name), name)


@pytest.mark.parametrize("chunk_rows", [128, 256, 0])
def test_chunking_does_not_change_a_bit(gp, counts, chunk_rows):
    units = [unit_args(u) for u in _units("IDENTITY3")]
    assert_units_equal(gp._score_pool_group(units, counts, chunk_rows), _single("IDENTITY3"), chunk_rows)


def test_order_and_number_of_the_units_do_not_change_a_bit(gp, counts):
    units = [unit_args(u) for u in _units("PROJECTED3")]
    want = _single("PROJECTED3")
    assert_units_equal(gp._score_pool_group(units[::-1], counts, 0), want[::-1], "reversed")
    for i in range(3):
        assert_units_equal(gp._score_pool_group(units[i:i + 1], counts, 0), want[i:i + 1], ("alone", i))
    assert_units_equal(gp._score_pool_group(units[:2], counts, 0), want[:2], "first two")
    assert_units_equal(gp._score_pool_group([units[2], units[0]], counts, 128), [want[2], want[0]], "last and first")


def test_no_response_counts_no_utility(gp):
    units = [unit_args(u) for u in _units("PROJECTED3")]
    got = gp._score_pool_group(units, None, 0)
    for g, w in zip(got, _single("PROJECTED3")):
        assert g["utility"] is None and all(same_bits(g[key], w[key]) for key in KEYS[:3])


# ------------------------------------------------------------------ 2. accuracy of the new shapes
@pytest.mark.parametrize("name,index", [(n, i) for n in ("PROJECTED3", "IDENTITY3") for i in range(3)])
def test_moments_are_as_accurate_as_todays_composition(gp, counts, name, index):
    group = {g[0]: g for g in groups.GROUPS}[name]
    c, u = groups.make_group(group)[index], _units(name)[index]
    mu_ref, s2_ref = groups.group_reference(group)[index]
    got = gp._score_pool_group([unit_args(v) for v in _units(name)], counts, 0)[index]
    xs, ref = u["xstar"][:, u["mask"]].contiguous(), u["_ref"]
    old = [gp.lambda_moments_star(xs[rows].contiguous(), u["xtilde"], u["C"], u["theta"], ref["K"], ref["Kinv"], ref["m"], ref["V"],
                                  ref["B"], "acosker") for rows in groups.reference_rows(c)]
    mu_o = torch.cat([o[0].reshape(-1) for o in old]).cpu().numpy()
    s2_o = torch.cat([o[1].reshape(-1) for o in old]).cpu().numpy()
    e_new = (cases.err(got["mu"].cpu().numpy(), mu_ref), cases.err(got["sigma2"].cpu().numpy(), s2_ref))
    e_old = (cases.err(mu_o, mu_ref), cases.err(s2_o, s2_ref))
    print(f"\n{name}[{index}] {(c['nt'], c['k'], c['d'])}: mu e_new {e_new[0]:.2e} e_old {e_old[0]:.2e} | "
          f"sigma2 e_new {e_new[1]:.2e} e_old {e_old[1]:.2e}")
    assert e_new[0] <= 10 * max(e_old[0], 1e-15)
    assert e_new[1] <= 10 * max(e_old[1], 1e-15)


# ------------------------------------------------------------------ 3. the utility of the population
def loop_sum(U, w):
    acc = w[0] * U[0]
    for u in range(1, U.shape[0]):
        acc = acc + w[u] * U[u]
    return acc


def test_population_utility_is_the_loop_in_the_callers_order(gp, counts, monkeypatch):
    cells = [unit_args(u) for u in _units("MIXED")]
    pool = cells[0]["xstar"]
    w = torch.tensor([0.5, 2.0, 1.25, 0.75, 3.0], dtype=torch.float64).cuda()
    ones = torch.ones(5, dtype=torch.float64).cuda()
    out = gp.score_pool_cells(pool, cells, r_masked=counts, weights=w)
    assert gp.last_pool_group_sizes == [3, 1, 1] and out["errors"] == [None] * 5
    assert_units_equal([{key: out[key][i] for key in KEYS} for i in range(5)], _single("MIXED"), "MIXED")
    assert same_bits(out["population_utility"], loop_sum(out["utility"], w))
    plain = gp.score_pool_cells(pool, cells, r_masked=counts)
    assert same_bits(plain["population_utility"], loop_sum(plain["utility"], ones))
    assert not same_bits(plain["population_utility"], out["population_utility"])
    cut = gp.score_pool_cells(pool, cells, r_masked=counts, weights=w, max_units=2)
    assert gp.last_pool_group_sizes == [2, 1, 1, 1]
    monkeypatch.setattr(gp, "POOL_GROUPS", False)          # what GPFIT_POOL_GROUPS=0 sets
    alone = gp.score_pool_cells(pool, cells, r_masked=counts, weights=w)
    assert gp.last_pool_group_sizes == [1] * 5
    for other in (cut, alone):
        assert all(same_bits(other[key], out[key]) for key in KEYS + ("population_utility",))
    assert gp.score_pool_cells(pool, cells)["population_utility"] is None


def test_utility_sum_of_more_rows_than_a_group_and_nan(gp, lib):
    P, n, ldu = 1000, 17, 1003
    g = torch.Generator(device="cpu").manual_seed(3)
    base = torch.randn(n, ldu, dtype=torch.float64, generator=g).cuda()
    w = torch.rand(n, dtype=torch.float64, generator=g).cuda() + 0.5
    U = base[:, :P]
    assert same_bits(gp._utility_sum(U, w), loop_sum(U, w))
    assert same_bits(gp._utility_sum(U), loop_sum(U, torch.ones(n, dtype=torch.float64).cuda()))
    # the rows in place, with their leading dimension; out starts as the sentinel and only its first P entries are written
    out = torch.full((P + 5,), SENTINEL, dtype=torch.float64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.gpfit_utility_sum(stream, base.data_ptr(), ldu, n, w.data_ptr(), P, out.data_ptr()) == 0
    torch.cuda.synchronize()
    assert same_bits(out[:P], loop_sum(U, w)) and bool((out[P:] == SENTINEL).all())
    holed = U.clone()
    holed[5, 321] = float("nan")
    total = gp._utility_sum(holed, w)
    nan = torch.isnan(total)
    assert bool(nan[321]) and int(nan.sum()) == 1
    keep = torch.ones(P, dtype=torch.bool, device="cuda")
    keep[321] = False
    assert same_bits(total[keep], loop_sum(U, w)[keep])
    assert lib.gpfit_utility_sum(stream, base.data_ptr(), P - 1, n, None, P, out.data_ptr()) == -3      # ldu < P
    assert lib.gpfit_utility_sum(stream, base.data_ptr(), ldu, 0, None, P, out.data_ptr()) == -3


# ------------------------------------------------------------------ 4. stale workspace
def test_padding_is_written_not_assumed(gp, lib, counts):
    units = [unit_args(u) for u in _units("PROJECTED3")]
    want = _single("PROJECTED3")
    engines = gp._group_engines(3, 256, 64, 64)            # the workspaces the group call takes
    for e in engines:
        for name in WORK_MATRICES:
            assert lib.gpfit_dev_ctx_fill(e._ctx, name, 0xFF) == 0          # every double a NaN
    try:
        assert all(a is b for a, b in zip(gp._group_engines(3, 256, 64, 64), engines))
        assert_units_equal(gp._score_pool_group(units, counts, 0), want, "stale workspace")
    finally:
        for e in engines:
            for name in WORK_MATRICES:
                assert lib.gpfit_dev_ctx_fill(e._ctx, name, 0) == 0         # as a fresh context holds them


# ------------------------------------------------------------------ 5. refusals through the raw entry point
def requests(gp, units):
    qs = []
    for u in units:
        q = gp._score_pool_prepare(u["xstar"], u["xtilde"], u["C"], u["theta"], u["folded"], u.get("mask"))
        q["A"], q["lambda0"] = gp._link_scalars(u["f_params"])
        qs.append(q)
    return qs


def raw(gp, ctxs, qs, r, chunk_rows=0, with_U=True):
    """gpfit_score_pool_batch itself: (rc, outputs [n][4][P] that started as the sentinel)."""
    out = torch.full((len(qs), 4, 130), SENTINEL, dtype=torch.float64, device="cuda")
    rc = gp._score_pool_batch_raw(ctxs, qs, r, chunk_rows, *[[out[i, j] for i in range(len(qs))] for j in range(3)],
                                  [out[i, 3] for i in range(len(qs))] if with_U else None)
    torch.cuda.synchronize()
    return rc, out


def with_basis_of(gp, unit, k):
    """The unit with a made-up posterior in a basis of k columns (a refusal needs no meaningful one)."""
    nt = unit["xtilde"].shape[0]
    g = torch.Generator(device="cpu").manual_seed(k)
    B = torch.linalg.qr(torch.randn(nt, k, dtype=torch.float64, generator=g))[0].contiguous().cuda()
    S = torch.randn(k, k, dtype=torch.float64, generator=g)
    folded = {"S": (0.5 * (S + S.T) / k).contiguous().cuda(), "w": (torch.randn(k, dtype=torch.float64, generator=g) / k).cuda(),
              "B": B, "k": k}
    return dict(unit, folded=folded)


def test_refusals(gp, counts):
    from gaussian_processes_amd import _lib
    from gaussian_processes_amd.engine import GPFitEngine
    units = [unit_args(u) for u in _units("MIXED")]
    qs = requests(gp, units)
    ctxs = [e._ctx for e in gp._group_engines(3, 256, 64, 64)]

    def refused(rc, out, *words):
        err = _lib.last_error()
        assert rc == -3 and bool((out == SENTINEL).all()), (rc, err)
        assert err.startswith("gpfit_score_pool_batch: ") and all(word in err for word in words), err

    refused(*raw(gp, [ctxs[0]] * 17, [qs[0]] * 17, counts), "1 .. 16 units")
    refused(*raw(gp, [ctxs[0], ctxs[1], ctxs[0]], qs[:3], counts), "unit 2: ", "context of its own")
    wide = requests(gp, [with_basis_of(gp, units[1], 130)])[0]                 # round_up(k, 128) = 256 beside 128
    refused(*raw(gp, ctxs, [qs[0], wide, qs[2]], counts), "unit 1: ", "round_up(k, 128)")
    refused(*raw(gp, ctxs[:2], [wide, qs[3]], counts), "unit 1: ", "basis")     # (200, 130) with B beside (200, 200) without
    small = GPFitEngine(64, 64, 64)                                            # capacity 128 < nt
    try:
        refused(*raw(gp, [ctxs[0], small._ctx, ctxs[1]], qs[:3], counts), "unit 1: ", "larger than the context capacity")
    finally:
        small.close()
    refused(*raw(gp, ctxs, qs[:3], counts, chunk_rows=100), "chunk_rows")
    with pytest.raises(_lib.GpfitError, match="chunk_rows"):
        _lib.check(-3, "gpfit_score_pool_batch")
    # an empty pool: nothing to do, nothing written
    rc, out = raw(gp, ctxs, [dict(q, P=0) for q in qs[:3]], counts)
    assert rc == 0 and bool((out == SENTINEL).all())
    # no response counts: the moments and the rate, no U[u] touched
    rc, out = raw(gp, ctxs, qs[:3], None)
    assert rc == 0 and not bool((out[:, :3] == SENTINEL).any()) and bool((out[:, 3] == SENTINEL).all())
    for i, w in enumerate(_single("MIXED")[:3]):
        assert all(same_bits(out[i, j], w[key]) for j, key in enumerate(KEYS[:3]))


# ------------------------------------------------------------------ 6. one round of a population's closed loop
def test_one_population_round_picks_the_images_of_the_single_calls(gp, counts):
    n0, P, px, per_round = 64, 130, 8, 4
    X = T(syn.stimuli(n0 + P, px * px))
    rs = [T(syn.cell_inputs(n0 + P, cell)[0])[:n0] for cell in range(3)]

    def start(cell):
        theta = {k: torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for k, v in syn.theta0().items()}
        fit = {"ntilde": n0, "maxiter": 2, "nEstep": 2, "nMstep": 3, "nFparamstep": 3, "kernfun": "acosker", "cellid": cell,
               "n_px_side": px, "display_hyper": False}
        return {"fit_parameters": fit, "xtilde": X[:n0].clone(), "hyperparams_tuple": (theta, LOWER, UPPER),
                "f_params": {"logA": torch.tensor(syn.F_PARAMS["logA"], dtype=torch.float64, requires_grad=True),
                             "lambda0": torch.tensor(syn.F_PARAMS["lambda0"], dtype=torch.float64)}}

    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fits = gp.varGP_cells(X[:n0], rs, [start(cell) for cell in range(3)])
    assert not any(err["is_error"] for _, err in fits)
    cells = [{"xtilde": X[:n0], "C": m["C"], "theta": m["hyperparams_tuple"][0], "f_params": m["f_params"], "mask": m["mask"],
              "folded": gp.fold_posterior(m["K_tilde_b"], m["K_tilde_inv_b"], m["m_b"], m["V_b"], m["B"])} for m, _ in fits]
    pool = X[n0:]
    out = gp.score_pool_cells(pool, cells, r_masked=counts)
    assert sum(gp.last_pool_group_sizes) == 3 and out["errors"] == [None] * 3
    alone = [gp.score_pool(pool, c["xtilde"], c["C"], c["theta"], c["folded"], c["f_params"], r_masked=counts, mask=c["mask"])
             for c in cells]
    total = loop_sum(torch.stack([a["utility"] for a in alone]), torch.ones(3, dtype=torch.float64).cuda())
    assert not torch.isnan(total).any()
    assert same_bits(out["population_utility"], total)
    assert torch.equal(torch.topk(out["population_utility"], per_round).indices, torch.topk(total, per_round).indices)
