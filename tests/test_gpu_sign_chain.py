"""The projector step of a basis rebuild as device calls (gpfit_sign_steps, gpfit_sign_steps_batch; utils._sign_steps,
_sign_steps_group) against the host loop of eigtop._kept_subspace through cholesky / matmul / gemm_into, bit for bit:
alone, in groups, beside a failing unit, behind the switches SIGN_CHAIN and BASIS_GROUPS, in one fit and in a wave of
varGP_cells.  The host loop is the hook of tests/test_sign_chain_cpu.py on the library's own primitives."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from gaussian_processes_amd import _lib, eigtop, synthetic as syn
from test_sign_chain_cpu import SIZES, TAU, TorchSignHook, gap_matrix
from test_gpu_trunc_group import assert_same_fit, in_a_thread

pytestmark = pytest.mark.gpu
KEYS = syn.THETA_KEYS
LOWER, UPPER = syn.limits()
CAYLEY, X2_READY = 1, 2
CS11 = eigtop._sign_schedule(eigtop._SIGN_L0, 0, 40)[0]


@pytest.fixture(scope="module")
def gp():
    from gaussian_processes_amd import utils
    return utils


def T(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).cuda()


@functools.lru_cache(maxsize=None)
def matrix(k, seed=0, negative=False):
    """(S, tau) on the device: the gap matrix of the CPU test, each seed with a scale (so a threshold) of its own;
    computed once, never written."""
    scale = 1.0 + 0.25 * seed
    return gap_matrix(k, 1.0, seed=seed, negative=negative, scale=scale).cuda().contiguous(), TAU * scale


def host_loop(gp):
    return TorchSignHook(gp.matmul, gp.cholesky, gp.gemm_into)


def assert_same(got, want, what):
    assert got is not None and want is not None, what
    for name, x, y in zip(("X", "X2"), got, want):
        assert torch.equal(x, y), (what, name)


@pytest.mark.parametrize("k", SIZES)
def test_the_single_call_has_the_bits_of_the_host_loop(gp, k):
    """k = 48: one padded leaf; 160: two leaves, no multiple of 128; 256.  Head + 11 steps, head alone, one step on a
    ready X2 at its0 = 11, and stretches that cross its = 7 and 15 (the symmetrisations)."""
    S, tau = matrix(k)
    keep = S.clone()
    loop = host_loop(gp)
    want = loop(S, tau, None, None, CS11, 0)
    got = gp._sign_steps(S, tau, None, None, CS11, 0)
    assert_same(got, want, (k, "head + 11"))
    assert torch.equal(S, keep)                                  # S is left alone
    assert float((gp.matmul(got[0], got[0]) - got[1]).abs().max()) == 0.0
    assert_same(gp._sign_steps(S, tau, None, None, [], 0), loop(S, tau, None, None, [], 0), (k, "head alone"))
    head = loop(S, tau, None, None, [], 0)
    assert torch.equal(head[0], head[0].T)
    # a straggler's stretch: X and the ready product of the first stretch, one more step
    step = loop(S, tau, want[0].clone(), want[1].clone(), [CS11[-1]], 11)
    assert_same(gp._sign_steps(S, tau, want[0].clone(), want[1].clone(), [CS11[-1]], 11), step, (k, "X2 ready"))
    # the same step counted from 0 is another number where the count decides a symmetrisation: its0 = 7
    sym = loop(S, tau, want[0].clone(), want[1].clone(), [CS11[-1]], 7)
    assert_same(gp._sign_steps(S, tau, want[0].clone(), want[1].clone(), [CS11[-1]], 7), sym, (k, "its0 = 7"))
    assert torch.equal(sym[0], sym[0].T)
    for n in (16, 17):                                           # across its = 7 and 15; 16 ends on a symmetrisation
        cs = CS11 + [1.0] * (n - 11)
        want_n, got_n = loop(S, tau, None, None, cs, 0), gp._sign_steps(S, tau, None, None, cs, 0)
        assert_same(got_n, want_n, (k, n))
        assert torch.equal(got_n[0], got_n[0].T) == torch.equal(want_n[0], want_n[0].T) == (n == 16)
    # a stretch without the head and without a ready product, from its0 = 5
    cs = [1.05, 1.0, 1.0, 1.0]
    assert_same(gp._sign_steps(S, tau, head[0].clone(), None, cs, 5), loop(S, tau, head[0].clone(), None, cs, 5), (k, "no flags"))
    assert torch.equal(S, keep)


def raw_group(gp, units, engines=None):
    """gpfit_sign_steps_batch through the C ABI on hand-built requests: the (steps, info) pairs and the requests."""
    engines = engines or gp._group_engines(len(units), int(units[0]["S"].shape[0]), exact=True)
    qs = [gp._sign_prepare(engine=e, **u) for u, e in zip(units, engines)]
    rc, rec = gp._sign_batch_raw([q["engine"]._ctx for q in qs], qs)
    assert rc == 0, _lib.last_error()
    return [(rec[2 * u], rec[2 * u + 1]) for u in range(len(qs))], qs


def test_every_unit_of_a_group_has_the_bits_of_its_single_call(gp):
    """Three units at k = 160 with their own S and tau: one call through the wrapper and one through the C ABI."""
    k = 160
    probs = [matrix(k, seed) for seed in range(3)]
    singles = [gp._sign_steps(S, tau, None, None, CS11, 0) for S, tau in probs]
    units = [{"S": S, "tau": tau, "cs": CS11} for S, tau in probs]
    group = gp._sign_steps_group(units)
    assert len(group) == 3
    for i in range(3):
        assert_same(group[i], singles[i], ("group", i))
    assert not torch.equal(group[0][0], group[1][0])
    rec, qs = raw_group(gp, units)
    assert rec == [(11, 0)] * 3
    for i, q in enumerate(qs):
        assert_same(gp._sign_result(q, i, [11, 0] * 3), singles[i], ("raw group", i))
    # second stretches as a group: the units' own X and ready products, one shared schedule
    units2 = [{"S": S, "tau": tau, "X": x.clone(), "X2": x2.clone(), "cs": [1.0, 1.0], "its0": 6}
              for (S, tau), (x, x2) in zip(probs, singles)]
    group2 = gp._sign_steps_group(units2)
    for i, (S, tau) in enumerate(probs):
        assert_same(group2[i], gp._sign_steps(S, tau, singles[i][0].clone(), singles[i][1].clone(), [1.0, 1.0], 6), ("stretch", i))


def test_a_unit_whose_head_is_indefinite_fails_alone(gp):
    """Unit 1 has an eigenvalue at -2 tau: S + tau I is indefinite.  It reports no steps and a positive info; units 0 and
    2 finish with the bits of their single calls."""
    k = 160
    probs = [matrix(k, 0), matrix(k, 1, True), matrix(k, 2)]
    units = [{"S": S, "tau": tau, "cs": CS11} for S, tau in probs]
    rec, qs = raw_group(gp, units)
    assert rec[0] == (11, 0) and rec[2] == (11, 0) and rec[1][0] == 0 and rec[1][1] > 0, rec
    for i in (0, 2):
        assert_same(gp._sign_result(qs[i], 0, [11, 0]), gp._sign_steps(*probs[i], None, None, CS11, 0), ("beside a failure", i))
    group = gp._sign_steps_group(units)
    assert group[1] is None and group[0] is not None and group[2] is not None
    assert_same(group[2], gp._sign_steps(*probs[2], None, None, CS11, 0), "wrapper, beside a failure")
    assert gp._sign_steps(*probs[1], None, None, CS11, 0) is None
    assert host_loop(gp)(*probs[1], None, None, CS11, 0) is None


def test_the_refusals_of_the_entry_points(gp):
    k = SIZES[0]
    S, tau = matrix(k)
    eng, other = gp._group_engines(2, k)
    q = gp._sign_prepare(S, tau, None, None, CS11, 0, engine=eng)
    lib = _lib.load()
    rec = (ctypes.c_int * 40)()

    def refused(ctxs, qs, word, name="gpfit_sign_steps_batch: "):
        rc, _ = gp._sign_batch_raw(ctxs, qs, rec)
        assert rc == -3 and name in _lib.last_error() and word in _lib.last_error(), (word, rc, _lib.last_error())
    refused([eng._ctx] * 17, [q] * 17, "1 .. 16 units")
    assert lib.gpfit_sign_steps_batch(gp._ctx_table([eng._ctx]), 0, q["stream"], gp._ptr_table([q], "S"), k, _lib.darr([tau]),
                                      gp._ptr_table([q], "X"), gp._ptr_table([q], "X2"), gp._ptr_table([q], "W"), 11,
                                      _lib.darr(CS11), 0, CAYLEY, rec) == -3
    assert "1 .. 16 units" in _lib.last_error()
    refused([eng._ctx, eng._ctx], [q, q], "context of its own")
    for what, word, over in (("k no multiple of 16", "bad size", {"k": 40}), ("k below 16", "bad size", {"k": 8}),
                             ("unknown flag", "unknown flag", {"flags": 5}),
                             ("a ready X2 with the head", "no X2 can be ready", {"flags": CAYLEY | X2_READY}),
                             ("too many steps", "n_steps = 65 is not within 0 .. 64", {"c": [1.0] * 65}),
                             ("a negative count", "its0", {"its0": -1}), ("no X", "null context or operand", {"X": None}),
                             ("the head without S", "null context or operand", {"S": None})):
        refused([eng._ctx], [dict(q, **over)], word)
    # steps without scalings: the single entry point, under its own name
    assert lib.gpfit_sign_steps(eng._ctx, q["stream"], S.data_ptr(), k, tau, q["X"].data_ptr(), q["X2"].data_ptr(),
                                q["W"].data_ptr(), 3, None, 0, CAYLEY, rec) == -3
    assert "gpfit_sign_steps: " in _lib.last_error() and "no scalings" in _lib.last_error()
    # two faults in one call -- unit 1 has no spare block, unit 2 is on unit 0's context: the units are checked in order
    refused([eng._ctx, other._ctx, eng._ctx], [q, dict(q, W=None), q], "gpfit_sign_steps_batch: unit 1: bad argument")
    small = gp.GPFitEngine(128, 1, 1, device=eng.device)
    S2, tau2 = matrix(256)
    refused([small._ctx], [gp._sign_prepare(S2, tau2, None, None, CS11, 0, engine=small)], "capacity")
    # and the request itself is accepted as it is
    rc, out = gp._sign_batch_raw([eng._ctx], [q])
    assert rc == 0 and (out[0], out[1]) == (11, 0)


@functools.lru_cache(maxsize=None)
def kernel_matrix(N, cell=0):
    """(K~, tol, count): the kernel matrix of N stimuli of 8 x 8 pixels and a tolerance at which it is truncated.  At the
    default tolerance every eigenvalue of so small a matrix is kept (the identity route, no basis to compare), so the
    threshold goes into the widest relative gap of the spectrum away from its ends, where the count is as clear as a
    count can be: the Cayley transform of both neighbours lies ten times further from zero than the bound the scaled
    sign iteration assumes (_SIGN_L0)."""
    from gaussian_processes_amd import utils as gp
    th = {key: torch.tensor(float(syn.theta0(cell)[key]), dtype=torch.float64) for key in KEYS}
    X = T(syn.stimuli(N, 64))
    C, mask = gp.localker(th, UPPER, LOWER, 8)
    xm = X[:, mask].contiguous()
    K = gp.acosker(th, xm, xm, C=C)
    K = ((K + K.T) * 0.5).contiguous()
    w = torch.linalg.eigvalsh(K).cpu()                            # ascending
    lo, hi = N // 8, N - 8
    i = lo + int(torch.argmax(w[lo + 1:hi + 1] / w[lo:hi]))
    tol = math.sqrt(float(w[i]) * float(w[i + 1])) / float(w[-1])
    print(f"N {N}: threshold between eigenvalues {float(w[i]):.4g} and {float(w[i + 1]):.4g} (lambda_max {float(w[-1]):.4g}), "
          f"tol {tol:.3e}, {N - i - 1} kept")
    ratio = math.sqrt(float(w[i + 1]) / float(w[i]))              # of either neighbour to the threshold
    assert (ratio - 1.0) / (ratio + 1.0) > 10.0 * eigtop._SIGN_L0 and tol > 1e-4
    return K, tol, N - i - 1


def counting(gp, calls):
    def chain(*a):
        calls.append((a[2] is None, len(a[4]), a[5]))
        return gp._sign_steps(*a)
    return chain


def test_the_dense_route_with_the_hook_and_without(gp):
    """kept_eigenspace_dense on the kernel matrix of 384 stimuli of 8 x 8 pixels: the same B, K_tilde_b, K_tilde_inv_b,
    count and sign iterations, bit for bit; the hook was really called."""
    K, tol, count = kernel_matrix(384)
    calls = []
    off = eigtop.kept_eigenspace_dense(K, tol, gp.matmul, gp.cholesky, gemm_into=gp.gemm_into)
    on = eigtop.kept_eigenspace_dense(K, tol, gp.matmul, gp.cholesky, gemm_into=gp.gemm_into, sign_chain=counting(gp, calls))
    assert off is not None and on is not None and off[1] is not None and on[1] is not None
    assert on[2]["n"] == count and on[1].shape == (384, count)
    assert calls and calls[0] == (True, 11, 0) and sum(c[1] for c in calls) == on[2]["sign_iterations"]
    assert on[2]["n"] == off[2]["n"] and on[2]["sign_iterations"] == off[2]["sign_iterations"]
    assert torch.equal(on[1], off[1])
    for key in ("K_tilde_b", "K_tilde_inv_b"):
        assert torch.equal(on[2][key], off[2][key]), key


def test_top_eigenpairs_with_both_chains_on_and_off(gp):
    """The gap matrix of tests/test_gpu_sweep_chain.py (n = 384, k0 = 128): bit-equal results and counters."""
    n, tol = 384, 1e-4
    g = torch.Generator().manual_seed(3)
    Qm, _ = torch.linalg.qr(torch.randn(n, n, dtype=torch.float64, generator=g))
    lam = torch.cat([torch.logspace(2, 0, 60, dtype=torch.float64), torch.logspace(-4, -6, n - 60, dtype=torch.float64)])
    K = (Qm * lam) @ Qm.T
    K = ((K + K.T) / 2).cuda().contiguous()
    calls = []
    kw = dict(k0=128, basis="subspace", gemm_into=gp.gemm_into)
    off = eigtop.top_eigenpairs(K, tol, gp.matmul, gp.cholesky, **kw)
    on = eigtop.top_eigenpairs(K, tol, gp.matmul, gp.cholesky, sweep_chain=gp._basis_sweeps, sign_chain=counting(gp, calls), **kw)
    assert off is not None and on is not None and off[0] is None and on[0] is None
    assert calls and calls[0][0] and calls[0][1] == 11
    assert on[2]["n"] == off[2]["n"] == 60
    assert torch.equal(on[1], off[1])
    for key in ("K_tilde_b", "K_tilde_inv_b"):
        assert torch.equal(on[2][key], off[2][key]), key
    for key in ("sweeps", "products", "k", "grown", "rr", "sign_iterations"):
        assert on[2][key] == off[2][key], key
    assert torch.equal(on[2]["state"]["Q"], off[2]["state"]["Q"]) and torch.equal(on[2]["state"]["U"], off[2]["state"]["U"])


# ---------------------------------------------------------------------------------------------- whole fits
def fit_args(N, X):
    th = {k: torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for k, v in syn.theta0(3).items()}
    fp = {"ntilde": N, "maxiter": 3, "nEstep": 2, "nMstep": 4, "nFparamstep": 3, "kernfun": "acosker", "cellid": 0,
          "n_px_side": 8, "display_hyper": False}
    return {"fit_parameters": fp, "xtilde": X, "hyperparams_tuple": (th, LOWER, UPPER),
            "f_params": {"logA": torch.tensor(syn.F_PARAMS["logA"], dtype=torch.float64, requires_grad=True),
                         "lambda0": torch.tensor(syn.F_PARAMS["lambda0"], dtype=torch.float64)}}


@functools.lru_cache(maxsize=None)
def stimuli_and_rates(N, cells):
    return T(syn.stimuli(N, 64)), tuple(T(syn.cell_inputs(N, 3 + c)[0]) for c in range(cells))


_ALONE = {}


def fit_alone(gp, N, cell, sign_chain=True, tol=1e-4):
    """varGP on one cell in a thread of its own, once per (N, cell, switch): (fit, err) and the hook's stretches."""
    key = (N, cell, sign_chain, tol)
    if key not in _ALONE:
        X, rs = stimuli_and_rates(N, 3)
        used = []
        real, was, tol_was = gp._sign_steps, gp.SIGN_CHAIN, gp.EIGVAL_TOL
        gp._sign_steps = lambda *a: used.append(len(a[4])) or real(*a)
        gp.SIGN_CHAIN, gp.EIGVAL_TOL = sign_chain, tol
        try:
            out = in_a_thread(lambda: gp.varGP(X, rs[cell], **fit_args(N, X)), gp)
        finally:
            gp._sign_steps, gp.SIGN_CHAIN, gp.EIGVAL_TOL = real, was, tol_was
        assert not out[1]["is_error"], out[1]
        _ALONE[key] = (out, used)
    return _ALONE[key]


def test_one_fit_with_the_switch_on_and_off(gp):
    """varGP at N = 2048, d = 64, three EM iterations: the same loss track, m_b, V_b, B and routes, bit for bit."""
    (a, used_on), (b, used_off) = fit_alone(gp, 2048, 0, True), fit_alone(gp, 2048, 0, False)
    assert len(used_on) >= 2 and used_on[0] == 11 and not used_off
    assert_same_fit(a, b, "SIGN_CHAIN on / off")
    a, b = a[0], b[0]
    va, vb = a["values_track"]["variation_par_track"], b["values_track"]["variation_par_track"]
    assert va["basis_route"] == vb["basis_route"] and set(va["basis_route"]) == {"subspace"} and a["basis_route"] == b["basis_route"]
    for key in ("m_b", "V_b"):
        for x, y in zip(va[key], vb[key]):
            assert torch.equal(x, y), key
    assert a["B"].shape == b["B"].shape and torch.equal(a["B"], b["B"]) and 0 < a["B"].shape[1] < 1024


def wave(gp, N, cells, on, tol=1e-4):
    X, rs = stimuli_and_rates(N, 3)
    was, tol_was = gp.BASIS_GROUPS, gp.EIGVAL_TOL
    gp.BASIS_GROUPS, gp.EIGVAL_TOL = on, tol
    try:
        out = in_a_thread(lambda: gp.varGP_cells(X, list(rs[:cells]), [fit_args(N, X) for _ in range(cells)]), gp)
    finally:
        gp.BASIS_GROUPS, gp.EIGVAL_TOL = was, tol_was
    books = {book: list(getattr(gp.varGP_cells, "last_" + book + "group_sizes")) for book in gp._ALL_BOOKS}
    assert len(gp.varGP_cells.last_basis_call_seconds) == len(books["basis_"])
    return out, books


def test_the_rebuilds_of_a_wave_meet_on_the_dense_route(gp):
    """Three cells at N = 512 on 8 x 8 stimuli (the projector of K~ itself, no sweeps) with BASIS_GROUPS on: sign calls
    of three units, every fit the fit of varGP alone; off: no basis call at the rendezvous, the other books unchanged."""
    N = 512
    tol = kernel_matrix(N, 3)[1]                  # (the fits start from this kernel matrix: theta0(3))
    cells, books = wave(gp, N, 3, True, tol)
    assert all(not err["is_error"] for _, err in cells)
    assert all(set(fit["values_track"]["variation_par_track"]["basis_route"]) == {"subspace"} for fit, _ in cells)
    sizes = books["basis_"]
    print(f"basis calls by units carried: {sizes}")
    assert sizes and 3 in sizes and all(1 <= n <= 3 for n in sizes) and gp.varGP_cells.last_seconds_in_basis_call > 0.0
    for i in range(3):
        alone, used = fit_alone(gp, N, i, tol=tol)
        assert used, "the fit alone went through the hook"
        assert_same_fit(cells[i], alone, i)
        assert torch.equal(cells[i][0]["B"], alone[0]["B"])
    assert sum(sizes) == sum(len(fit_alone(gp, N, i, tol=tol)[1]) for i in range(3))     # sign stretches only: no sweeps at this size
    cells_off, books_off = wave(gp, N, 3, False, tol)
    assert books_off["basis_"] == [] and gp.varGP_cells.last_seconds_in_basis_call == 0.0
    assert {b: v for b, v in books_off.items() if b != "basis_"} == {b: v for b, v in books.items() if b != "basis_"}
    for i in range(3):
        assert_same_fit(cells_off[i], cells[i], ("off", i))


def test_the_rebuilds_of_a_wave_meet_with_their_sweeps(gp, monkeypatch):
    """Two cells at N = 2048, d = 64: a sweeps call and a sign call carried both, and both fits are the fits alone."""
    N = 2048
    kinds = []
    real = gp._request_run_group
    monkeypatch.setattr(gp, "_request_run_group", lambda qs: kinds.append((qs[0]["kind"], len(qs))) or real(qs))
    cells, books = wave(gp, N, 2, True)
    assert all(not err["is_error"] for _, err in cells)
    print(f"basis calls by units carried: {books['basis_']}")
    assert ("sweeps", 2) in kinds and ("sign", 2) in kinds, kinds
    assert 2 in books["basis_"]
    for i in range(2):
        alone, _ = fit_alone(gp, N, i)
        assert_same_fit(cells[i], alone, i)
        assert torch.equal(cells[i][0]["B"], alone[0]["B"])
        assert set(cells[i][0]["values_track"]["variation_par_track"]["basis_route"]) == {"subspace"}
