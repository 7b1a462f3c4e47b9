"""gpfit_subspace_sweeps / gpfit_subspace_sweeps_batch (the sweeps of a basis rebuild as one device call) on the GPU:
the single call against the host loop it replaces (eigtop's inner loop through utils.matmul and utils.cholesky), bit for
bit; every unit of a group against its single call; a unit whose Gram matrix is singular stops alone; top_eigenpairs and
a whole varGP with the switch on and off.

Shapes (N, k): (160, 48) one padded leaf of the factorisation, N no multiple of 128; (384, 160) a factor of two leaves, k
no multiple of 128; (512, 256).  K~ is the arc-cosine kernel matrix of 8 x 8 synthetic stimuli, Q0 the hash matrix
orthonormalised by the host's CholeskyQR2."""
import contextlib
import ctypes
import functools
import io
import warnings

import numpy as np
import pytest
import torch

from gaussian_processes_amd import _lib, eigtop, synthetic as syn

pytestmark = pytest.mark.gpu
KEYS = syn.THETA_KEYS
LOWER, UPPER = syn.limits()
SHAPES = [(160, 48), (384, 160), (512, 256)]
Y_READY, WANT_RR = 1, 2


@pytest.fixture(scope="module")
def gp():
    from gaussian_processes_amd import utils
    return utils


def T(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).cuda()


@functools.lru_cache(maxsize=None)
def problem(N, k, seed=0):
    """(K~, Q0, shifts [0, s1, s2]); computed once per shape and seed, never written."""
    from gaussian_processes_amd import utils as gp
    th = {key: torch.tensor(float(syn.theta0()[key]), dtype=torch.float64) for key in KEYS}
    X = T(syn.stimuli(N, 64, seed=seed))
    C, mask = gp.localker(th, UPPER, LOWER, 8)
    xm = X[:, mask].contiguous()
    K = gp.acosker(th, xm, xm, C=C)
    K = ((K + K.T) * 0.5).contiguous()
    Q0 = eigtop._cholqr(eigtop._hash_matrix(N, k, K.device, K.dtype), gp.matmul, gp.cholesky, 2)
    assert Q0 is not None
    a = float((Q0 * gp.matmul(K, Q0)).sum(0).min())          # the smallest Rayleigh quotient: shifts well inside the spectrum
    assert a > 0
    return K, Q0.contiguous(), (0.0, 0.6 * a, 0.15 * a)


def host_loop(gp, K, Q, shifts, y_ready, want_rr):
    """What the chain replaces, call for call: the inner loop of top_eigenpairs and the three lines behind it."""
    Y = gp.matmul(K, Q) if y_ready else None
    for j, sigma in enumerate(shifts):
        if not (j == 0 and y_ready):
            Y = gp.matmul(K, Q)
        if sigma != 0.0:
            Y.sub_(Q, alpha=sigma)
        Q = eigtop._cholqr(Y, gp.matmul, gp.cholesky, 2 if j == len(shifts) - 1 else 1)
        assert Q is not None
    if not want_rr:
        return Q, None, None
    Y = gp.matmul(K, Q)
    S = gp.matmul(Q, Y, transA=True)
    return Q, Y, (S + S.T) * 0.5


def single(gp, K, Q, shifts, y_ready, want_rr=True):
    return gp._basis_sweeps(K, Q, gp.matmul(K, Q) if y_ready else None, list(shifts), want_rr)


def assert_same(got, want, what):
    assert got is not None, what
    for name, x, y in zip("QYS", got, want):
        assert (x is None and y is None) or torch.equal(x, y), (what, name)


@pytest.mark.parametrize("y_ready", [False, True])
@pytest.mark.parametrize("m", [0, 1, 3])
@pytest.mark.parametrize("N,k", SHAPES)
def test_the_single_call_has_the_bits_of_the_host_loop(gp, N, k, m, y_ready):
    """m = 1: two rounds at once; m = 3: shifts [0, s1, s2], the non-zero ones pin the rounding of Y -= sigma Q; m = 0:
    the tail only."""
    K, Q0, shifts = problem(N, k)
    keep = Q0.clone()
    want = host_loop(gp, K, Q0, shifts[:m], y_ready, True)
    got = single(gp, K, Q0, shifts[:m], y_ready)
    assert_same(got, want, (N, k, m, y_ready))
    assert torch.equal(Q0, keep)                                 # the caller's block is left alone
    if m:
        assert not torch.equal(got[0], Q0)
    assert float((got[2] - got[2].T).abs().max()) == 0.0
    eye = torch.eye(k, dtype=torch.float64, device=K.device)
    assert float((gp.matmul(got[0], got[0], transA=True) - eye).abs().max()) < 1e-12


def test_a_shifted_first_step_on_a_ready_product_and_no_tail(gp):
    """The hand-over of a planned pass: Y = K Q is there and the FIRST step is shifted; and the call without the tail."""
    N, k = SHAPES[1]
    K, Q0, shifts = problem(N, k)
    order = (shifts[1], shifts[2])
    assert_same(single(gp, K, Q0, order, True), host_loop(gp, K, Q0, order, True, True), "shifted first step")
    got = single(gp, K, Q0, order, False, want_rr=False)
    want = host_loop(gp, K, Q0, order, False, False)
    assert got[2] is None and torch.equal(got[0], want[0])


def raw_group(gp, units, flags, engines=None):
    """gpfit_subspace_sweeps_batch through the C ABI on hand-built requests: the (step, info) pairs and the requests."""
    k = units[0]["Q"].shape[1]
    engines = engines or gp._group_engines(len(units), k, exact=True)
    qs = [gp._sweeps_prepare(engine=e, want_rr=bool(flags & WANT_RR), **u) for u, e in zip(units, engines)]
    assert all(q["flags"] == flags for q in qs)
    rc, rec = gp._sweeps_batch_raw([q["engine"]._ctx for q in qs], qs)
    assert rc == 0, _lib.last_error()
    return [(rec[2 * u], rec[2 * u + 1]) for u in range(len(qs))], qs


@pytest.mark.parametrize("y_ready", [False, True])
def test_every_unit_of_a_group_has_the_bits_of_its_single_call(gp, y_ready):
    """Three units at (384, 160) with m = (1, 3, 2): every step's launches carry only the units that still have it, the
    second round of a unit's last step only that unit."""
    N, k = SHAPES[1]
    ms = (1, 3, 2)
    probs = [problem(N, k, seed) for seed in range(3)]
    units = []
    for (K, Q0, shifts), m in zip(probs, ms):
        u = {"K": K, "Q": Q0, "shifts": list(shifts[:m])}
        if y_ready:
            u["Y"] = gp.matmul(K, Q0)
        units.append(u)
    group = gp._basis_sweeps_group(units)
    assert len(group) == 3
    for i, ((K, Q0, shifts), m) in enumerate(zip(probs, ms)):
        assert_same(group[i], single(gp, K, Q0, shifts[:m], y_ready), ("group", i))
    assert not torch.equal(group[0][0], group[1][0])
    # the same through the C ABI, with the records: every unit ran its own number of steps
    units = [dict(u, Y=gp.matmul(u["K"], u["Q"])) if y_ready else u for u in units]
    rec, qs = raw_group(gp, units, WANT_RR | (Y_READY if y_ready else 0))
    assert rec == [(1, 0), (3, 0), (2, 0)]
    for i, q in enumerate(qs):
        assert_same((q["Q"], q["Y"], q["S"]), group[i], ("raw group", i))


def test_a_unit_whose_gram_matrix_is_singular_stops_alone(gp):
    """Unit 1 starts from a block whose column 3 is zero: the Gram matrix of its first step has pivot 4 exactly zero.  It
    reports step 1 with info 4 and keeps its block; units 0 and 2 finish with the bits of their single calls."""
    N, k = SHAPES[1]
    probs = [problem(N, k, seed) for seed in range(3)]
    bad = probs[1][1].clone()
    bad[:, 3] = 0.0
    units = [{"K": K, "Q": bad if i == 1 else Q0, "shifts": list(shifts)} for i, (K, Q0, shifts) in enumerate(probs)]
    rec, qs = raw_group(gp, units, WANT_RR)
    assert rec == [(3, 0), (1, 4), (3, 0)]
    assert torch.equal(qs[1]["Q"], bad)                          # nothing of the failed step became visible
    for i in (0, 2):
        K, Q0, shifts = probs[i]
        assert_same((qs[i]["Q"], qs[i]["Y"], qs[i]["S"]), single(gp, K, Q0, shifts, False), ("beside a failure", i))
    # the wrapper: None in the unit's place; the single call: None
    group = gp._basis_sweeps_group(units)
    assert group[1] is None and group[0] is not None and group[2] is not None
    assert gp._basis_sweeps(probs[1][0], bad, None, list(probs[1][2]), True) is None
    # a unit alone, in a shifted step, with another column: pivot 6
    K, Q0, shifts = probs[1]
    sick = Q0.clone()
    sick[:, 5] = 0.0
    rec, qs = raw_group(gp, [{"K": K, "Q": sick, "shifts": [shifts[1]]}], WANT_RR)
    assert rec == [(1, 6)] and torch.equal(qs[0]["Q"], sick)


def test_the_refusals_of_the_entry_point(gp):
    N, k = SHAPES[0]
    K, Q0, shifts = problem(N, k)
    eng = gp.get_engine(k, 1)
    q = gp._sweeps_prepare(K, Q0, None, shifts, True, engine=eng)
    lib = _lib.load()
    rec = (ctypes.c_int * 4)()
    for what, word, over in (("the same context twice", "context of its own", {}), ("k no multiple of 16", "bad size", {"k": 40}),
                             ("k above N", "bad size", {"k": 176}), ("unknown flag", "unknown flag", {"flags": 7})):
        q2 = dict(q, **over)
        rc, _ = gp._sweeps_batch_raw([eng._ctx, eng._ctx] if not over else [eng._ctx], [q2, q2] if not over else [q2], rec)
        assert rc == -3 and "gpfit_subspace_sweeps_batch: " in _lib.last_error() and word in _lib.last_error(), (what, _lib.last_error())
    # two faults in one call -- unit 1 has more steps than a call takes (the one size a unit has of its own), unit 2 is on
    # unit 0's context: the units are checked in order
    other = gp._group_engines(2, k)[1]
    rec6 = (ctypes.c_int * 6)()
    rc, _ = gp._sweeps_batch_raw([eng._ctx, other._ctx, eng._ctx], [q, dict(q, shifts=[0.0] * 1025), q], rec6)
    assert rc == -3 and "gpfit_subspace_sweeps_batch: unit 1: m = 1025 is not within 0 .. 1024" in _lib.last_error(), _lib.last_error()
    small = gp.GPFitEngine(128, 1, 1, device=eng.device)
    N2, k2 = SHAPES[2]
    K2, Q2, s2 = problem(N2, k2)
    rc, _ = gp._sweeps_batch_raw([small._ctx], [gp._sweeps_prepare(K2, Q2, None, s2, True, engine=small)], rec)
    assert rc == -3 and "capacity" in _lib.last_error()
    assert lib.gpfit_subspace_sweeps(eng._ctx, gp._stream(), K.data_ptr(), N, N, k, Q0.data_ptr(), None, None, None, 0, None, 0,
                                     rec) == -3


def test_top_eigenpairs_with_the_switch_on_and_off(gp):
    """N = 384, k0 = 128 on a matrix with a clear gap at the threshold: the same B, K_tilde_b and count, bit for bit, and
    the same counters; the chain was really called."""
    n, tol = 384, 1e-4
    g = torch.Generator().manual_seed(3)
    Qm, _ = torch.linalg.qr(torch.randn(n, n, dtype=torch.float64, generator=g))
    lam = torch.cat([torch.logspace(2, 0, 60, dtype=torch.float64), torch.logspace(-4, -6, n - 60, dtype=torch.float64)])
    K = (Qm * lam) @ Qm.T
    K = ((K + K.T) / 2).cuda().contiguous()
    calls = []

    def chain(*a):
        calls.append(len(a[3]))
        return gp._basis_sweeps(*a)
    kw = dict(k0=128, basis="subspace", gemm_into=gp.gemm_into)
    off = eigtop.top_eigenpairs(K, tol, gp.matmul, gp.cholesky, **kw)
    on = eigtop.top_eigenpairs(K, tol, gp.matmul, gp.cholesky, sweep_chain=chain, **kw)
    assert off is not None and on is not None and off[0] is None and on[0] is None
    assert calls and sum(calls) >= 2
    assert on[2]["n"] == off[2]["n"] == 60
    assert torch.equal(on[1], off[1]) and torch.equal(on[2]["K_tilde_b"], off[2]["K_tilde_b"])
    assert torch.equal(on[2]["K_tilde_inv_b"], off[2]["K_tilde_inv_b"])
    for key in ("sweeps", "products", "k", "grown", "rr"):
        assert on[2][key] == off[2][key], key
    assert torch.equal(on[2]["state"]["Q"], off[2]["state"]["Q"])
    # warm, from the state of the first solve
    K2 = (K * (1 + 1e-5)).contiguous()
    off2 = eigtop.top_eigenpairs(K2, tol, gp.matmul, gp.cholesky, start=off[2]["state"], **kw)
    on2 = eigtop.top_eigenpairs(K2, tol, gp.matmul, gp.cholesky, start=on[2]["state"], sweep_chain=chain, **kw)
    assert on2[2]["warm"] and torch.equal(on2[1], off2[1]) and on2[2]["sweeps"] == off2[2]["sweeps"]


def test_one_fit_with_the_switch_on_and_off(gp, monkeypatch):
    """varGP at N = 2048, d = 64, the reference's default tolerance, three EM iterations: the same loss track, m_b, V_b,
    kept counts and routes, bit for bit."""
    N, d = 2048, 64
    X = T(syn.stimuli(N, d))
    r = T(syn.cell_inputs(N, 3)[0])
    used = []
    real = gp._basis_sweeps
    monkeypatch.setattr(gp, "_basis_sweeps", lambda *a: used.append(len(a[3])) or real(*a))

    def run(on):
        monkeypatch.setattr(gp, "SWEEP_CHAIN", on)
        th = {k: torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for k, v in syn.theta0(3).items()}
        fp = {"ntilde": N, "maxiter": 3, "nEstep": 2, "nMstep": 4, "nFparamstep": 3, "kernfun": "acosker", "cellid": 0,
              "n_px_side": 8, "display_hyper": False}
        args = {"fit_parameters": fp, "xtilde": X, "hyperparams_tuple": (th, LOWER, UPPER),
                "f_params": {"logA": torch.tensor(syn.F_PARAMS["logA"], dtype=torch.float64, requires_grad=True),
                             "lambda0": torch.tensor(syn.F_PARAMS["lambda0"], dtype=torch.float64)}}
        gp._BASIS.__dict__.pop("regime", None)
        with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fit, err = gp.varGP(X, r, **args)
        assert not err["is_error"], err
        return fit

    a = run(True)
    n_on = len(used)
    b = run(False)
    assert n_on >= 2 and len(used) == n_on                       # the chain ran in the rebuilds of the first fit only
    va, vb = a["values_track"], b["values_track"]
    for key in va["loss_track"]:
        assert torch.equal(torch.as_tensor(va["loss_track"][key]), torch.as_tensor(vb["loss_track"][key])), key
    assert va["variation_par_track"]["basis_route"] == vb["variation_par_track"]["basis_route"]
    assert set(va["variation_par_track"]["basis_route"]) == {"subspace"} and a["basis_route"] == b["basis_route"]
    for key in ("m_b", "V_b"):
        assert torch.equal(a[key], b[key]), key
        for x, y in zip(va["variation_par_track"][key], vb["variation_par_track"][key]):
            assert torch.equal(x, y), key
    assert a["B"].shape == b["B"].shape and torch.equal(a["B"], b["B"]) and 0 < a["B"].shape[1] < 1024
