"""gpfit_fit_eval_projected_batch (the truncated-rank M-step closures of several independent units as one device call) on
the GPU: every unit against gpfit_fit_eval_projected on that unit alone on the same context, bit for bit; the reference;
a failing unit stops alone; the refusals; and varGP_cells, whose truncated closures now meet like its chains, against the
same fits run one after another."""
import contextlib
import copy
import ctypes
import functools
import io
import math
import threading
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden
from gaussian_processes_amd import _lib, synthetic as syn

pytestmark = pytest.mark.gpu
KEYS = syn.THETA_KEYS
LOWER, UPPER = syn.limits()
N_PX = 8                # an 8 x 8 pixel grid
# (N, capacity of the contexts, n_kept per unit).  np = round_up(N, 128), nb = round_up(n_kept, 128), cap the contexts'.
#   200 / 256 / nb = 128: one leaf; 2 nb np = 65536 <= cap^2: the concatenated lift
#   200 / 256 / nb = 256: 2 nb np = 131072 > cap^2: the plain product plus symmetrize_avg; ragged n_kept under one padded size
#   600 / 1024 / nb = 384: the uneven 256 + 128 recursion split; k = 640 >= 512 and a scratch of 1024^2, so both
#   projections are cut into k slabs (and 2 nb np <= cap^2: the concatenated lift again)
SHAPES = [(200, 256, (70, 101, 120)), (200, 256, (130, 199, 180)), (600, 1024, (300, 257, 384))]
# The slabs of a projection are min(splitk_for, what the context's scratch holds) (fit.hip: gemm_splitk_list) and the route
# of the lift depends on the capacity too, so a closure's bits depend on the capacity of the context it runs on -- for the
# single call as for a unit of a group.  Every comparison below runs the single call on the context the unit had in the
# group.
# -2log2beta per unit: the first keeps every pixel, the others mask the corners of the grid, each a different number
LOGBETA = (-2.0 * math.log(1.2), 1.3, 1.9)
JOIN_S = 300            # a fit thread still alive after this is a deadlock: the test fails instead of hanging
SENTINEL = -12345.0
TILE = 128


@pytest.fixture(scope="module")
def gp():
    from gaussian_processes_amd import utils
    return utils


def T(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).cuda()


def tth(vec):
    return {k: torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for k, v in zip(KEYS, vec)}


def fparams(logA, lambda0):
    return {"logA": torch.tensor(float(logA), dtype=torch.float64), "lambda0": torch.tensor(float(lambda0), dtype=torch.float64)}


@functools.lru_cache(maxsize=None)
def stimuli(N):
    return T(syn.stimuli(N, N_PX * N_PX, seed=N))


@functools.lru_cache(maxsize=None)
def unit(N, nk, i, bad_V=False):
    """The arguments of _closure_projected for unit i of a shape, from seeds: an orthonormal basis of nk columns, an SPD V_b
    (bad_V: one eigenvalue negative), a theta, r, m_b, logA and lambda0 of its own.  Computed once, never written."""
    rng = np.random.default_rng(1000 * N + 10 * nk + i)
    B = T(np.linalg.qr(rng.standard_normal((N, nk)))[0])
    Q = np.linalg.qr(rng.standard_normal((nk, nk)))[0]
    ev = 0.05 + rng.random(nk)
    if bad_V:
        ev[nk // 2] = -0.1
    V_b = T((Q * ev) @ Q.T)
    V_b = ((V_b + V_b.T) * 0.5).contiguous()
    th = dict(syn.theta_eval())
    th["-2log2beta"] = LOGBETA[i % 3]
    th["eps_0x"] += 0.03 * i
    th["Amp"] *= 1.0 + 0.02 * i
    return {"theta": tth([th[k] for k in KEYS]), "lims": (LOWER, UPPER), "n_px_side": N_PX, "x": stimuli(N),
            "r": T(rng.poisson(0.7, N).astype(np.float64)), "B": B, "m_b": T(0.1 * rng.standard_normal(nk)), "V_b": V_b,
            "f_params": fparams(math.log(0.05) + 0.05 * i, -0.3 - 0.02 * i)}


_ENGINES = {}


def engines_for(gp, count, cap):
    """`count` contexts created for exactly `cap` stimuli (kept for the module: a context is created once)."""
    have = _ENGINES.setdefault(cap, [])
    while len(have) < count:
        have.append(gp.GPFitEngine(cap, N_PX * N_PX, N_PX * N_PX, device=torch.cuda.current_device()))
    return have[:count]


def requests(gp, units, engines):
    return [gp._closure_projected_prepare(engine=e, **u) for u, e in zip(units, engines)]


def batch(gp, units, engines, ctxs=None):
    """gpfit_fit_eval_projected_batch on the units: (return code, out[16] per unit, rc per unit)."""
    qs = requests(gp, units, engines)
    rc, out, rcs = gp._closure_projected_batch_raw(ctxs or [e._ctx for e in engines], qs)
    return rc, [list(out[16 * u:16 * u + 16]) for u in range(len(units))], [int(v) for v in rcs]


_SINGLES = {}


def single(gp, u, tag, eng):
    """gpfit_fit_eval_projected on the unit alone, on the context `eng`: (rc, out[16]); computed once per (tag, context)."""
    key = (tag, eng._ctx.value if hasattr(eng._ctx, "value") else eng._ctx)
    if key not in _SINGLES:
        _SINGLES[key] = gp._closure_projected_run_single(gp._closure_projected_prepare(engine=eng, **u))
    return _SINGLES[key]


def same(x, y):
    """Lists of floats equal entry by entry, NaN equal to NaN."""
    return len(x) == len(y) and all(p == q or (math.isnan(p) and math.isnan(q)) for p, q in zip(x, y))


def round_up(a, b):
    return -(-a // b) * b


def slabs(M, Nc, K, ld, cap):
    """fit.hip's splitk_for / gemm_splitk_list for an M x Nc x K product whose output has leading dimension ld, on a
    context of capacity cap."""
    tiles = (-(-M // TILE)) * (-(-Nc // TILE))
    if tiles >= 384:
        return 1
    sp = max(1, min(-(-768 // tiles), max(1, K // 256)))
    return max(1, min(sp, (cap * cap) // (M * ld)))


# ---------------------------------------------------------------------------------------------- the C entry point
@pytest.mark.parametrize("N,cap,nks", SHAPES)
def test_every_unit_has_the_bits_of_its_single_closure(gp, N, cap, nks):
    units = [unit(N, nk, i) for i, nk in enumerate(nks)]
    engines = engines_for(gp, 3, cap)
    assert all(round_up(e.n_max, TILE) == cap for e in engines)
    np_, nb = round_up(N, TILE), round_up(nks[0], TILE)
    assert all(round_up(nk, TILE) == nb for nk in nks)
    concatenated = 2 * nb * np_ <= cap * cap
    assert concatenated == (nks != SHAPES[1][2]), "the second shape alone takes the plain product and symmetrize_avg"
    cut = (slabs(np_, nb, np_, nb, cap), slabs(nb, nb, np_, nb, cap))
    if N == 600:
        assert cut[0] >= 2 and cut[1] >= 2, cut          # both projections really are cut into k slabs
    rc, outs, rcs = batch(gp, units, engines)
    assert rc == 0 and rcs == [0, 0, 0], (rc, rcs, _lib.last_error())
    for i, u in enumerate(units):
        rc1, want = single(gp, u, (N, nks[i], i), engines[i])
        assert rc1 == 0, (i, _lib.last_error())
        assert all(math.isfinite(v) for v in want), (i, want)
        assert same(outs[i], want), (N, nks, i, outs[i], want)
    assert len({o[0] for o in outs}) == 3, [o[0] for o in outs]          # the units really are different
    assert len({o[13] for o in outs}) == 3, [o[13] for o in outs]        # ... with different masked pixel counts


def test_sixteen_units_and_a_group_of_one(gp):
    N, cap, _ = SHAPES[0]
    nks = [70 + (50 * i) // 15 for i in range(16)]            # 70 .. 120 under one padded size
    assert nks[0] == 70 and nks[-1] == 120
    units = [unit(N, nk, i) for i, nk in enumerate(nks)]
    engines = engines_for(gp, 16, cap)
    rc, outs, rcs = batch(gp, units, engines)
    assert rc == 0 and rcs == [0] * 16, (rc, rcs, _lib.last_error())
    for i in range(16):
        rc1, want = single(gp, units[i], (N, nks[i], i), engines[i])
        assert rc1 == 0 and same(outs[i], want), ("16 units", i, outs[i], want)
    rc, one, rcs = batch(gp, units[3:4], engines[3:4])
    assert rc == 0 and rcs == [0]
    assert same(one[0], single(gp, units[3], (N, nks[3], 3), engines[3])[1]), "one unit against the single call"
    assert same(one[0], outs[3]), "one unit against the same unit in the group of 16"


def test_group_against_the_fixture(gp):
    """g3_closure_trunc_N96_d16 (72 of 96 kept) is the middle unit of three, the other two with theta and r perturbed: its
    loss and gradient meet the reference's within the bounds of test_gpu_dropin.test_projected_adjoint_closure_matches_reference
    for the same fixture (1e-9 on the loss, 1e-7 on the gradients)."""
    g = load_golden("g3_closure_trunc_N96_d16.npz")
    X, B, m_b, V_b = T(g["X"]), T(g["B"]), T(g["m_b"]), T(g["V_b"])
    assert B.shape == (96, 72)
    n_px = int(g["n_px"])
    rng = np.random.default_rng(11)
    logA, lam0 = float(g["logA"]), float(g["lambda0"])
    units = []
    for i in range(3):
        th = np.array(g["theta"], dtype=np.float64)
        r = np.array(g["r"], dtype=np.float64)
        if i != 1:
            th = th + 0.03 * (i + 1) * rng.standard_normal(6) * np.array([1, 0.3, 0.3, 1, 1, 1])
            r = rng.poisson(np.maximum(r.mean(), 0.2), r.shape).astype(np.float64)
        units.append({"theta": tth(th), "lims": (LOWER, UPPER), "n_px_side": n_px, "x": X, "r": T(r), "B": B, "m_b": m_b,
                      "V_b": V_b, "f_params": fparams(logA, lam0)})
    engines = [gp.GPFitEngine(96, X.shape[1], n_px * n_px, device=torch.cuda.current_device()) for _ in range(3)]
    rc, outs, rcs = batch(gp, units, engines)
    assert rc == 0 and rcs == [0, 0, 0], (rc, rcs, _lib.last_error())
    d_loss = abs(outs[1][0] - float(g["loss"])) / abs(float(g["loss"]))
    d_grad = np.abs(np.array(outs[1][3:9]) - g["grad"]).max() / np.abs(g["grad"]).max()
    print(f"the fixture's unit in a group of three: loss {d_loss:.2e}, grad {d_grad:.2e}")
    assert d_loss <= 1e-9 and d_grad <= 1e-7, (d_loss, d_grad)
    assert len({o[0] for o in outs}) == 3
    assert same(outs[1], gp._closure_projected_run_single(requests(gp, units[1:2], engines[1:2])[0])[1])
    for e in engines:
        e.close()


def forget_workspaces(gp):
    """Drop the workspaces varGP_cells keeps and those the pool still holds for host threads that have ended (a new
    thread that gets such a thread's ident would inherit its workspace): the fits below then all run on workspaces
    created for their own N -- a closure's last bits depend on the capacity of its workspace (slab counts, the lift)."""
    gp.release_cell_workspaces()
    alive = {t.ident for t in threading.enumerate()}
    with gp._POOL.lock:
        for k in [k for k in gp._POOL.eng if k[1] not in alive or k[1] == threading.get_ident()]:
            del gp._POOL.eng[k]


def in_a_thread(fn, gp=None):
    """fn() in a fresh host thread, joined with a bound: its result, or its exception re-raised here.  gp: the thread
    starts without an inherited workspace (forget_workspaces)."""
    box = {}

    def body():
        try:
            if gp is not None:
                forget_workspaces(gp)
            with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                box["out"] = fn()
        except BaseException as err:
            box["err"] = err
    t = threading.Thread(target=body, daemon=True)
    t.start()
    t.join(JOIN_S)
    assert not t.is_alive(), "the fit thread is still running: a fit waits for one that will never arrive"
    if "err" in box:
        raise box["err"]
    return box["out"]


def outcome(fn):
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")
        try:
            return fn()
        except Exception as err:
            return err


def same_outcome(a, b):
    if isinstance(a, Exception) or isinstance(b, Exception):
        return type(a) is type(b) and str(a) == str(b)
    return same([a[0]] + [a[1][k] for k in KEYS], [b[0]] + [b[1][k] for k in KEYS])


def test_a_unit_whose_factorisation_fails_stops_alone(gp):
    N, cap, _ = SHAPES[0]
    units = [unit(N, 101, 0), unit(N, 101, 1, bad_V=True), unit(N, 120, 2)]
    engines = engines_for(gp, 3, cap)
    rc, outs, rcs = batch(gp, units, engines)
    assert rc == 0, _lib.last_error()
    assert rcs[1] > 0 and outs[1][15] != 0 and rcs[0] == 0 and rcs[2] == 0, (rcs, outs[1])
    assert rcs[1] == single(gp, units[1], "bad V", engines[1])[0]
    for i, tag in ((0, (N, 101, 0)), (2, (N, 120, 2))):
        assert same(outs[i], single(gp, units[i], tag, engines[i])[1]), i
    # through the Python layer: the failing unit takes the step-by-step formulation, alone.  (In a fresh host thread: its
    # workspace is created for these N stimuli, the capacity the group's workspaces have.)
    group, alone, steps = in_a_thread(lambda: (outcome(lambda: gp._closure_projected_group(units)),
                                               [outcome(lambda: gp._closure_projected(**u)) for u in units],
                                               outcome(lambda: gp._closure_projected_steps(**units[1]))), gp)
    assert not isinstance(group, Exception), group
    for i in range(3):
        assert same_outcome(group[i], alone[i]), (i, group[i], alone[i])
    assert not isinstance(steps, Exception) and same_outcome(group[1], steps), (group[1], steps)
    assert not isinstance(group[0], Exception) and math.isfinite(group[0][0])


def test_a_unit_outside_its_limits_gets_the_infinite_loss_alone(gp):
    N, cap, _ = SHAPES[0]
    out_of_box = dict(unit(N, 101, 1))
    th = [float(v.detach()) for v in out_of_box["theta"].values()]
    th[1] = 1.5                                              # eps_0x above its upper limit of 1
    out_of_box["theta"] = tth(th)
    units = [unit(N, 101, 0), out_of_box, unit(N, 120, 2)]
    engines = engines_for(gp, 3, cap)
    rc, outs, rcs = batch(gp, units, engines)
    assert rc == 0 and rcs == [0, -2, 0], (rc, rcs, _lib.last_error())
    assert outs[1][0] == math.inf and all(v == math.inf for v in outs[1][3:9]), outs[1]
    for i, tag in ((0, (N, 101, 0)), (2, (N, 120, 2))):
        assert same(outs[i], single(gp, units[i], tag, engines[i])[1]), i
    group, alone = in_a_thread(lambda: (outcome(lambda: gp._closure_projected_group(units)),
                                        [outcome(lambda: gp._closure_projected(**u)) for u in units]), gp)
    assert isinstance(alone[1], ValueError) and "eps_0x" in str(alone[1]), alone[1]
    for i in range(3):
        assert same_outcome(group[i], alone[i]), (i, group[i], alone[i])


def test_refusals_enqueue_nothing(gp):
    """0 and 17 units, a null operand, a repeated context, n_kept > N, a leading dimension below n_kept, mixed padded sizes
    and mixed capacities: a return value below 0 with a message naming the cause, and neither out_host nor rc_out changes."""
    N, cap, nks = SHAPES[1]
    engines = engines_for(gp, 3, cap)
    good = [unit(N, nk, i) for i, nk in enumerate(nks)]

    def raw(ctxs, qs, nu=None):
        n = max(len(qs), 1)
        out = (ctypes.c_double * (16 * n))(*([SENTINEL] * (16 * n)))
        rcs = (ctypes.c_int * n)(*([77] * n))
        if nu == 0:      # the arrays of one unit, n_units = 0
            vp1, i641 = ctypes.c_void_p * 1, ctypes.c_int64 * 1
            q = qs[0]
            rc = _lib.load().gpfit_fit_eval_projected_batch(
                vp1(ctxs[0].value if isinstance(ctxs[0], ctypes.c_void_p) else ctxs[0]), 0, q["stream"], _lib.darr(q["theta"]),
                _lib.darr(q["lower"]), _lib.darr(q["upper"]), q["rows"], q["cols"], vp1(q["x"].data_ptr()), q["x"].stride(0), q["N"],
                vp1(q["r"].data_ptr()), vp1(q["B"].data_ptr()), i641(q["B"].stride(0)), i641(q["n_kept"]), vp1(q["m_b"].data_ptr()),
                vp1(q["V_b"].data_ptr()), i641(q["V_b"].stride(0)), _lib.darr([q["logA"]]), _lib.darr([q["lambda0"]]), out, rcs)
        else:
            rc, _, _ = gp._closure_projected_batch_raw(ctxs, qs, out, rcs)
        return rc, list(out), list(rcs)

    def refused(ctxs, qs, word, nu=None):
        rc, out, rcs = raw(ctxs, qs, nu)
        assert rc < 0, (word, rc)
        assert word in _lib.last_error(), (word, _lib.last_error())
        assert all(v == SENTINEL for v in out) and all(v == 77 for v in rcs), word

    ctxs = [e._ctx for e in engines]
    qs = requests(gp, good, engines)
    refused(ctxs[:1], qs[:1], "units per call", nu=0)
    refused((ctxs * 6)[:17], (qs * 6)[:17], "units per call")
    qs = requests(gp, good, engines)
    qs[1]["m_b"] = None
    refused(ctxs, qs, "null")
    refused([ctxs[0], ctxs[1], ctxs[0]], requests(gp, good, engines), "context of its own")
    qs = requests(gp, good, engines)
    qs[2]["n_kept"] = N + 1
    refused(ctxs, qs, "n_kept")

    class Narrow:      # B with a leading dimension below n_kept
        def __init__(self, t, ld):
            self.t, self.ld = t, ld

        def data_ptr(self):
            return self.t.data_ptr()

        def stride(self, i):
            return self.ld
    qs = requests(gp, good, engines)
    qs[1]["B"] = Narrow(qs[1]["B"], qs[1]["n_kept"] - 1)
    refused(ctxs, qs, "leading dimension")
    # two faults in one call -- that leading dimension of unit 1, unit 2 on unit 0's context: the units are checked in order
    refused([ctxs[0], ctxs[1], ctxs[0]], qs, "gpfit_fit_eval_projected_batch: unit 1: bad leading dimension")
    refused(ctxs, requests(gp, [good[0], unit(N, 100, 1), good[2]], engines), "round_up(n_kept, 128)")
    large = engines_for(gp, 1, 1024)[0]
    refused([ctxs[0], ctxs[1], large._ctx], requests(gp, good, engines), "capacity")
    # and the same three units are accepted as they are
    rc, out, rcs = raw(ctxs, requests(gp, good, engines))
    assert rc == 0 and rcs == [0, 0, 0], (_lib.last_error(), rcs)
    assert all(v != SENTINEL and math.isfinite(v) for v in out)


# ---------------------------------------------------------------------------------------------- varGP_cells
def vargp_args(g, X, ntilde, **fit_kwargs):
    fit_parameters = {"ntilde": ntilde, "maxiter": int(g["maxiter"]), "nEstep": int(g["nEstep"]), "nMstep": int(g["nMstep"]),
                      "nFparamstep": int(g["nFparamstep"]), "kernfun": "acosker", "cellid": 0, "n_px_side": 8,
                      "display_hyper": False}
    fit_parameters.update(fit_kwargs)
    theta = {k: torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for k, v in zip(KEYS, g["theta0"])}
    f_params = {"logA": syn.F_PARAMS["logA"], "lambda0": syn.F_PARAMS["lambda0"]}
    return {"fit_parameters": fit_parameters, "xtilde": X[:ntilde].clone(), "hyperparams_tuple": (theta, LOWER, UPPER),
            "f_params": {k: torch.tensor(float(v), dtype=torch.float64) for k, v in f_params.items()}}


def assert_same_fit(a, b, what):
    (fit, err), (fit1, err1) = a, b
    assert err["is_error"] == err1["is_error"], what
    for group in ("loss_track", "theta_track", "f_par_track"):
        for k, v in fit["values_track"][group].items():
            assert torch.equal(v, fit1["values_track"][group][k]), (what, group, k)
    for k in ("m_b", "V_b"):
        assert torch.equal(fit[k], fit1[k]), (what, k)
    for k in KEYS:
        assert float(fit["hyperparams_tuple"][0][k]) == float(fit1["hyperparams_tuple"][0][k]), (what, k)
    assert fit["f_params"].keys() == fit1["f_params"].keys()
    for k in fit["f_params"]:
        x, y = float(fit["f_params"][k]), float(fit1["f_params"][k])
        assert x == y or (math.isnan(x) and math.isnan(y)), (what, k, x, y)


def count_prepares(gp, monkeypatch, name):
    calls = [0]
    prepare = getattr(gp, name)

    def counting(*a, **k):
        calls[0] += 1
        return prepare(*a, **k)
    monkeypatch.setattr(gp, name, counting)
    return calls


def test_vargp_cells_truncated_closures_meet_and_every_fit_is_vargp_alone(gp, monkeypatch):
    """Three cells with ntilde == ntrain at the shape and tolerance of g6_vargp_trunc_N128 (cell 0 is the fixture's): the
    fits truncate, every fit has the bits of varGP on that cell alone, and the closures went out as calls of up to 3
    units -- as many unit-calls as the three fits make closure device calls alone."""
    g = load_golden("g6_vargp_trunc_N128.npz")
    X = T(g["X"])
    N = int(X.shape[0])
    rng = np.random.default_rng(17)
    rs = [T(g["r"])] + [T(rng.poisson(np.maximum(g["r"].mean(), 0.2), g["r"].shape).astype(np.float64)) for _ in range(2)]
    monkeypatch.setattr(gp, "EIGVAL_TOL", float(g["tol"]))
    kwargs = [vargp_args(g, X, N) for _ in rs]
    cells = in_a_thread(lambda: gp.varGP_cells(X, rs, copy.deepcopy(kwargs)), gp)   # workspaces of this size: one bucket
    closure_sizes = list(gp.varGP_cells.last_closure_group_sizes)
    assert len(gp.varGP_cells.last_closure_call_seconds) == len(closure_sizes)
    assert len(cells) == 3 and all(not err["is_error"] for _, err in cells)
    assert all(fit["B"].shape[1] < N for fit, _ in cells), "the fits are in the truncated regime"
    assert cells[0][0]["B"].shape[1] == int(g["n_kept"])
    assert 3 in closure_sizes and all(1 <= n <= 3 for n in closure_sizes), closure_sizes
    calls = count_prepares(gp, monkeypatch, "_closure_projected_prepare")
    for i, r in enumerate(rs):
        alone = in_a_thread(lambda: gp.varGP(X, r, **copy.deepcopy(kwargs[i])), gp)
        assert not alone[1]["is_error"], alone[1]
        assert_same_fit(cells[i], alone, i)
    print(f"closure calls by units carried: {closure_sizes}; device calls of the three fits alone: {calls[0]}")
    assert calls[0] > 0 and sum(closure_sizes) == calls[0], (closure_sizes, calls[0])


def test_a_wave_of_a_truncated_and_a_sparse_fit_never_mixes_regimes(gp, monkeypatch):
    """One fit with ntilde == ntrain (truncated) and one with ntilde < ntrain (sparse) in one wave, on the stimuli and at
    the tolerance of g6_vargp_trunc_N128: the wave ends, both fits have the bits of their own varGP, both regimes asked
    closures, and every closure call carried one unit."""
    g = load_golden("g6_vargp_trunc_N128.npz")
    X = T(g["X"])
    N = int(X.shape[0])
    ntilde = N // 2
    r = T(g["r"])
    monkeypatch.setattr(gp, "EIGVAL_TOL", float(g["tol"]))
    kwargs = [vargp_args(g, X, N), vargp_args(g, X, ntilde)]
    trunc = count_prepares(gp, monkeypatch, "_closure_projected_prepare")
    sparse = count_prepares(gp, monkeypatch, "_closure_sparse_prepare")
    cells = in_a_thread(lambda: gp.varGP_cells(X, [r, r], copy.deepcopy(kwargs)), gp)
    closure_sizes = list(gp.varGP_cells.last_closure_group_sizes)
    print(f"closure calls of a truncated and a sparse fit in one wave: {closure_sizes}; {trunc[0]} truncated, {sparse[0]} sparse")
    assert [err["is_error"] for _, err in cells] == [False, False]
    assert cells[0][0]["B"].shape[1] < N and cells[1][0]["B"].shape[0] == ntilde
    assert trunc[0] > 0 and sparse[0] > 0
    assert closure_sizes and all(n == 1 for n in closure_sizes), closure_sizes
    assert len(closure_sizes) == trunc[0] + sparse[0]
    for i in range(2):
        alone = in_a_thread(lambda: gp.varGP(X, r, **copy.deepcopy(kwargs[i])), gp)
        assert_same_fit(cells[i], alone, i)
