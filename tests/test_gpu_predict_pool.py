"""Scoring a stimulus pool in one device call (gpfit_score_pool through utils.fold_posterior, pool_moments and score_pool)
against the long-double restatement of lambda_moments_star (predict_cases.reference) and against today's composition
(lambda_moments_star, nd_utility) on the same inputs; the lower-triangle convention of S, exactness across chunk sizes,
row offsets, repeats and the mask path; rate and utility; stale workspace; refusals.

Shapes (P, nt, k, px), the smallest at which each mechanism can fail: predict_cases.CASES.

Accuracy bound: the error of the new form may be at most ten times that of lambda_moments_star on the same inputs (both
against long double, relative to max |.|, floored at 1e-15).  The two forms share the leading error term
eps |z|^2 |K~^-1|^2 |V - K~| and differ in association and summation order only; the numpy restatement shows them equal
to two digits (test_predict_cases_cpu.py), and one decade is the room for the device's summation order over up to 384
terms."""
import contextlib
import ctypes
import functools
import io
import warnings

import numpy as np
import pytest
import torch

import predict_cases as cases
from conftest import load_golden, relerr
from gaussian_processes_amd import synthetic as syn

pytestmark = pytest.mark.gpu
KEYS = syn.THETA_KEYS
LOWER, UPPER = syn.limits()
EPS = float(np.finfo(np.float64).eps)
SENTINEL = -12345.0
WORK_MATRICES = (b"Abuf", b"Tbuf", b"Wbuf", b"Zbuf", b"Cos", b"TmpV")
IDS = lambda s: "P{}-nt{}-k{}-px{}".format(*s)  # noqa: E731


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
def link():
    return {"logA": torch.tensor(syn.F_PARAMS["logA"], dtype=torch.float64),
            "lambda0": torch.tensor(syn.F_PARAMS["lambda0"], dtype=torch.float64)}


@pytest.fixture(scope="module")
def counts():
    return torch.arange(0, 100, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _unit(shape):
    """The case on the device (shared between the tests, never written): masked stimuli, the posterior and its fold."""
    from gaussian_processes_amd import utils as gp
    c = cases.make_case(*shape)
    mask = torch.from_numpy(c["mask"]).cuda()
    u = {k: T(c[k]) for k in ("C", "K", "Kinv", "m", "V")}
    u["xs_full"], u["xt_full"], u["mask"] = T(c["xstar"]), T(c["xtilde"]), mask
    u["xs"], u["xt"] = u["xs_full"][:, mask].contiguous(), u["xt_full"][:, mask].contiguous()
    u["B"] = gp._mark_identity(torch.eye(c["nt"], dtype=torch.float64, device="cuda")) if c["B"] is None else T(c["B"])
    u["theta"] = c["theta"]
    u["folded"] = gp.fold_posterior(u["K"], u["Kinv"], u["m"], u["V"], u["B"])
    return u


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def raw(lib, ctx, u, S=None, r=None, chunk_rows=0, A=1.0, lambda0=0.0, U=None):
    """gpfit_score_pool itself on the masked inputs of a unit: (rc, mu, sigma2, rate, U); U starts as the sentinel."""
    f = u["folded"]
    S = f["S"] if S is None else S
    B = f["B"]
    P, nt, d = u["xs"].shape[0], u["xt"].shape[0], u["xs"].shape[1]
    mu, s2, rate = (torch.full((P,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(3))
    U = torch.full((P,), SENTINEL, dtype=torch.float64, device="cuda") if U is None else U
    rc = lib.gpfit_score_pool(ctx, _stream(), float(u["theta"]["sigma_0"]), u["xs"].data_ptr(), u["xs"].stride(0), P, None, d,
                              u["xt"].data_ptr(), u["xt"].stride(0), nt, d, u["C"].data_ptr(), u["C"].stride(0),
                              B.data_ptr() if B is not None else None, B.stride(0) if B is not None else 0, f["k"],
                              S.data_ptr(), S.stride(0), f["w"].data_ptr(), A, lambda0,
                              r.data_ptr() if r is not None else None, r.numel() if r is not None else 0, chunk_rows,
                              mu.data_ptr(), s2.data_ptr(), rate.data_ptr(), U.data_ptr())
    torch.cuda.synchronize()
    return rc, mu, s2, rate, U


# ------------------------------------------------------------------ 1. accuracy against the reference
@pytest.mark.parametrize("shape", cases.CASES, ids=IDS)
def test_moments_are_as_accurate_as_todays_composition(gp, shape):
    u = _unit(shape)
    mu_ref, s2_ref = cases.reference(*shape)
    mu, s2 = gp.pool_moments(u["xs"], u["xt"], u["C"], u["theta"], u["folded"])
    mu_o, s2_o = gp.lambda_moments_star(u["xs"], u["xt"], u["C"], u["theta"], u["K"], u["Kinv"], u["m"], u["V"], u["B"], "acosker")
    assert mu.shape == (shape[0],) and s2.shape == (shape[0],)
    e_new = (cases.err(mu.cpu().numpy(), mu_ref), cases.err(s2.cpu().numpy(), s2_ref))
    e_old = (cases.err(mu_o.reshape(-1).cpu().numpy(), mu_ref), cases.err(s2_o.reshape(-1).cpu().numpy(), s2_ref))
    print(f"\n{shape}: mu e_new {e_new[0]:.2e} e_old {e_old[0]:.2e} | sigma2 e_new {e_new[1]:.2e} e_old {e_old[1]:.2e}")
    assert e_new[0] <= 10 * max(e_old[0], 1e-15)
    assert e_new[1] <= 10 * max(e_old[1], 1e-15)


# ------------------------------------------------------------------ 2. the real reference
def test_predict_matches_golden(gp):
    """Fixture g5 (the real reference's lambda_moments_star), set up as test_gpu_dropin.test_predict_matches_golden does:
    the eigenbasis of K~ as B.  The tolerances are that test's."""
    g = load_golden("g5_predict_N64.npz")
    th = {k: torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for k, v in zip(KEYS, g["theta"])}
    C, mask = gp.localker(th, UPPER, LOWER, 8)
    X, Xs = T(g["X"])[:, mask].contiguous(), T(g["Xstar"])[:, mask].contiguous()
    Kt = gp.acosker(th, X, X, C=C)
    ev, evec = torch.linalg.eigh(Kt)
    m_b = gp.matmul(evec, T(g["m"]), transA=True)
    V_b = gp.matmul(evec, gp.matmul(T(g["V"]), evec), transA=True)
    folded = gp.fold_posterior(torch.diag(ev), torch.diag(1 / ev), m_b, V_b, evec)
    assert folded["B"] is not None and folded["k"] == 64
    mu, s2 = gp.pool_moments(Xs, X, C, th, folded)
    print(f"\ng5: mu {relerr(mu.cpu().numpy(), g['mu']):.2e} sigma2 {relerr(s2.cpu().numpy(), g['s2']):.2e}")
    assert relerr(mu.cpu().numpy(), g["mu"]) < 1e-9 and relerr(s2.cpu().numpy(), g["s2"]) < 1e-8
    # whole images with the mask, one row
    mu1, _ = gp.pool_moments(T(g["Xstar"])[2:3], X, C, th, folded, mask=mask)
    assert abs(float(mu1) - g["mu"][2]) < 1e-9 * abs(g["mu"][2])


# ------------------------------------------------------------------ 3. the lower triangle of S is canonical
@pytest.mark.parametrize("shape", [cases.CASES[1], cases.PROJECTED], ids=IDS)
def test_strict_upper_triangle_of_S_is_never_read(gp, lib, shape):
    u = _unit(shape)
    k = u["folded"]["k"]
    eng = gp.get_engine(max(shape[1], k), u["xs"].shape[1])
    S_nan = u["folded"]["S"].clone()
    S_nan[torch.triu(torch.ones(k, k, dtype=torch.bool, device="cuda"), diagonal=1)] = float("nan")
    rc0, mu0, s20, _, _ = raw(lib, eng._ctx, u)
    rc1, mu1, s21, _, _ = raw(lib, eng._ctx, u, S=S_nan)
    assert rc0 == 0 and rc1 == 0
    assert not torch.isnan(s20).any()
    assert same_bits(mu0, mu1) and same_bits(s20, s21)


# ------------------------------------------------------------------ 4. chunks, row offsets, repeats
def test_chunking_row_offset_and_repeats_do_not_change_a_bit(gp, link, counts):
    u = _unit(cases.CHUNKED)
    args = (u["xt"], u["C"], u["theta"], u["folded"], link)
    base = gp.score_pool(u["xs"], *args, r_masked=counts, chunk_rows=128)
    assert all(not torch.isnan(base[key]).any() for key in ("mu", "sigma2", "rate", "utility"))
    for chunk_rows in (256, 0, 128):       # 128 again: a repeated call
        other = gp.score_pool(u["xs"], *args, r_masked=counts, chunk_rows=chunk_rows)
        for key in ("mu", "sigma2", "rate", "utility"):
            assert same_bits(base[key], other[key]), (chunk_rows, key)
    alone = gp.score_pool(u["xs"][129:131].contiguous(), *args, r_masked=counts)
    for key in ("mu", "sigma2", "rate", "utility"):
        assert same_bits(base[key][129:131], alone[key]), key


def test_chunking_and_row_offset_with_a_basis(gp):
    """The same with the projected panel (130 rows: chunks of 128 + 2 against one chunk of 130, and row 129 alone)."""
    u = _unit(cases.PROJECTED)
    args = (u["xt"], u["C"], u["theta"], u["folded"])
    mu, s2 = gp.pool_moments(u["xs"], *args)
    mu_c, s2_c = gp.pool_moments(u["xs"], *args, chunk_rows=128)
    mu_1, s2_1 = gp.pool_moments(u["xs"][129:130].contiguous(), *args)
    assert same_bits(mu, mu_c) and same_bits(s2, s2_c)
    assert same_bits(mu[129:130], mu_1) and same_bits(s2[129:130], s2_1)


def test_chunking_with_a_basis_at_a_size_the_gemm_launcher_would_balance(gp):
    """nt = k = 1024 in a dense orthonormal basis, 8320 pool rows.  As an ordinary product the projection K* B of one chunk
    of 8320 rows is a launch of 65 x 8 = 520 whole tiles with K = 1024: the size from which the GEMM launcher puts the
    tail tiles (520 mod 512 = 8) on its stream-K schedule and cuts their k range, while chunks of 4096 or 128 rows stay
    data-parallel.  The call sends the product out so that no chunk is cut: one chunk, chunks of 4096 and of 128 rows and
    rows scored alone must agree bit for bit.  (Bit-equality needs no meaningful posterior: S, w random, B from a QR.)"""
    u = _unit(cases.CASES[1])
    P, nt = 8320, 1024
    g = torch.Generator(device="cpu").manual_seed(11)
    X = torch.randn(P + nt, 64, dtype=torch.float64, generator=g).cuda()
    xs, xt = X[:P].contiguous(), X[P:].contiguous()
    B = torch.linalg.qr(torch.randn(nt, nt, dtype=torch.float64, generator=g))[0].contiguous().cuda()
    S = torch.randn(nt, nt, dtype=torch.float64, generator=g)
    folded = {"S": (0.5 * (S + S.T) / nt).contiguous().cuda(), "w": (torch.randn(nt, dtype=torch.float64, generator=g) / nt).cuda(),
              "B": B, "k": nt}
    gp.reserve(P, 64)                      # chunk_rows = 0 is then one chunk of 8320 rows
    args = (xt, u["C"], u["theta"], folded)
    mu, s2 = gp.pool_moments(xs, *args)
    assert not torch.isnan(mu).any() and not torch.isnan(s2).any()
    for chunk_rows in (4096, 128):
        mu_c, s2_c = gp.pool_moments(xs, *args, chunk_rows=chunk_rows)
        assert same_bits(mu, mu_c) and same_bits(s2, s2_c), chunk_rows
    for lo, hi in ((8200, 8203), (0, 1), (8319, 8320)):
        mu_1, s2_1 = gp.pool_moments(xs[lo:hi].contiguous(), *args)
        assert same_bits(mu[lo:hi], mu_1) and same_bits(s2[lo:hi], s2_1), (lo, hi)


# ------------------------------------------------------------------ 5. the mask path
def test_whole_images_with_a_mask_equal_masked_images(gp, link, counts):
    """The metric's own mask keeps every pixel of these small images, so the test drops nine pixels more: 55 columns
    gathered out of 64 (C restricted to them is a metric like any other; S and w are inputs like any other)."""
    u = _unit(cases.CASES[1])
    keep = torch.ones(64, dtype=torch.bool)
    keep[torch.tensor([0, 5, 9, 17, 30, 31, 32, 50, 63])] = False
    keep = keep.cuda()
    Csub = u["C"][keep][:, keep].contiguous()
    xt = u["xt_full"][:, keep].contiguous()
    a = gp.score_pool(u["xs_full"][:, keep].contiguous(), xt, Csub, u["theta"], u["folded"], link, r_masked=counts)
    b = gp.score_pool(u["xs_full"], xt, Csub, u["theta"], u["folded"], link, r_masked=counts, mask=keep)
    c = gp.score_pool(u["xs_full"], u["xt_full"], Csub, u["theta"], u["folded"], link, r_masked=counts, mask=keep)
    full = gp.score_pool(u["xs"], u["xt"], u["C"], u["theta"], u["folded"], link, r_masked=counts)
    for key in ("mu", "sigma2", "rate", "utility"):
        assert same_bits(a[key], b[key]) and same_bits(a[key], c[key]), key
    assert not same_bits(a["sigma2"], full["sigma2"])      # the dropped pixels do matter


# ------------------------------------------------------------------ 6. rate and utility
@pytest.mark.parametrize("shape", [cases.CASES[1], cases.PROJECTED], ids=IDS)
def test_rate_and_utility_follow_the_calls_own_moments(gp, link, counts, shape):
    u = _unit(shape)
    out = gp.score_pool(u["xs"], u["xt"], u["C"], u["theta"], u["folded"], link, r_masked=counts)
    mu, s2 = out["mu"], out["sigma2"]
    m2, v2 = gp.pool_moments(u["xs"], u["xt"], u["C"], u["theta"], u["folded"])
    assert same_bits(mu, m2) and same_bits(s2, v2)
    A, lambda0 = torch.exp(link["logA"]), link["lambda0"]
    assert same_bits(out["utility"], gp.nd_utility(A ** 2 * s2, A * mu + lambda0, counts))
    arg = A * mu + 0.5 * A * A * s2 + lambda0
    want = torch.exp(arg)
    rel = (torch.abs(out["rate"] - want) / want).cpu().numpy()
    bound = 16 * EPS * np.maximum(1.0, np.abs(arg.cpu().numpy()))
    print(f"\n{shape}: rate, worst relative difference over its bound {float(np.max(rel / bound)):.3f}")
    assert np.all(rel <= bound)


def test_best_image_of_the_closed_loop_fixture(gp, counts):
    """First round of fixture g9 (test_gpu_dropin.test_closed_loop_step_matches_reference): the image of largest utility
    is the one today's composition picks, and the one the real reference picked."""
    g = load_golden("g9_active_step.npz")
    dev = torch.device("cuda")
    images, spikes = T(g["X"]), T(g["R"])
    n0, pool = int(g["n_start"]), int(g["X"].shape[0])
    settings = {"ntilde": n0, "maxiter": int(g["maxiter"]), "nEstep": 2, "nMstep": 3, "nFparamstep": 3, "kernfun": "acosker",
                "cellid": 0, "n_px_side": 8, "display_hyper": False}
    start_theta = {k: torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for k, v in syn.theta0().items()}
    fp = {"logA": torch.tensor(syn.F_PARAMS["logA"]), "lambda0": torch.tensor(syn.F_PARAMS["lambda0"])}
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        first, err = gp.varGP(images[:n0], spikes[:n0], fit_parameters=settings, xtilde=images[:n0],
                              hyperparams_tuple=(start_theta, LOWER, UPPER), f_params=fp)
    assert not err["is_error"], err
    rest = torch.arange(n0, pool, device=dev)
    th, px, C, basis = first["hyperparams_tuple"][0], first["mask"].to(dev), first["C"], first["B"]
    cand = images[rest][:, px].contiguous()
    k_self = gp.acosker(th, cand, x2=None, C=C, diag=True)
    k_cross = gp.matmul(gp.acosker(th, cand, images[:n0][:, px].contiguous(), C=C), basis)
    mean, var = gp.lambda_moments(cand, first["K_tilde_b"], gp.matmul(k_cross, first["K_tilde_inv_b"]), k_self, k_cross, C,
                                  first["m_b"], first["V_b"], th)
    gain_A = torch.exp(first["f_params"]["logA"]).to(dev)
    gain = gp.nd_utility(gain_A ** 2 * var, gain_A * mean + first["f_params"]["lambda0"].to(dev), counts)
    folded = gp.fold_posterior(first["K_tilde_b"], first["K_tilde_inv_b"], first["m_b"], first["V_b"], basis)
    out = gp.score_pool(images[rest], images[:n0], C, th, folded, first["f_params"], r_masked=counts, mask=px)
    print(f"\ng9: utility against the composition {relerr(out['utility'].cpu().numpy(), gain.cpu().numpy()):.2e}")
    assert int(out["utility"].argmax()) == int(gain.argmax()) == int(g["i_best"])


# ------------------------------------------------------------------ 7. stale workspace
def test_padding_is_written_not_assumed(gp, lib):
    u = _unit(cases.PROJECTED)
    clean = gp.pool_moments(u["xs"], u["xt"], u["C"], u["theta"], u["folded"])
    eng = gp.get_engine(200, 64, 64)
    for name in WORK_MATRICES:
        assert lib.gpfit_dev_ctx_fill(eng._ctx, name, 0xFF) == 0          # every double a NaN
    assert gp.get_engine(200, 64, 64) is eng
    mu, s2 = gp.pool_moments(u["xs"], u["xt"], u["C"], u["theta"], u["folded"])
    assert not torch.isnan(mu).any() and not torch.isnan(s2).any()
    assert same_bits(mu, clean[0]) and same_bits(s2, clean[1])
    for name in WORK_MATRICES:
        assert lib.gpfit_dev_ctx_fill(eng._ctx, name, 0) == 0             # as a fresh context holds them


# ------------------------------------------------------------------ 8. edges
def test_empty_pool(gp, link, counts):
    u = _unit(cases.CASES[1])
    out = gp.score_pool(u["xs"][:0], u["xt"], u["C"], u["theta"], u["folded"], link, r_masked=counts)
    assert all(out[key].shape == (0,) and out[key].dtype == torch.float64 for key in ("mu", "sigma2", "rate", "utility"))
    mu, s2 = gp.pool_moments(u["xs"][:0], u["xt"], u["C"], u["theta"], u["folded"])
    assert mu.shape == (0,) and s2.shape == (0,)


def test_no_response_counts_no_utility(gp, lib, link):
    u = _unit(cases.CASES[1])
    assert gp.score_pool(u["xs"], u["xt"], u["C"], u["theta"], u["folded"], link)["utility"] is None
    eng = gp.get_engine(200, 64)
    rc, mu, s2, rate, U = raw(lib, eng._ctx, u, A=0.05, lambda0=-0.3)
    assert rc == 0 and not (mu == SENTINEL).any() and not (s2 == SENTINEL).any() and not (rate == SENTINEL).any()
    assert bool((U == SENTINEL).all())


def test_refusals(gp, lib, link):
    from gaussian_processes_amd import _lib
    from gaussian_processes_amd.engine import GPFitEngine
    u = _unit(cases.CASES[1])
    small = GPFitEngine(64, 64)            # capacity 128 < nt = 200
    try:
        rc, mu, _, _, _ = raw(lib, small._ctx, u)
        assert rc == -3 and "larger than the context capacity" in _lib.last_error()
        assert bool((mu == SENTINEL).all())
        with pytest.raises(_lib.GpfitError, match="context capacity"):
            _lib.check(rc, "gpfit_score_pool")
    finally:
        small.close()
    with pytest.raises(ValueError):
        gp.pool_moments(u["xs"], u["xt"], u["C"], u["theta"], u["folded"], chunk_rows=100)
    with pytest.raises(ValueError):
        gp.score_pool(u["xs"], u["xt"], u["C"], u["theta"], u["folded"], link, chunk_rows=100)
    eng = gp.get_engine(200, 64)
    rc, mu, _, _, _ = raw(lib, eng._ctx, u, chunk_rows=100)
    assert rc == -3 and "chunk_rows" in _lib.last_error() and bool((mu == SENTINEL).all())
