"""``utils._stabilised_basis`` -- the routing between the reference's eigh, the spectral projector of K~ itself and the
block subspace sweeps, on the library's own GEMM, Cholesky, sweep chain and sign chain -- on the designed spectra of
spectrum_cases.py: clustered tops, eigenvalues a hair above and below the threshold, the floor branch, the orthogonal
start, a plateau wider than the start block, kept counts beyond the largest block, nothing dropped.  The truth is the
design of each matrix.  K is built on the host and uploaded; the sizes are the smallest at which each route and each edge of the routing exists: 256 (the first dense
size), 264 (padded to 272 inside), 1776 (the last dense size), 1792 (the first sweeps size), 2048 (where the largest
block becomes half of n).  test_spectrum_cases_cpu.py runs the full table through ``eigtop`` on CPU stand-ins."""
import numpy as np
import pytest
import torch

import spectrum_cases as sc
from gaussian_processes_amd import eigtop

pytestmark = pytest.mark.gpu
SIZES = (256, 264, 1776, 1792, 2048)
TOL = 1e-3
ROUTES = ("identity", "subspace", "eigtop", "eigh")
CASES = [pytest.param(n, i, id=f"{c.name}") for n in SIZES for i, c in enumerate(sc.gpu_cases(n))]


@pytest.fixture(scope="module")
def gp():
    from gaussian_processes_amd import utils
    return utils


@pytest.fixture
def tol(gp):
    """EIGVAL_TOL of the table for one test, and no regime hint before or after it."""
    old = gp.EIGVAL_TOL
    gp.EIGVAL_TOL = TOL
    gp._BASIS.__dict__.pop("regime", None)
    try:
        yield TOL
    finally:
        gp.EIGVAL_TOL = old
        gp._BASIS.__dict__.pop("regime", None)
        gp._BASIS.state = None


def T(a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()


def check_basis(gp, case, K, out, n_kept=None):
    """B orthonormal and spanning the design's kept columns, K~_b = B^T K~ B and its inverse."""
    _, B, Kb, Kib = out
    n = case.count if n_kept is None else n_kept
    assert tuple(B.shape) == (case.n, n), (gp._BASIS.route, tuple(B.shape), n)
    eye = torch.eye(n, dtype=torch.float64, device=B.device)
    assert float((B.T @ B - eye).abs().max()) < 1e-12
    P = T(case.Q()[:, :n]).T @ B
    assert float((P.T @ P - eye).abs().max()) < 1e-9
    assert float((Kb - B.T @ K @ B).abs().max()) < 1e-12 * float(case.lam[0])
    assert float((Kib @ Kb - eye).abs().max()) < 1e-9


@pytest.mark.parametrize("n, i", CASES)
def test_the_design_count_and_space_by_whichever_route(gp, tol, n, i):
    """Every MUST_DECIDE and NEVER_WRONG case of the table, at every size: through ``_stabilised_basis`` neither may be
    wrong, the reference's eigh is the last resort -- also where more is kept than the largest block holds, and where
    nothing is dropped (the only cases the identity basis may answer).  The recorded route replays the same bits."""
    case = sc.gpu_cases(n)[i]
    assert case.tol == tol and sc.AMBIGUOUS not in (case.cls, case.cls_dense)
    K = T(case.K())
    out = gp._stabilised_basis(K)
    route = gp._BASIS.route
    print(f"{case.name}: route {route} kept {out[1].shape[1]} design {case.count}")
    assert route in ROUTES and (route == "identity") <= (case.extent == "all")
    check_basis(gp, case, K, out)
    again = gp._stabilised_basis(K, route=route)
    assert gp._BASIS.route == route
    for a, b in zip(out[1:], again[1:]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n", (264, 1792))
def test_regime_hints_never_change_the_answer(gp, tol, n):
    """truncated -> everything kept -> truncated -> clustered at one size: the hint of (n, tol) is set by each answer and
    only decides which rank check runs first, never the route's count."""
    key = (n, float(tol))
    truncated, clustered = sc.decay(n, "rho0.5", -5e-4), sc.decay(n, "rho0.9", -5e-4)
    full = sc.all_kept(n, tol=tol)
    for step, case in enumerate((truncated, full, truncated, clustered)):
        K = T(case.K())
        out = gp._stabilised_basis(K)
        route, hint = gp._BASIS.route, gp._BASIS.regime.get(key)
        print(f"n {n} step {step} {case.name}: route {route} hint {hint} kept {out[1].shape[1]}")
        assert tuple(out[1].shape) == (n, case.count), (step, route)
        if case is full:
            # the sweeps decline (nothing to truncate); below 1792 the projector proves it, from there the norm bounds
            # of the all-kept proof have to, and where they are not sharp enough the reference's eigh keeps every column
            assert route == "identity" if n < 1792 else route in ("identity", "eigh")
            assert hint == ("full" if route == "identity" else "truncated")
            eye = torch.eye(n, dtype=torch.float64, device=K.device)
            assert float((out[1].T @ out[1] - eye).abs().max()) < 1e-12
        else:
            assert route in ("subspace", "eigtop", "eigh") and hint == "truncated"
            check_basis(gp, case, K, out)


def _spd(n, lam):
    Q = sc.orthogonal(n)
    K = (Q * lam) @ Q.T
    return T((K + K.T) * 0.5)


def test_the_all_kept_proof_never_claims_a_matrix_with_an_eigenvalue_below_the_threshold(gp, tol):
    """lambda_min = tau (1 - delta), delta = 1e-2 ... 1e-6, tau = lambda_1 tol: the norm bounds are rigorous, so the proof
    must say no -- and ``_stabilised_basis`` drops exactly that one direction.  A matrix well inside (lambda in [1, 2] at
    tol = 1e-6: lambda_min >= 1 / n by the bound's own inequalities, against a threshold of at most 1.5 n tol) is
    claimed."""
    n = 256
    for delta in (1e-2, 1e-3, 1e-4, 1e-5, 1e-6):
        lam = np.geomspace(2.0, 2.0 * tol * 1.5, n)
        lam[-1] = 2.0 * tol * (1.0 - delta)
        K = _spd(n, lam)
        kept, L, Li = gp._all_eigenvalues_kept(K)
        assert kept is False and L is not None, delta
        gp._BASIS.__dict__.pop("regime", None)
        out = gp._stabilised_basis(K)
        assert gp._BASIS.route != "identity" and tuple(out[1].shape) == (n, n - 1), (delta, gp._BASIS.route)
    gp.EIGVAL_TOL = 1e-6
    K = _spd(n, np.linspace(2.0, 1.0, n))
    assert gp._all_eigenvalues_kept(K)[0] is True
    gp._BASIS.__dict__.pop("regime", None)
    out = gp._stabilised_basis(K)
    assert gp._BASIS.route == "identity" and tuple(out[1].shape) == (n, n) and gp._is_identity(out[1])


def test_a_clustered_top_has_the_same_bits_with_the_chains_on_and_off(gp, tol, monkeypatch):
    """n = 2048, rho = 0.9, the nearest eigenvalue 5e-4 tau below the threshold: SWEEP_CHAIN and SIGN_CHAIN change how the
    sweeps and the sign iteration are issued, not one bit of the basis."""
    case = sc.decay(2048, "rho0.9", -5e-4)
    K = T(case.K())
    outs = {}
    for sweep in (True, False):
        for sign in (True, False):
            monkeypatch.setattr(gp, "SWEEP_CHAIN", sweep)
            monkeypatch.setattr(gp, "SIGN_CHAIN", sign)
            gp._BASIS.__dict__.pop("regime", None)
            outs[sweep, sign] = gp._stabilised_basis(K), gp._BASIS.route
    ref, route = outs[True, True]
    check_basis(gp, case, K, ref)
    for key, (out, r) in outs.items():
        assert r == route, key
        for a, b in zip(ref[1:], out[1:]):
            assert torch.equal(a, b), key


def test_warm_start_from_the_fits_kernel_matrix_onto_a_clustered_top(gp, tol):
    """The solver state a basis rebuild of the fit's own kernel matrix leaves at N = 2048 (single dominant top), handed
    to the rebuild of a clustered matrix of the same size: the start is taken, and the count is the design's."""
    from test_gpu_dropin import _bench_kernel_matrix
    _, Kfit = _bench_kernel_matrix(gp, 2048)
    gp.EIGVAL_TOL = 1e-4                       # the fit's default keeps ~540 of 2048: a block of 1024 holds them
    gp._stabilised_basis(Kfit)
    state = gp._BASIS.state
    assert gp._BASIS.route == "subspace" and state is not None and state["Q"].shape[0] == 2048
    gp.EIGVAL_TOL = tol
    gp._BASIS.__dict__.pop("regime", None)
    case = sc.decay(2048, "rho0.9", -5e-4)
    K = T(case.K())
    sw = eigtop.top_eigenpairs(K, tol, gp.matmul, gp.cholesky, basis="subspace", gemm_into=gp.gemm_into, start=state,
                               sweep_chain=gp._basis_sweeps)
    assert sw is not None and sw[2]["warm"] is True and sw[2]["n"] == case.count
    out = gp._stabilised_basis(K, start=state)
    print(f"warm: route {gp._BASIS.route} kept {out[1].shape[1]}")
    assert gp._BASIS.route in ("subspace", "eigtop")          # the sweeps answered, from the start they were given
    check_basis(gp, case, K, out)
    # the cold rebuild of the same matrix: the same space, and the canonical basis to the sweeps' certificate
    gp._BASIS.__dict__.pop("regime", None)
    cold = gp._stabilised_basis(K)
    check_basis(gp, case, K, cold)
    if gp._BASIS.route == "subspace" and sw[0] is None:
        print(f"warm vs cold: max |dB| {float((out[1] - cold[1]).abs().max()):.2e}")
        assert float((out[1] - cold[1]).abs().max()) < 1e-5
