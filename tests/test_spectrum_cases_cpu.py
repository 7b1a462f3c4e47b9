"""The rank decision of a basis rebuild -- how many eigenvalues of K~ lie above ``max(lambda_1 tol, tol)`` -- on spectra the
routes of ``eigtop`` were not built on: clustered tops, eigenvalues a hair above and below the threshold, the floor
branch, a start vector orthogonal to the top eigenvector, kept counts around and beyond the block (spectrum_cases.py).
The truth is the design of each matrix, no solver.  Everything here runs ``eigtop`` on the CPU stand-ins of
test_eigtop_cpu.py at n = 600 / 608, ``k0 = 128``; test_gpu_basis_spectra.py runs the table through the library."""
import numpy as np
import pytest
import torch

import spectrum_cases as sc
from gaussian_processes_amd import eigtop
from test_eigtop_cpu import cpu_cholesky, cpu_matmul

CASES = sc.cpu_cases()
CALLERS = ("subspace", "eigenvectors", "dense", "direct")


# ------------------------------------------------------------------ the table itself
def test_the_table_covers_its_axes():
    cases = sc.table(600)
    pairs = {(c.top, c.delta) for c in cases if c.q == "qr" and c.lam[0] > 1 and c.moved >= 0 and c.top in sc.TOPS}
    assert pairs == {(t, d) for t in sc.TOPS for d in sc.DELTAS}
    assert len(sc.DELTAS) == 12 and {abs(d) for d in sc.DELTAS} == {1e-2, 1e-3, 5e-4, 1e-5, 1e-6, 1e-10}
    floor = [c for c in cases if c.lam[0] < 1]
    assert {c.top for c in floor} == {"rho0.5", "rho0.9"} and all(c.tau == c.tol for c in floor)
    assert all(c.tau == c.lam[0] * c.tol > c.tol for c in cases if c.lam[0] > 1)
    assert any(c.q == "householder" for c in cases)
    assert {c.count for c in cases if c.top == "geom" and c.extent == "fits"} == {sc.K0 - 1, sc.K0, sc.K0 + 1}
    assert any(c.extent == "too_wide" and c.count > c.n // 3 for c in cases)
    assert any(c.extent == "all" and c.count == c.n for c in cases)
    plateau = [c for c in cases if c.name.startswith("plateau")]
    assert len(plateau) == 1
    lam, tau = plateau[0].lam, plateau[0].tau
    assert int((lam == 1.05 * tau).sum()) == 145 and plateau[0].count == 146 > sc.K0 and float(lam[146]) <= 0.5 * tau
    assert {c.n % 16 == 0 for c in CASES} == {True, False}
    for c in CASES:
        # the classes follow the rule of the module's docstring; none is stricter on the dense route than on the sweeps
        if c.cls == sc.MUST_DECIDE or c.cls_dense == sc.MUST_DECIDE:
            assert abs(c.delta) >= 1e-3
        if c.cls_dense == sc.MUST_DECIDE:
            assert c.cls == sc.MUST_DECIDE
        assert (c.cls == sc.AMBIGUOUS) == (abs(c.delta) == 1e-10) == (c.cls_dense == sc.AMBIGUOUS)
        if c.top in sc.TOPS and abs(c.delta) >= 1e-3:
            assert (c.cls == sc.MUST_DECIDE) == (c.top in ("rho0.5", "rho0.9", "rho0.99", "double", "triple"))
            assert (c.cls_dense == sc.MUST_DECIDE) == (c.top in ("rho0.5", "rho0.9", "double", "triple"))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_design_is_the_spectrum(case):
    """fp64 ``eigvalsh`` of K has the design's top eigenvalue to 1e-13 and, where the moved eigenvalue is 1e-6 or more
    from the threshold, the design's count; the gap across the threshold is 1e-2 tau or more."""
    K = case.K()
    assert np.array_equal(K, K.T)
    w = np.linalg.eigvalsh(K)
    assert abs(w[-1] - case.lam[0]) <= 1e-13 * case.lam[0]
    assert case.count == int((case.lam > case.tau).sum())
    if abs(case.delta) >= 1e-6:
        assert int((w > max(w[-1] * case.tol, case.tol)).sum()) == case.count
    assert case.gap() >= 1e-2 * case.tau
    if case.moved >= 0 and case.top in sc.TOPS:
        assert case.lam[case.moved] == case.tau * (1.0 + case.delta)
        assert case.count == case.moved + (1 if case.delta > 0 else 0)
    Q = case.Q()
    assert float(np.abs(Q.T @ Q - np.eye(case.n)).max()) < 1e-13
    if case.q == "householder":
        j = int(np.argmax(np.diagonal(K)))
        best, top = K[:, j], Q[:, 0]
        assert j == 1 and abs(float(best @ top)) <= 1e-15 * float(np.linalg.norm(best))
        assert case.lam[1] == 0.9 * case.lam[0]


# ------------------------------------------------------------------ every case through the four callers
def _run(caller, case, K, **kw):
    """``(n, B, K_tilde_b, K_tilde_inv_b, lam_max, route)`` of an answer, ``"all"`` for an all-kept proof, None."""
    if caller in ("subspace", "eigenvectors"):
        out = eigtop.top_eigenpairs(K, case.tol, cpu_matmul, cpu_cholesky, k0=sc.K0, basis=caller, **kw)
        if out is None:
            return None
        vals, vecs, info = out
        if vals is None:
            assert info["route"] == "subspace"
            return info["n"], vecs, info["K_tilde_b"], info["K_tilde_inv_b"], info["lam_max"], info
        # the eigenpair route (asked for, or the fall-through of basis="subspace") records no info["lam_max"]: its
        # threshold comes from the top Ritz value of its own k x k eigh, the last of ``vals``, which is held to the same 1e-8
        assert "lam_max" not in info
        return info["n"], vecs, torch.diag(vals), torch.diag(1 / vals), float(vals[-1]), info
    if caller == "dense":
        out = eigtop.kept_eigenspace_dense(K, case.tol, cpu_matmul, cpu_cholesky)
        if out is None:
            return None
        if out[1] is None:
            assert out[2]["all_kept"] and out[2]["n"] == case.n and out[2]["route"] == "identity"
            return "all"
        info = out[2]
        return info["n"], out[1], info["K_tilde_b"], info["K_tilde_inv_b"], info["lam_max"], info
    sub = eigtop._kept_subspace(torch.eye(case.n, dtype=torch.float64), K, K, case.tol, 0.0, cpu_matmul, cpu_cholesky, 1e-7)
    if sub is None:
        return None
    assert sub["angle"] < 1e-7            # the whole space as the block: nothing leaves it
    return sub["n"], sub["B"], sub["K_tilde_b"], sub["K_tilde_inv_b"], sub["lam_max"], sub


def _check_answer(case, got):
    """What every answer must satisfy, whatever the class: the count rule of the class, lambda_max to the certificate,
    an orthonormal B that spans the design's kept columns, K~_b with the kept eigenvalues and its inverse."""
    n, B, Kb, Kib, lam_max, _ = got
    if case.cls == sc.AMBIGUOUS:
        # only the one moved eigenvalue, 1e-10 tau from the threshold, may land on either side
        assert n in (case.moved, case.moved + 1), (n, case.count)
    else:
        assert n == case.count, (n, case.count)
    assert abs(lam_max - case.lam[0]) <= 1e-8 * case.lam[0], lam_max / case.lam[0] - 1
    eye = torch.eye(n, dtype=torch.float64)
    assert B.shape == (case.n, n)
    assert float((B.T @ B - eye).abs().max()) < 1e-12
    P = torch.from_numpy(case.Q()[:, :n].copy()).T @ B
    assert float((P.T @ P - eye).abs().max()) < 1e-9
    lam = torch.from_numpy(case.lam[:n].copy()).flip(0)
    assert float(((torch.linalg.eigvalsh(Kb) - lam).abs() / lam).max()) < 1e-10
    assert float((Kib @ Kb - eye).abs().max()) < 1e-8


@pytest.mark.parametrize("caller", CALLERS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_caller_keeps_to_the_class_of_the_case(case, caller):
    """``top_eigenpairs`` in both basis modes, ``kept_eigenspace_dense`` and ``_kept_subspace`` with the whole space as
    its block (Q = I): MUST_DECIDE cases are answered, and every answer of any class is the design's.

    Declines seen on NEVER_WRONG cases, and meant: on the matrix itself (``dense``, ``direct``) a top cluster
    lambda_1 = lambda_2, lambda_3 = lambda_1 (1 - 1e-6) leaves the Rayleigh quotient about 1e-7 lambda_1 short, which the
    1e-8 certificate refuses, and telling members 1e-6 apart takes ~1e7 power steps against the 2e4 of the unstick
    branch; through the sweeps the k x k quotient matrix happens to settle within the certificate."""
    K = torch.from_numpy(case.K())
    got = _run(caller, case, K)
    sweeps = caller in ("subspace", "eigenvectors")
    if case.extent != "fits" and sweeps:
        assert got is None                 # more is kept than the largest block holds: not a truncation problem
        return
    if case.extent == "all":
        # the dense route proves it; the block of ``direct`` IS the whole space and cannot hold a complement
        assert got == ("all" if caller == "dense" else None)
        return
    cls = case.cls if sweeps else case.cls_dense
    if cls == sc.MUST_DECIDE:
        assert got is not None
    if got is not None:
        assert got != "all"
        _check_answer(case, got)


# ------------------------------------------------------------------ warm start
@pytest.mark.parametrize("delta", (-5e-4, -1e-5))
def test_warm_start_from_a_dominant_top_onto_a_clustered_one(delta):
    """The state of a solve on a matrix with a single dominant top eigenvalue, handed to the solve of a nearby matrix
    whose top is clustered (rho = 0.9, the nearest eigenvalue at tau (1 + delta) below the threshold): the count is the
    design's.  The second matrix is the table's plus a symmetric perturbation of norm 1e-4 |delta| tau, which moves no
    eigenvalue across the threshold (Weyl) and the block's best column off the old top eigenvector."""
    first, second = sc.decay(600, "rho0.5", -1e-2), sc.decay(600, "rho0.9", delta)
    cold = eigtop.top_eigenpairs(torch.from_numpy(first.K()), first.tol, cpu_matmul, cpu_cholesky, k0=sc.K0, basis="subspace")
    assert cold is not None and cold[2]["route"] == "subspace" and cold[2]["n"] == first.count
    E = np.random.default_rng(9).standard_normal((600, 600))
    E = (E + E.T) / 2
    K2 = torch.from_numpy(second.K() + 1e-4 * abs(delta) * second.tau * E / np.linalg.norm(E, 2))
    warm = eigtop.top_eigenpairs(K2, second.tol, cpu_matmul, cpu_cholesky, k0=sc.K0, basis="subspace", start=cold[2]["state"])
    assert warm is not None and warm[2]["warm"] is True
    assert warm[2]["n"] == second.count == 31
    if warm[0] is None:
        assert abs(warm[2]["lam_max"] - second.lam[0]) <= 1e-8 * second.lam[0]
    P = torch.from_numpy(second.kept_columns().copy()).T @ warm[1]
    assert float((P.T @ P - torch.eye(31, dtype=torch.float64)).abs().max()) < 1e-9
    # the cold solve of the same matrix: the same count, and the canonical basis up to the sweeps' certificate (the bound
    # the existing warm-start test holds)
    cold2 = eigtop.top_eigenpairs(K2, second.tol, cpu_matmul, cpu_cholesky, k0=sc.K0, basis="subspace")
    assert cold2 is not None and cold2[2]["n"] == 31
    if warm[0] is None and cold2[0] is None:
        assert float((warm[1] - cold2[1]).abs().max()) < 1e-5


# ------------------------------------------------------------------ the unstick branch
def test_the_orthogonal_start_enters_the_unstick_branch_and_the_dense_route_decides():
    """On the orthogonal-start matrix the column of the largest diagonal entry is ``lambda_2 e_1`` to the bit, an
    eigenvector: power steps never leave it, the quotient stands still at 0.9 lambda_1 and the certificate refuses it.
    The dense route then takes the branch that squares S six times -- seen here as the FIRST six products, each of a
    matrix with itself, before the Cayley transform's ``L^-T L^-1``.  (Up to the parent of this test the route declined
    here: no power of S moves an exact eigenvector either.  The branch now mixes a fixed pseudo-random vector into the
    iterate first, and the route decides: two certificate factorisations, the second one passing.)"""
    case = next(c for c in sc.table(600) if c.q == "householder" and c.delta == -5e-4)
    products, certificates = [], []

    def matmul(A, B, transA=False, transB=False):
        products.append((A is B, transA, transB, tuple(A.shape)))
        return cpu_matmul(A, B, transA, transB)

    def cholesky(M, want_inverse=False):
        out = cpu_cholesky(M, want_inverse)
        if not want_inverse:
            certificates.append(out[3])
        return out

    out = eigtop.kept_eigenspace_dense(torch.from_numpy(case.K()), case.tol, matmul, cholesky)
    assert products[:6] == [(True, False, False, (608, 608))] * 6 and products[6] == (True, True, False, (608, 608))
    assert len(certificates) == 2 and certificates[0] != 0 and certificates[1] == 0
    assert out is not None and out[2]["n"] == case.count == 31
    assert abs(out[2]["lam_max"] - case.lam[0]) <= 1e-8 * case.lam[0]
    # a friendly top passes the first certificate: no squarings
    products.clear(), certificates.clear()
    easy = sc.decay(600, "rho0.5", -5e-4)
    assert eigtop.kept_eigenspace_dense(torch.from_numpy(easy.K()), easy.tol, matmul, cholesky)[2]["n"] == 31
    assert certificates == [0] and products[0] == (True, True, False, (608, 608))


def test_the_block_route_certifies_lambda_max_or_declines():
    """``_kept_subspace`` on a converged block (Q given): one certificate factorisation when the top eigenvalue stands
    alone; with a clustered top the first one fails, more steps follow, and lambda_max is the top eigenvalue of S to 1e-8;
    a certificate that never passes makes the function decline, so that ``top_eigenpairs`` takes its eigenpair route."""
    certificates = []

    def cholesky(M, want_inverse=False):
        out = cpu_cholesky(M, want_inverse)
        if not want_inverse:
            certificates.append(out[3])
        return out

    for top, fails in (("rho0.5", 0), ("rho0.99", 1)):
        case = sc.decay(600, top, -1e-3)
        certificates.clear()
        out = eigtop.top_eigenpairs(torch.from_numpy(case.K()), case.tol, cpu_matmul, cholesky, k0=sc.K0, basis="subspace")
        assert out[2]["route"] == "subspace" and out[2]["n"] == 31
        assert sum(1 for c in certificates if c != 0) >= fails and certificates[-1] == 0
        assert len(certificates) == 1 if not fails else len(certificates) >= 2

    def never(M, want_inverse=False):
        return cpu_cholesky(M, want_inverse) if want_inverse else (None, None, 0.0, 1)

    case = sc.decay(600, "rho0.5", -1e-3)
    K = torch.from_numpy(case.K())
    assert eigtop._kept_subspace(torch.eye(600, dtype=torch.float64), K, K, case.tol, 0.0, cpu_matmul, never, 1e-7) is None
    out = eigtop.top_eigenpairs(K, case.tol, cpu_matmul, never, k0=sc.K0, basis="subspace")
    assert out is not None and out[0] is not None and out[2]["rr"] >= 1 and out[2]["n"] == 31
