"""CPU arithmetic shared by the tests of the chained damped E-steps (test_estep_damped_chain_cpu.py,
test_gpu_estep_damped_chain.py): the n-step loop a call of gpfit_estep_chain_damped stands for, restated in numpy fp64
on the inputs of estep_damped_cases.  A step is an update of (m, V), the moments of lambda at the new (m, V), and the
rate-parameter optimiser on those moments (the library's host instance, gpfit_fparam_lbfgs_host), which hands logA and
the rate to the next step.  Two updates: ``cholesky_update`` (estep_damped_cases.cholesky_estep, the formulation of the
device call) and ``reference_update`` (estep_damped_cases.reference_estep, the reference's lines with their LU solves).
Both answer a V that is not positive definite with the full Newton step for that one update, as varGP's host loop
does."""
import ctypes

import numpy as np

import estep_damped_cases as cases
from gaussian_processes_amd import _lib

LBFGS = (0.1, 1e-7, 1e-9)   # lr, tol_grad, tol_change of the rate-parameter optimiser inside a chain (utils._FPARAM_LBFGS)


def kv0_of(N, seed=0):
    """A fixed, positive Kvec - rowsum(K o a) for a case of N training points."""
    return 0.05 + 0.1 * np.random.default_rng(500 + 13 * seed + N).random(N)


def indefinite(V):
    """V minus twice its largest eigenvalue along the top eigenvector: symmetric with one negative eigenvalue."""
    w, Q = np.linalg.eigh(V)
    v = Q[:, -1]
    Vi = V - 2.0 * w[-1] * np.outer(v, v)
    return (Vi + Vi.T) / 2


def is_posdef(V):
    try:
        np.linalg.cholesky(V)
        return True
    except np.linalg.LinAlgError:
        return False


def full_cholesky_estep(r, a, m, logA, f, K):
    """The full Newton step from Cholesky factors only: with K~ = L L^T, Y = diag(A sqrt f) (a L), W1 = I + Y^T Y,
    V_new = (L L_W1^-T)(L L_W1^-T)^T, m_new = L W1^-1 (a L)^T u, u = A^2 f (a m) + A (r - f)."""
    A = np.exp(logA)
    n = K.shape[0]
    I = np.eye(n)
    L = np.linalg.cholesky(K)
    aL = a @ L
    Y = (A * np.sqrt(f))[:, None] * aL
    LW1 = np.linalg.cholesky(I + Y.T @ Y)
    u = A * A * f * (a @ m) + A * (r - f)
    m_new = L @ np.linalg.solve(LW1.T, np.linalg.solve(LW1, aL.T @ u))
    T = L @ np.linalg.solve(LW1, I).T
    return m_new, T @ T.T


def cholesky_update(r, a, m, logA, f, K, V, alpha):
    """(m_new, V_new, full): the damped update from Cholesky factors, or the full step when V is not positive definite."""
    if not is_posdef(V):
        return full_cholesky_estep(r, a, m, logA, f, K) + (True,)
    return cases.cholesky_estep(r, a, m, logA, f, K, V, alpha) + (False,)


def reference_update(r, a, m, logA, f, K, V, alpha):
    """The same with the reference's own lines (alpha = 1 where V is not positive definite)."""
    if not is_posdef(V):
        return cases.reference_estep(r, a, m, logA, f, K, alpha=1) + (True,)
    return cases.reference_estep(r, a, m, logA, f, K, V, alpha) + (False,)


def moments(a, m, V, kv0):
    """lam_m = a m, lam_var = kv0 + diag(a V a^T)."""
    return a @ m, kv0 + np.einsum("ij,jk,ik->i", a, V, a)


def fparam_lbfgs_host(lam_m, lam_var, r, logA0, max_iter):
    """gpfit_fparam_lbfgs_host with the closed-form lambda0: (the rate at the final point, out[9])."""
    n = lam_m.shape[0]
    lam_m, lam_var, r = (np.ascontiguousarray(x, dtype=np.float64) for x in (lam_m, lam_var, r))
    f = np.empty(n)
    out = (ctypes.c_double * 9)()
    rc = _lib.load().gpfit_fparam_lbfgs_host(lam_m.ctypes.data, lam_var.ctypes.data, r.ctypes.data, n, float(logA0), 0, 0.0,
                                             int(max_iter), int(max_iter), *LBFGS, f.ctypes.data, out)
    assert rc == 0 and out[6] == 0, (rc, list(out))
    return f, list(out)


def loop(c, kv0, alpha, n_steps, nfp, update, V=None):
    """The n-step loop on the case ``c`` from its (m, V, f, logA): per step (m, V, lam_m, lam_var, f, logA, full)."""
    m, f, logA = c["m"], c["f"], float(c["logA"])
    V = c["V"] if V is None else V
    steps = []
    for _ in range(n_steps):
        m, V, full = update(c["r"], c["a"], m, logA, f, c["K"], V, alpha)
        V = (V + V.T) / 2
        lam_m, lam_var = moments(c["a"], m, V, kv0)
        f, out = fparam_lbfgs_host(lam_m, lam_var, c["r"], logA, nfp)
        logA = out[0]
        steps.append(dict(m=m, V=V, lam_m=lam_m, lam_var=lam_var, f=f, logA=logA, full=full))
    return steps
