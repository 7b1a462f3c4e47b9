"""Inputs and CPU arithmetic shared by the tests of the damped E-step (test_estep_damped_cpu.py,
test_gpu_estep_damped.py) and by the generator of their fixture (golden/make_golden_damped.py).  numpy fp64 only.

``reference_estep`` restates the reference's ``Estep`` (utils.py:1420-1438, both alpha branches) line by line, LU solves
included; ``cholesky_estep`` is the formulation the device call implements.  The restatement is pinned to the real
reference by ``golden/g11_estep_damped.npz``."""
import numpy as np

SHAPES = ((64, 64), (130, 130), (200, 130), (1000, 300))
CONDS = (1e2, 1e4, 1e8)
ALPHAS = (0.5, 0.05)
V_KINDS = ("prior", "newton")
LOG_A = 0.1


def make_case(N, nb, cond, v_kind, seed=0):
    """K~ = Q diag(ev) Q^T with ev log-spaced down from 50, a ~ N(0, 1) / sqrt(nb) (orthogonal when N == nb: the
    full-rank use), f = exp(0.7 lam - 0.3) with lam ~ 0.5 N(0, 1), r ~ Poisson(f), m ~ N(0, 1); V = K~ ("prior") or the
    symmetrised solve(I + 1.7 K~ G, K~) ("newton": a previous Newton result at another rate)."""
    rng = np.random.default_rng(1000 * seed + 7 * N + nb)
    Q, _ = np.linalg.qr(rng.standard_normal((nb, nb)))
    ev = 50.0 * np.logspace(0.0, -np.log10(cond), nb)
    K = (Q * ev) @ Q.T
    K = (K + K.T) / 2
    if N == nb:
        a, _ = np.linalg.qr(rng.standard_normal((N, nb)))
    else:
        a = rng.standard_normal((N, nb)) / np.sqrt(nb)
    lam = 0.5 * rng.standard_normal(N)
    f = np.exp(0.7 * lam - 0.3)
    r = rng.poisson(f).astype(np.float64)
    m = rng.standard_normal(nb)
    if v_kind == "prior":
        V = K.copy()
    else:
        A = np.exp(LOG_A)
        G = 1.7 * A * A * a.T @ (a * f[:, None])
        V = np.linalg.solve(np.eye(nb) + K @ G, K)
        V = (V + V.T) / 2
    return dict(K=K, a=np.ascontiguousarray(a), f=f, r=r, m=m, V=V, logA=LOG_A)


def reference_estep(r, a, m, logA, f, K, V=None, alpha=1.0):
    """utils.py:1420-1438 as written there."""
    A = np.exp(logA)
    g = A * a.T @ (r - f)                                                                      # :1421
    G = A * A * a.T @ (a * f[:, None])                                                         # :1422
    n = K.shape[0]
    if alpha == 1:
        V_new = np.linalg.solve(np.eye(n) + K @ G, K)                                          # :1430
        m_new = V_new @ (G @ m + g)                                                            # :1431
    else:
        V_new = V @ np.linalg.solve((1 - alpha) * K + alpha * V + alpha * (K @ G) @ V, K)      # :1435
        m_new = m - alpha * np.linalg.solve(np.eye(n) + K @ G, m - K @ g)                      # :1436
    return m_new, (V_new + V_new.T) / 2                                                        # :1438


def cholesky_estep(r, a, m, logA, f, K, V, alpha):
    """The same update from Cholesky factors only (every ``np.linalg.cholesky`` raises unless its matrix is positive
    definite): with K~ = L L^T,
        Y = diag(A sqrt f) (a L),  W1 = I + Y^T Y,  P = L^-1 V L^-T,  W_a = (1 - a) P^-1 + a W1,
        V_new = (L L_Wa^-T)(L L_Wa^-T)^T,  m_new = m - a L W1^-1 (L^-1 m - A (a L)^T (r - f))."""
    A = np.exp(logA)
    n = K.shape[0]
    I = np.eye(n)
    L = np.linalg.cholesky(K)
    Li = np.linalg.solve(L, I)
    aL = a @ L
    Y = (A * np.sqrt(f))[:, None] * aL
    W1 = I + Y.T @ Y
    P = Li @ V @ Li.T
    P = (P + P.T) / 2
    LPi = np.linalg.solve(np.linalg.cholesky(P), I)
    Wa = (1 - alpha) * LPi.T @ LPi + alpha * W1
    Wa = (Wa + Wa.T) / 2
    T = L @ np.linalg.solve(np.linalg.cholesky(Wa), I).T
    V_new = T @ T.T
    LW1 = np.linalg.cholesky(W1)
    rhs = Li @ m - A * aL.T @ (r - f)
    m_new = m - alpha * L @ np.linalg.solve(LW1.T, np.linalg.solve(LW1, rhs))
    return m_new, V_new
