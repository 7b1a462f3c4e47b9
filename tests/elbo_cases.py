"""Inputs and CPU arithmetic shared by the tests of the fused loss (test_elbo_cpu.py, test_gpu_elbo.py).

The inputs are those of the damped E-step (``estep_damped_cases.make_case``) with ``Kinv = sym(inv(K))``, ``lam_m = a m``
and ``lambda0 = -0.3``.  ``elbo_reference`` restates compute_loglikelihood (utils.py:1243) and compute_KL_div
(utils.py:1318-1326, with the log-determinants of :1278) in numpy fp64 as written there, ``trace(V @ Kinv)`` included;
``elbo_reference_longdouble`` is the same arithmetic in ``np.longdouble`` with a column-by-column Cholesky, the yardstick of
the restatement's own error."""
import numpy as np

from estep_damped_cases import CONDS, SHAPES, V_KINDS, make_case  # noqa: F401  (re-exported)

LAMBDA0 = -0.3
SLOTS = ("loglik", "KL", "loglik - KL", "log|V|", "log|K~|", "m^T K~^-1 m", "tr(V K~^-1)", "r.lam_m", "sum r", "sum f")
ALL_CASES = tuple((N, nb, cond, v_kind) for (N, nb) in SHAPES for cond in CONDS for v_kind in V_KINDS)


def make_elbo_case(N, nb, cond, v_kind):
    c = make_case(N, nb, cond, v_kind)
    Kinv = np.linalg.inv(c["K"])
    return dict(m=c["m"], V=c["V"], K=c["K"], Kinv=(Kinv + Kinv.T) / 2, r=c["r"], f=c["f"], lam_m=c["a"] @ c["m"],
                logA=c["logA"], lambda0=LAMBDA0, N=N, nb=nb)


def _assemble(A, lambda0, rlam, sum_r, sum_f, logdet_V, logdet_K, mkm, tr):
    loglik = A * rlam + lambda0 * sum_r - sum_f                                           # :1243
    KL = -0.5 * logdet_V + 0.5 * logdet_K + 0.5 * mkm + 0.5 * tr                         # :1326
    return [loglik, KL, loglik - KL, logdet_V, logdet_K, mkm, tr, rlam, sum_r, sum_f]


def elbo_reference(c, elementwise=False):
    """The ten numbers of gpfit_elbo in numpy fp64.  ``elementwise``: tr(V K~^-1) as sum_ij V_ij K~^-1_ij (what the
    device call evaluates) instead of the trace of the product (what :1318 writes)."""
    m, V, K, Kinv, r, f, lam_m = (c[k] for k in ("m", "V", "K", "Kinv", "r", "f", "lam_m"))
    b = Kinv @ m                                                                          # :1320
    tr = np.sum(V * Kinv) if elementwise else np.trace(V @ Kinv)                          # :1318, :1326
    logdet = [2.0 * np.sum(np.log(np.diagonal(np.linalg.cholesky(M)))) for M in (V, K)]   # :1278
    return np.array(_assemble(np.exp(c["logA"]), c["lambda0"], r @ lam_m, np.sum(r), np.sum(f), logdet[0], logdet[1], m @ b, tr),
                    dtype=np.float64)


def _logdet_longdouble(M):
    """2 sum log diag of the Cholesky factor, column by column in np.longdouble."""
    A = M.astype(np.longdouble)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is not positive")
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return 2 * np.sum(np.log(np.diagonal(L)))


def elbo_reference_longdouble(c, elementwise=False):
    ld = np.longdouble
    m, V, K, Kinv, r, f, lam_m = (c[k].astype(ld) for k in ("m", "V", "K", "Kinv", "r", "f", "lam_m"))
    b = Kinv @ m
    tr = np.sum(V * Kinv) if elementwise else np.trace(V @ Kinv)
    return np.array(_assemble(np.exp(ld(c["logA"])), ld(c["lambda0"]), r @ lam_m, np.sum(r), np.sum(f), _logdet_longdouble(c["V"]),
                              _logdet_longdouble(c["K"]), m @ b, tr), dtype=ld)
