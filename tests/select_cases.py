"""Inputs and CPU arithmetic shared by the tests of the batch-aware selection (test_select_cases_cpu.py,
test_gpu_pool_covariance.py, test_gpu_select_batch.py).

``sigma_longdouble`` is the posterior covariance of the latents of a pool, ``k(x_i, x_j) + z_i S z_j^T`` with the diagonal in
the ``k** + z S z^T`` form of the moments, from ``acosker_ld`` / ``acosker_diag_ld`` and the case's ``S`` in
``np.longdouble``.  ``greedy`` is the recurrence of gpfit_select_batch -- utility, pick, rank-1 conditioning with
pseudo-noise ``tau = 1 / (A^2 f)`` -- in the dtype asked for: ``greedy_reference`` runs it in ``np.longdouble`` (the
yardstick), ``greedy_f64`` is the plain numpy fp64 transcription.  The utility comes from ``oracle.active_utility`` on the
fp64-rounded arguments in both.

Link scalars: ``A = 1`` or ``A = 0.5`` with ``lambda0 = -0.3``, not ``synthetic.F_PARAMS``: at ``A = 0.05`` the pseudo-noise is
in the hundreds, one presentation conditions nothing and the rule degenerates to the top-B (asserted once, as a property,
in test_select_cases_cpu.py)."""
import functools

import numpy as np
import torch

import predict_cases as cases
import predict_group_cases as groups
from oracle import gp_oracle as orc
from test_kernel_reference_cpu import acosker_diag_ld, acosker_ld

LD = np.longdouble
COUNTS = np.arange(100, dtype=np.float64)
LAMBDA0 = -0.3

# name -> (shape of predict_cases.CASES, A, n_select)
SINGLE = {"identity130": ((130, 200, 200, 8), 1.0, 8), "projected130": ((130, 200, 77, 8), 0.5, 8),
          "identity300": ((300, 384, 384, 8), 1.0, 128)}
# name -> (group of predict_group_cases, weights, n_select); unit u has A = 1 (u even) or 0.5 (u odd)
UNITS = {"three": (groups.PROJECTED3, (1.0, 0.5, 2.0), 8),
         "sixteen": (groups.SIXTEEN, tuple(0.5 + 0.1 * u for u in range(16)), 8)}
DUPLICATE_SHAPE = (130, 200, 200, 8)
DUPLICATES = ((20, 21, 1.0), (46, 47, 1.001))      # (row, its copy, scale of the copy)


def unit_A(u):
    return 1.0 if u % 2 == 0 else 0.5


def _basis(c):
    return np.eye(c["nt"], dtype=LD) if c["B"] is None else c["B"].astype(LD)


def fold_S_ld(c):
    Ki = c["Kinv"].astype(LD)
    S = Ki @ (c["V"].astype(LD) - c["K"].astype(LD)) @ Ki.T
    return (S + S.T) / 2


def sigma_longdouble(c):
    """(Sigma [P, P], mu [P]) of the latents of the case's pool, np.longdouble."""
    s0, mask = c["theta"]["sigma_0"], c["mask"]
    xs, xt = c["xstar"][:, mask], c["xtilde"][:, mask]
    P = xs.shape[0]
    # acosker symmetrises a square kernel matrix: the cross kernel over two halves of the pool where P == nt
    parts = (slice(0, P),) if P != xt.shape[0] else (slice(0, P // 2), slice(P // 2, P))
    z = np.concatenate([acosker_ld(s0, xs[rows], xt, c["C"])[0] for rows in parts]) @ _basis(c)
    S = fold_S_ld(c)
    zS = z @ S
    Sigma = acosker_ld(s0, xs, xs, c["C"])[0] + zS @ z.T
    Sigma = (Sigma + Sigma.T) / 2
    Sigma[np.arange(P), np.arange(P)] = acosker_diag_ld(s0, xs, c["C"])[0] + (zS * z).sum(1)
    mu = z @ (c["Kinv"].astype(LD) @ c["m"].astype(LD))
    return Sigma, mu


def utility_f64(s2, mu):
    return orc.active_utility(torch.from_numpy(np.asarray(s2, dtype=np.float64)), torch.from_numpy(np.asarray(mu, dtype=np.float64)),
                              torch.from_numpy(COUNTS)).numpy()


def greedy(Sigmas, mus, As, lambda0s, weights, n_select, dtype):
    """The recurrence of gpfit_select_batch in ``dtype``.  Sigmas, mus: per unit.  Returns a dict: ``picked`` (-1 once
    nothing qualifies), ``utility`` (T of the pick, NaN), ``sigma2`` (per unit, the conditional variances), ``tau`` (per
    unit and pick), ``gap`` (per step: (best - runner-up) / |best| among the rows that qualify, inf without a runner-up)
    and ``T`` (per step, the population utility of every row)."""
    nu, M = len(Sigmas), Sigmas[0].shape[0]
    Sig = [np.asarray(S, dtype=dtype) for S in Sigmas]
    mu = [np.asarray(m, dtype=dtype) for m in mus]
    s = [np.array(np.diag(S), dtype=dtype) for S in Sig]
    G = [np.zeros((n_select, M), dtype=dtype) for _ in range(nu)]
    picked, util, gaps, Ts, taus = [], [], [], [], [[] for _ in range(nu)]
    free = np.ones(M, dtype=bool)
    for t in range(n_select):
        if picked and picked[-1] < 0:
            picked.append(-1)
            util.append(np.nan)
            continue
        U = [utility_f64(dtype(As[u]) ** 2 * s[u], dtype(As[u]) * mu[u] + dtype(lambda0s[u])) for u in range(nu)]
        T = U[0] if weights is None else weights[0] * U[0]
        for u in range(1, nu):
            T = T + (U[u] if weights is None else weights[u] * U[u])
        Ts.append(T)
        ok = free & np.isfinite(T)
        if not ok.any():
            picked.append(-1)
            util.append(np.nan)
            continue
        cand = np.where(ok, T, -np.inf)
        i = int(np.argmax(cand))                      # the lowest index of the largest value
        rest = np.delete(cand, i)
        rest = rest[np.isfinite(rest)]
        gaps.append(float((cand[i] - rest.max()) / abs(cand[i])) if rest.size else np.inf)
        picked.append(i)
        util.append(float(T[i]))
        free[i] = False
        for u in range(nu):
            A = dtype(As[u])
            tau = 1 / (A * A * np.exp(A * mu[u][i] + A * A * s[u][i] / 2 + dtype(lambda0s[u])))
            v = s[u][i] + tau
            c = Sig[u][:, i] - G[u][:t].T @ G[u][:t, i]
            G[u][t] = c / np.sqrt(v)
            s[u] = s[u] - G[u][t] ** 2
            taus[u].append(tau)
    return {"picked": picked, "utility": util, "sigma2": s, "tau": taus, "gap": gaps, "T": Ts}


def greedy_reference(Sigmas, mus, As, lambda0s, weights, n_select):
    return greedy(Sigmas, mus, As, lambda0s, weights, n_select, LD)


def greedy_f64(Sigmas, mus, As, lambda0s, weights, n_select):
    return greedy(Sigmas, mus, As, lambda0s, weights, n_select, np.float64)


def exact_conditioning(Sigma, picks, tau):
    """diag(Sigma - Sigma[:, I] (Sigma[I, I] + diag(tau))^-1 Sigma[I, :]) by a dense np.longdouble solve."""
    Sigma = np.asarray(Sigma, dtype=LD)
    I = np.asarray(picks, dtype=int)
    Minv = cases.inv_spd_ld(Sigma[np.ix_(I, I)] + np.diag(np.asarray(tau, dtype=LD)))
    W = Sigma[:, I]
    return np.diag(Sigma) - ((W @ Minv) * W).sum(1)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def single_inputs(name):
    """(Sigma, mu) of a SINGLE case rounded to fp64: what the device, the transcription and the reference all start from."""
    Sigma, mu = sigma_longdouble(cases.make_case(*SINGLE[name][0]))
    return _frozen(np.asarray(Sigma, dtype=np.float64), np.asarray(mu, dtype=np.float64))


@functools.lru_cache(maxsize=None)
def single_reference(name):
    _, A, n_select = SINGLE[name]
    Sigma, mu = single_inputs(name)
    return greedy_reference([Sigma], [mu], [A], [LAMBDA0], None, n_select)


@functools.lru_cache(maxsize=None)
def unit_inputs(name):
    """Per unit (Sigma, mu) in fp64 for a UNITS case."""
    out = [sigma_longdouble(c) for c in groups.make_group(UNITS[name][0])]
    return tuple(_frozen(np.asarray(S, dtype=np.float64), np.asarray(m, dtype=np.float64)) for S, m in out)


@functools.lru_cache(maxsize=None)
def unit_reference(name):
    group, weights, n_select = UNITS[name]
    inp = unit_inputs(name)
    n = len(inp)
    return greedy_reference([S for S, _ in inp], [m for _, m in inp], [unit_A(u) for u in range(n)], [LAMBDA0] * n, weights, n_select)


@functools.lru_cache(maxsize=None)
def duplicate_case():
    """DUPLICATE_SHAPE's case with an exact copy and a near-copy among the pool's rows."""
    c = dict(cases.make_case(*DUPLICATE_SHAPE))
    xs = c["xstar"].copy()
    for row, copy, scale in DUPLICATES:
        xs[copy] = scale * xs[row]
    xs.setflags(write=False)
    c["xstar"] = xs
    return c


@functools.lru_cache(maxsize=None)
def duplicate_inputs():
    Sigma, mu = sigma_longdouble(duplicate_case())
    return _frozen(np.asarray(Sigma, dtype=np.float64), np.asarray(mu, dtype=np.float64))


@functools.lru_cache(maxsize=None)
def duplicate_reference():
    Sigma, mu = duplicate_inputs()
    return greedy_reference([Sigma], [mu], [1.0], [LAMBDA0], None, 8)


def top_b(T, b):
    """The b rows of largest T, lowest index first among equals (what the examples do without --batch-aware)."""
    return [int(i) for i in np.argsort(-np.asarray(T, dtype=np.float64), kind="stable")[:b]]
