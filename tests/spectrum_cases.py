"""Symmetric positive definite matrices with a DESIGNED spectrum, for the one discrete decision of a fit: how many
eigenvalues of K~ lie above ``max(lambda_1 tol, tol)`` (test_spectrum_cases_cpu.py checks this module and runs it
through ``eigtop`` on CPU stand-ins; test_gpu_basis_spectra.py runs it through ``utils._stabilised_basis``).

``K = Q diag(lambda) Q^T`` (symmetrised) with ``Q`` orthogonal, so the truth is the design and no solver: the kept count
is ``#{lambda_i > tau}``, ``tau = max(lambda_1 tol, tol)``, and the kept space is spanned by the matching columns of Q.
Every input is seeded, nothing here imports torch or the library.

The spectra
  decay     ``lambda_i = lam1 (1 + i)^-2 + floor`` (i = 0 ...): the smooth decay through the threshold of the fit's own
            kernel matrices, on which the routes were built -- then bent where they were not tried:
              * the TOP CLUSTER: ``lambda_2 = rho lambda_1`` (rho = 0.5, 0.9, 0.99, 0.999), an exactly double or triple
                top eigenvalue, or the triple with one member at ``lambda_1 (1 - 1e-6)``;
              * the eigenvalue nearest the threshold moved to ``tau (1 + delta)``: kept for delta > 0, dropped for
                delta < 0, whatever |delta| is;
              * ``lam1 < 1``: the threshold is the floor ``tol`` itself, not ``lambda_1 tol``.
  count     a kept count chosen to the unit (the block of the subspace iteration starts at ``k0 = 128`` columns):
            log-spaced from lambda_1 down to 1.3 tau, one eigenvalue at ``tau (1 + delta)``, the rest from 0.7 tau down.
  plateau   lambda_1, then 145 equal eigenvalues at 1.05 tau, everything else at 0.5 tau and below.
  all kept  ``linspace(1, 2)``: nothing is dropped.

``Q`` is the orthogonal factor of a seeded Gaussian matrix, or (``q = "householder"``) the ORTHOGONAL-START
construction: one Householder reflector H that swaps the first coordinate axis with a unit vector w spread evenly over
the even coordinates from 2 up.  H is symmetric and orthogonal and leaves the second axis alone, so ``K = H diag(lambda) H``
has the top eigenvector w, the eigenvector e_1 for ``lambda_2 = 0.9 lambda_1``, its largest diagonal entry at (1, 1) and
column 1 equal to ``lambda_2 e_1`` to the bit: a power iteration started from the column of the largest diagonal entry
starts on an eigenvector that is exactly orthogonal to the top one.

Classes (what a caller may do with a case)
  MUST_DECIDE  an answer, and its count is the design's;
  NEVER_WRONG  any answer has the design count, declining (``None``) is allowed;
  AMBIGUOUS    |delta| = 1e-10: declining is allowed, an answer has the design count or differs from it by the one
               moved eigenvalue.
``cls`` is the class for ``top_eigenpairs`` (MUST_DECIDE: |delta| >= 1e-3 and rho <= 0.99 or an exact multiple top),
``cls_dense`` the one for ``kept_eigenspace_dense`` and for ``_kept_subspace`` on the matrix itself (narrower:
rho <= 0.9 or an exact multiple).  NEVER_WRONG starts at |delta| = 1e-6, a hundred times the 1e-8 to which the
solver's lambda_max, and so its tau, is certified.  ``extent`` says what the block iteration can do with the count:
``"fits"``, ``"too_wide"`` (more is kept than the largest block holds: ``top_eigenpairs`` must decline) or ``"all"``
(nothing is dropped: ``top_eigenpairs`` must decline, the dense route must report it)."""
import functools
from dataclasses import dataclass

import numpy as np

MUST_DECIDE, NEVER_WRONG, AMBIGUOUS = "MUST_DECIDE", "NEVER_WRONG", "AMBIGUOUS"
TOPS = ("rho0.5", "rho0.9", "rho0.99", "rho0.999", "double", "triple", "triple_near")
_RHO = {"rho0.5": 0.5, "rho0.9": 0.9, "rho0.99": 0.99, "rho0.999": 0.999}
DELTAS = tuple(s * d for d in (1e-2, 1e-3, 5e-4, 1e-5, 1e-6, 1e-10) for s in (1.0, -1.0))
K0 = 128                      # the start block of the CPU tests


@dataclass(frozen=True)
class Case:
    name: str
    n: int
    tol: float
    lam: np.ndarray           # descending, read-only
    count: int
    delta: float
    top: str
    cls: str
    cls_dense: str
    q: str = "qr"
    extent: str = "fits"
    moved: int = -1           # index of the eigenvalue that was put at tau (1 + delta); -1: none

    @property
    def tau(self):
        return max(float(self.lam[0]) * self.tol, self.tol)

    def Q(self):
        return orthogonal(self.n, self.q)

    def K(self):
        """Q diag(lambda) Q^T, symmetrised (a new array)."""
        Q = self.Q()
        K = (Q * self.lam) @ Q.T
        return (K + K.T) * 0.5

    def kept_columns(self):
        """The design's kept eigenvectors [n, count]."""
        return self.Q()[:, :self.count]

    def gap(self):
        """lambda_count - lambda_{count+1}: what the kept space is conditioned by (inf when nothing is dropped)."""
        return float(self.lam[self.count - 1] - self.lam[self.count]) if self.count < self.n else float("inf")


# ------------------------------------------------------------------ the orthogonal factors
@functools.lru_cache(maxsize=None)
def orthogonal(n, kind="qr"):
    """Read-only (shared).  ``qr``: of a seeded Gaussian; ``householder``: the orthogonal-start reflector (see above)."""
    if kind == "qr":
        Q, _ = np.linalg.qr(np.random.default_rng(104729 + n).standard_normal((n, n)))
    elif kind == "householder":
        w = np.zeros(n)
        w[2::2] = 1.0
        w /= np.linalg.norm(w)
        u = -w
        u[0] = 1.0                                   # u = e_0 - w, u^T u = 2
        Q = np.eye(n) - np.outer(u, u)
    else:
        raise ValueError(kind)
    Q.setflags(write=False)
    return Q


# ------------------------------------------------------------------ the spectra
def _classes(top, delta):
    if abs(delta) < 1e-6:
        return AMBIGUOUS, AMBIGUOUS
    if abs(delta) < 1e-3:
        return NEVER_WRONG, NEVER_WRONG
    exact = top in ("double", "triple")
    rho = _RHO.get(top)
    return (MUST_DECIDE if exact or (rho is not None and rho <= 0.99) else NEVER_WRONG,
            MUST_DECIDE if exact or (rho is not None and rho <= 0.9) else NEVER_WRONG)


def _set_top(lam, top):
    if top in _RHO:
        lam[1] = _RHO[top] * lam[0]
    elif top == "double":
        lam[1] = lam[0]
    elif top in ("triple", "triple_near"):
        lam[1] = lam[2] = lam[0]
        if top == "triple_near":
            lam[2] = lam[0] * (1.0 - 1e-6)
    else:
        raise ValueError(top)


def _finish(name, n, tol, lam, delta, top, q="qr", extent="fits", moved=-1, classes=None):
    assert np.all(np.diff(lam) <= 0), name
    tau = max(lam[0] * tol, tol)
    count = int((lam > tau).sum())
    lam = np.array(lam)
    lam.setflags(write=False)
    cls, cls_dense = classes or _classes(top, delta)
    case = Case(name, n, tol, lam, count, delta, top, cls, cls_dense, q, extent, moved)
    # the kept space stays well determined however close the moved eigenvalue is to the threshold
    assert case.gap() >= 1e-2 * tau, (name, case.gap() / tau)
    return case


def decay(n, top, delta, tol=1e-3, lam1=1e4, q="qr", tag=None):
    """The decaying spectrum with the top cluster ``top`` and the eigenvalue nearest tau at ``tau (1 + delta)``."""
    lam = lam1 * (1.0 + np.arange(n)) ** -2.0 + 1e-7 * lam1
    _set_top(lam, top)
    tau = max(lam[0] * tol, tol)
    j = int(np.argmin(np.abs(lam - tau)))
    lam[j] = tau * (1.0 + delta)
    branch = "rel" if lam1 * tol > tol else "floor"
    return _finish(tag or f"{branch}-{q}-n{n}-{top}-d{delta:+.0e}", n, tol, lam, delta, top, q=q, moved=j)


def counted(n, count, tol=1e-3, lam1=1e4, extent="fits"):
    """Exactly ``count`` kept: log-spaced down to 1.3 tau, the last kept one at 1.01 tau, the rest from 0.7 tau down."""
    tau = lam1 * tol
    lam = np.concatenate([np.geomspace(lam1, 1.3 * tau, count - 1), [1.01 * tau],
                          0.7 * tau * (1.0 + np.arange(n - count)) ** -2.0 + 1e-4 * tau])
    rho = lam[1] / lam[0]                           # 0.95 at count = 127, 0.98 at 400: a clustered top of its own
    return _finish(f"count{count}-n{n}", n, tol, lam, 1e-2, "geom", extent=extent, moved=count - 1,
                   classes=(MUST_DECIDE if rho <= 0.99 else NEVER_WRONG, MUST_DECIDE if rho <= 0.9 else NEVER_WRONG))


def plateau(n, width=145, tol=1e-3, lam1=1e4):
    tau = lam1 * tol
    lam = np.concatenate([[lam1], np.full(width, 1.05 * tau), 0.5 * tau / (1.0 + np.arange(n - width - 1))])
    return _finish(f"plateau{width}-n{n}", n, tol, lam, 5e-2, "single", classes=(MUST_DECIDE, MUST_DECIDE))


def all_kept(n, tol=1e-3):
    return _finish(f"allkept-n{n}", n, tol, np.linspace(2.0, 1.0, n), 1.0, "linear", extent="all",
                   classes=(MUST_DECIDE, MUST_DECIDE))


# ------------------------------------------------------------------ the table
@functools.lru_cache(maxsize=None)
def table(n=600):
    """The cases of one size: every pair of top cluster and delta on the relative branch; the floor branch with and
    without a cluster; the orthogonal start; the extents of the block (for ``K0``); all kept."""
    cases = [decay(n, top, d) for top in TOPS for d in DELTAS]
    cases += [decay(n, top, d, lam1=0.5) for top in ("rho0.5", "rho0.9") for d in (1e-3, -1e-3, 1e-6, -1e-6)]
    cases += [decay(n, "rho0.9", d, q="householder") for d in (1e-2, -5e-4, -1e-6)]
    kmax = (2 * n) // 3 // 128 * 128                # the largest block top_eigenpairs iterates on below n = 2048
    cases += [counted(n, c) for c in (K0 - 1, K0, K0 + 1)]
    cases += [plateau(n), counted(n, kmax + 16, extent="too_wide"), all_kept(n)]
    assert kmax + 16 > n // 3 and len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def cpu_cases():
    """n = 600 (padded to 608 inside the solvers) in full, and the multiple of 16 next to it for one case of each kind."""
    small = [decay(608, "rho0.9", -5e-4), decay(608, "double", 1e-3), decay(608, "rho0.5", -1e-3, lam1=0.5),
             decay(608, "rho0.9", -5e-4, q="householder"), counted(608, K0 + 1), all_kept(608)]
    return table(600) + tuple(small)


def gpu_cases(n):
    """What the device runs at size ``n``: every case of ``table(n)`` that is not AMBIGUOUS (87 of its 101)."""
    return tuple(c for c in table(n) if AMBIGUOUS not in (c.cls, c.cls_dense))
