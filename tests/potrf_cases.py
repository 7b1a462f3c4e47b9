"""Inputs, the plain reference and the comparison helpers shared by the tests of the Cholesky recursion
(test_potrf_cases_cpu.py checks this module; test_gpu_potrf.py checks potrf_lockstep and the 128 x 128 leaf with it).

``reference`` is the textbook column-by-column Cholesky in ``np.longdouble`` (64-bit mantissa on x86; where longdouble
is no wider than double it runs in mpmath at 80 digits and refuses n > 128), the inverse by forward substitution in
the same precision, and ``info`` by the rule of include/gpfit_mi355x.h: the 1-based index of the first pivot with
``not (p > 0)`` -- a NaN pivot included -- after which it stops.

Every input is seeded.  The SPD matrices ``M M^T / n + I`` have their spectrum in [1, 5], so forward errors mean
something.  The four failing variants of a matrix and what each must report are described at ``VARIANTS``."""
import functools

import numpy as np

LD = np.longdouble
WIDE = np.finfo(LD).nmant > np.finfo(np.float64).nmant
VARIANTS = ("negative", "zero", "nan_diag", "nan_below")
# the pivot positions the CPU test runs against LAPACK (n = 384): 52 of them, every panel edge of the first leaf's
# first panels and the edges of panels and leaves further on
POSITIONS_384 = tuple(range(0, 40)) + (111, 112, 127, 128, 129, 143, 144, 255, 256, 257, 300, 383)


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def spd(n, seed=0):
    """M M^T / n + I, M ~ N(0, 1): symmetric, eigenvalues in about [1, 5].  Read-only (shared)."""
    rng = np.random.default_rng(7919 * seed + n)
    M = rng.standard_normal((n, n))
    A = M @ M.T / n + np.eye(n)
    A = (A + A.T) / 2
    A.setflags(write=False)
    return A


def nan_row(n, j):
    """The row the ``nan_below`` variant poisons for pivot column j: 37 rows further down (another panel, often another
    leaf), the last row where that does not exist.  None for the last column, below which there is nothing."""
    return min(n - 1, j + 37) if j < n - 1 else None


def failing(A, variant, j, L0=None):
    """A copy of the SPD matrix A whose factorisation fails, and the info it must report.
      negative   A[j, j] -= 2 L0[j, j]^2 (L0: the factor of A): pivot j becomes about -L0[j, j]^2, the pivots before it
                 are untouched                                                                        info = j + 1
      zero       row and column j zeroed, the diagonal included: pivot j is exactly 0 in any summation order
                                                                                                      info = j + 1
      nan_diag   A[j, j] = nan                                                                        info = j + 1
      nan_below  A[i, j] = A[j, i] = nan, i = nan_row(n, j) > j: L[i, j] is NaN, which stays in row i of the factor
                 and in column i of the Schur complement until pivot i is reached                     info = i + 1"""
    n = A.shape[0]
    B = np.array(A, dtype=A.dtype)
    if variant == "negative":
        d = (np.asarray(reference(A).L if L0 is None else L0)[j, j]) ** 2
        B[j, j] -= B.dtype.type(2 * d)
        return B, j + 1
    if variant == "zero":
        B[j, :] = 0
        B[:, j] = 0
        return B, j + 1
    if variant == "nan_diag":
        B[j, j] = np.nan
        return B, j + 1
    if variant == "nan_below":
        i = nan_row(n, j)
        if i is None:
            raise ValueError("nan_below: no row below the last column")
        B[i, j] = B[j, i] = np.nan
        return B, i + 1
    raise ValueError(variant)


SQRT_SPECIALS = (1.0, 2.0, float(np.nextafter(1.0, 0.0)), float(np.nextafter(1.0, 2.0)), float(np.nextafter(4.0, 0.0)),
                 3.0, 9.0 / 4.0)


@functools.lru_cache(maxsize=None)
def sqrt_pivots():
    """128 pivots for the leaf's square root: log-spaced over [1, 4) (every binade parity of the exponent once), with
    seven of them replaced by exact squares, the neighbours of 1 and 4, and plain values.  (nextafter(1, 0) lies just
    below the interval: the mantissa of all ones.)"""
    p = 4.0 ** (np.arange(128) / 128.0)
    for k, v in enumerate(SQRT_SPECIALS):
        p[5 + 17 * k] = v
    p.setflags(write=False)
    return p


def diagonal_matrix(p):
    """diag(p): every Schur update of its factorisation is exactly zero, so L_ii is the square-root routine alone."""
    return np.diag(np.asarray(p, dtype=np.float64))


def scaled(A, k):
    """A 4^k, exact in binary floating point: the factor scales by exactly 2^k, the inverse by 2^-k."""
    return A * np.ldexp(1.0, 2 * k)


# ------------------------------------------------------------------ the reference
class Ref:
    """L, Linv (longdouble, or None after a failure), logdet (float), info (int)."""
    def __init__(self, L, Linv, logdet, info):
        self.L, self.Linv, self.logdet, self.info = L, Linv, logdet, info


def _reference_longdouble(A, want_inverse):
    n = A.shape[0]
    A = np.asarray(A, dtype=LD)
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        row = L[j, :j]
        p = A[j, j] - row @ row
        if not (p > 0):
            return Ref(None, None, float("nan"), j + 1)
        d = np.sqrt(p)
        L[j, j] = d
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ row) / d
    Li = None
    if want_inverse:
        Li = np.zeros((n, n), dtype=LD)
        for i in range(n):
            r = -(L[i, :i] @ Li[:i, :])
            r[i] += 1
            Li[i, :] = r / L[i, i]
    return Ref(L, Li, float(2 * np.sum(np.log(np.diag(L)))), 0)


def _reference_mpmath(A, want_inverse):
    import mpmath
    n = A.shape[0]
    if n > 128:
        raise ValueError("the mpmath reference is kept to n <= 128")
    with mpmath.workdps(80):
        a = [[mpmath.mpf(float(A[i, j])) for j in range(n)] for i in range(n)]
        L = [[mpmath.mpf(0)] * n for _ in range(n)]
        for j in range(n):
            p = a[j][j] - mpmath.fsum(L[j][k] ** 2 for k in range(j))
            if not (p > 0):
                return Ref(None, None, float("nan"), j + 1)
            L[j][j] = mpmath.sqrt(p)
            for i in range(j + 1, n):
                L[i][j] = (a[i][j] - mpmath.fsum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]
        Li = None
        if want_inverse:
            Li = [[mpmath.mpf(0)] * n for _ in range(n)]
            for i in range(n):
                for c in range(i + 1):
                    s = (1 if c == i else 0) - mpmath.fsum(L[i][k] * Li[k][c] for k in range(c, i))
                    Li[i][c] = s / L[i][i]
        logdet = float(2 * mpmath.fsum(mpmath.log(L[i][i]) for i in range(n)))
        to = lambda X: np.array([[float(v) for v in r] for r in X], dtype=LD)
        return Ref(to(L), to(Li) if want_inverse else None, logdet, 0)


def reference_uncached(A, want_inverse=True):
    A = np.asarray(A)
    return _reference_longdouble(A, want_inverse) if WIDE else _reference_mpmath(A, want_inverse)


_CACHE = {}


def reference(A, want_inverse=True):
    """The reference of a matrix, computed once per matrix content (the tests share it and leave it unchanged)."""
    A = np.ascontiguousarray(A)
    key = (A.shape, A.dtype.str, A.tobytes())
    hit = _CACHE.get(key)
    if hit is None or (want_inverse and hit.info == 0 and hit.Linv is None):
        hit = reference_uncached(A, want_inverse)
        for X in (hit.L, hit.Linv):
            if X is not None:
                X.setflags(write=False)
        _CACHE[key] = hit
    return hit


# ------------------------------------------------------------------ comparison helpers (every one of them can fail:
# test_potrf_cases_cpu.py feeds each a corrupted factor)
def _max(X):
    return float(np.max(np.abs(X)))


def err_factor(L, ref, scale=1.0):
    """max |L - scale L_ref| / max |scale L_ref| over the lower triangle (conftest.relerr's measure)."""
    Lr = np.tril(ref.L) * LD(scale)
    return float(np.max(np.abs(np.tril(np.asarray(L, dtype=LD)) - Lr)) / np.max(np.abs(Lr)))


def err_inverse(Li, ref, scale=1.0):
    """max |Li (scale L_ref) - I|: the inverse against the reference FACTOR (the identity's largest entry is 1)."""
    n = ref.L.shape[0]
    P = np.tril(np.asarray(Li, dtype=LD)) @ (np.tril(ref.L) * LD(scale))
    return float(np.max(np.abs(P - np.eye(n, dtype=LD))))


def err_backward(L, A):
    """max |L L^T - A| / max |A| over the lower triangle (the strict upper part of A may hold anything)."""
    L = np.tril(np.asarray(L, dtype=LD))
    R = np.tril(L @ L.T - np.asarray(A, dtype=LD))
    return float(np.max(np.abs(R)) / np.max(np.abs(np.tril(np.asarray(A, dtype=LD)))))


def err_product(Li, L):
    """max |Li L - I| of a computed pair (what test_gpu_stability.py measures)."""
    n = L.shape[0]
    P = np.tril(np.asarray(Li, dtype=LD)) @ np.tril(np.asarray(L, dtype=LD))
    return float(np.max(np.abs(P - np.eye(n, dtype=LD))))


def upper_is_zero(X, block=None):
    """True when the strict upper triangle of X -- with ``block``: of every block x block diagonal block of X, the part
    the leaf writes -- is exactly 0.0 (no NaN, no negative-zero exception: -0.0 == 0.0)."""
    X = np.asarray(X)
    n = X.shape[0]
    if block is None:
        return bool(np.all(X[np.triu_indices(n, 1)] == 0.0))
    return all(upper_is_zero(X[r:r + block, r:r + block]) for r in range(0, n, block))


def same_bits(X, Y):
    """Bit-for-bit equality of two arrays of the same type and shape (NaNs with equal payload are equal, 0.0 != -0.0)."""
    X, Y = np.ascontiguousarray(X), np.ascontiguousarray(Y)
    return X.shape == Y.shape and X.dtype == Y.dtype and X.tobytes() == Y.tobytes()


def ulp_error(x, exact):
    """|x - exact| in units of the spacing of float64 at the correctly rounded ``exact`` (a longdouble array)."""
    exact = np.asarray(exact, dtype=LD)
    ulp = np.spacing(np.abs(exact).astype(np.float64)).astype(LD)
    return np.abs(np.asarray(x, dtype=LD) - exact) / ulp


def top_block(n, tile=128):
    """Rows of the top block of potrf_lockstep's split of an n x n node: ceil(k / 2) of its k tiles."""
    k = n // tile
    return ((k + 1) // 2) * tile
