"""CPU-side checks of the Cholesky test material (potrf_cases.py) and of the hook gpfit_dev_potrf's refusals: the plain
reference against LAPACK, its inverse, its info rule on the failing variants, the exact scaling and the correctly
rounded square roots it stands for -- and every comparison helper on a deliberately corrupted factor, so that the
helpers test_gpu_potrf.py relies on are known to be able to fail.  No call reaches a GPU here.

LAPACK is the second opinion for the factor and for the ``negative`` and ``zero`` variants (all 52 positions agree).
It is NOT one for the NaN variants: the dpotrf of this scipy / OpenBLAS returns info = 0 for a NaN pivot (seen at every
one of the 52 positions, NaN on and below the diagonal), so there the expectation is the rule of the header alone --
the first pivot with ``not (p > 0)``."""
import ctypes

import numpy as np
import pytest
from scipy.linalg import lapack

import potrf_cases as pc
from conftest import relerr
from gaussian_processes_amd import _lib
from gaussian_processes_amd.build import build_library

LD = pc.LD
N_INFO = 384 if pc.WIDE else 128
POSITIONS = tuple(j for j in pc.POSITIONS_384 if j < N_INFO)


@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _lib.load()


def lapack_info(A):
    return int(lapack.dpotrf(np.tril(A), lower=1)[1])


# ---- the reference
@pytest.mark.parametrize("n", [128, 256, 384] if pc.WIDE else [128])
def test_reference_factor_matches_lapack_and_its_inverse_inverts_it(n):
    A = pc.spd(n)
    assert np.linalg.cond(A) < 10
    ref = pc.reference(A)
    c, info = lapack.dpotrf(np.tril(A), lower=1)
    assert info == 0 and ref.info == 0
    e = relerr(np.asarray(ref.L, dtype=np.float64), np.tril(c))
    print(f"n {n}: reference against dpotrf {e:.2e}")
    assert e < 1e-13
    # longdouble forward substitution: n eps_ld cond(L) with eps_ld = 1.1e-19, cond(L) < sqrt(10)
    assert pc.err_inverse(ref.Linv, ref) < 1e-15
    assert pc.err_backward(ref.L, A) < 1e-17 if pc.WIDE else 1e-15
    assert abs(ref.logdet - np.linalg.slogdet(A)[1]) < 1e-12 * abs(ref.logdet)


def test_negative_and_zero_variants_fail_where_lapack_fails():
    A = pc.spd(N_INFO)
    L0 = pc.reference(A).L
    assert len(POSITIONS) == (52 if pc.WIDE else len(POSITIONS))
    for j in POSITIONS:
        for variant in ("negative", "zero"):
            B, want = pc.failing(A, variant, j, L0)
            assert want == j + 1
            got = pc.reference(B, want_inverse=False)
            assert got.info == want and got.L is None, (variant, j, got.info)
            assert lapack_info(B) == want, (variant, j)


def test_nan_variants_follow_the_rule_of_the_header():
    """The helper's rule only (see the module docstring: this LAPACK answers 0 for a NaN pivot)."""
    A = pc.spd(N_INFO)
    for j in POSITIONS:
        B, want = pc.failing(A, "nan_diag", j)
        assert want == j + 1 and pc.reference(B, want_inverse=False).info == want
        if pc.nan_row(N_INFO, j) is None:
            with pytest.raises(ValueError):
                pc.failing(A, "nan_below", j)
            continue
        B, want = pc.failing(A, "nan_below", j)
        i = pc.nan_row(N_INFO, j)
        assert want == i + 1 and i > j and np.isnan(B[i, j])
        assert pc.reference(B, want_inverse=False).info == want, j
    # the NaN does not leave its row: one column later the other pivots are still those of A
    j = 16
    B, want = pc.failing(A, "nan_below", j)
    B[want - 1, :] = A[want - 1, :]
    B[:, want - 1] = A[:, want - 1]
    assert pc.reference(B, want_inverse=False).info == 0


def test_two_bad_pivots_report_the_first():
    A = pc.spd(N_INFO)
    L0 = pc.reference(A).L
    for j in (3, 70):
        B, _ = pc.failing(A, "negative", j, L0)
        B[j + 40, j + 40] = -1.0
        assert pc.reference(B, want_inverse=False).info == j + 1 == lapack_info(B)


def test_scaling_by_a_power_of_four_is_exact_in_the_reference_and_in_lapack():
    A = pc.spd(128)
    ref = pc.reference(A)
    L0 = np.linalg.cholesky(A)
    for k in (-250, 250):
        As = pc.scaled(A, k)
        assert np.array_equal(np.ldexp(As, -2 * k), A)
        rs = pc.reference(As)
        assert rs.info == 0
        assert np.array_equal(rs.L, ref.L * LD(2.0) ** k) and np.array_equal(rs.Linv, ref.Linv * LD(2.0) ** -k)
        assert np.abs(np.ldexp(np.linalg.cholesky(As), -k) - L0).max() == 0.0


def test_diagonal_matrices_isolate_the_square_root():
    p = pc.sqrt_pivots()
    assert p.shape == (128,) and all(v in p for v in pc.SQRT_SPECIALS)
    assert p.min() == np.nextafter(1.0, 0.0) and p.max() == np.nextafter(4.0, 0.0)
    for k in (0, -250, 250):
        ps = p * np.ldexp(1.0, 2 * k)
        ref = pc.reference(pc.diagonal_matrix(ps))
        assert ref.info == 0
        assert np.count_nonzero(ref.L) == 128 and np.count_nonzero(ref.Linv) == 128
        # np.sqrt is correctly rounded: within half an ulp of the wide square root
        assert pc.ulp_error(np.sqrt(ps), np.diag(ref.L)).max() <= 0.5 + 1e-3
        assert pc.ulp_error(1.0 / np.sqrt(ps), np.diag(ref.Linv)).max() <= 1.5


# ---- the comparison helpers can fail
def test_helpers_reject_corrupted_factors():
    n = 128
    A = pc.spd(n)
    ref = pc.reference(A)
    L = np.asarray(ref.L, dtype=np.float64)
    Li = np.asarray(ref.Linv, dtype=np.float64)
    # the honest double-rounded factor passes the bounds test_gpu_potrf.py asserts ...
    assert pc.err_factor(L, ref) < 1e-12 and pc.err_inverse(Li, ref) < 1e-11 and pc.err_backward(L, A) <= 2e-14
    assert pc.upper_is_zero(L) and pc.upper_is_zero(L, 128) and pc.same_bits(L, L.copy())
    # ... one 16 x 16 tile transposed does not (a tile below the diagonal, and the diagonal tile of panel 3)
    for (r, c) in ((64, 16), (48, 48)):
        T = L.copy()
        T[r:r + 16, c:c + 16] = L[r:r + 16, c:c + 16].T.copy()
        assert pc.err_factor(T, ref) > 1e-3
        assert pc.err_backward(np.tril(T), A) > 1e-3
        Ti = Li.copy()
        Ti[r:r + 16, c:c + 16] = Li[r:r + 16, c:c + 16].T.copy()
        assert pc.err_inverse(Ti, ref) > 1e-3 and pc.err_product(Ti, L) > 1e-3
        assert not pc.same_bits(T, L)
    assert not pc.upper_is_zero(L + np.triu(np.full((n, n), 1e-300), 1))
    # one element a few ulp off: the forward bounds are tight enough to see 1e-12 relative
    T = L.copy()
    T[100, 3] += 2e-12 * np.abs(L).max()
    assert pc.err_factor(T, ref) > 1e-12 and not pc.same_bits(T, L)
    U = L.copy()
    U[3, 100] = np.nan
    assert not pc.upper_is_zero(U) and not pc.upper_is_zero(U, 128)
    U = L.copy()
    U[3, 100] = -0.0
    assert pc.upper_is_zero(U)
    assert not pc.same_bits(np.array([0.0]), np.array([-0.0]))
    # the scale argument is really applied
    assert pc.err_factor(L * 2.0 ** 250, ref, 2.0 ** 250) < 1e-12 < pc.err_factor(L * 2.0 ** 250, ref, 2.0 ** 249)
    # ulp distances: exact for neighbours, and a square root one Newton step short is far outside 2 ulp
    x = np.sqrt(np.array([2.0, 3.0]))
    exact = np.sqrt(np.array([2.0, 3.0], dtype=LD))
    three_up = np.nextafter(np.nextafter(np.nextafter(x, 9.0), 9.0), 9.0)
    assert pc.ulp_error(x, exact).max() <= 0.5 and 2.5 <= pc.ulp_error(three_up, exact).min() <= 3.5
    assert pc.ulp_error(x * (1 + 2.0 ** -27), exact).min() > 1e6


def test_info_off_by_one_is_seen():
    """The info comparison is an equality against the reference's info: a stand-in that counts pivots from 0, or that
    reports the last bad pivot instead of the first, differs at every position."""
    A = pc.spd(128)

    def counts_from_zero(B):       # the corrupted stand-in: the reference with info off by one
        return pc.reference(B, want_inverse=False).info - 1

    for variant in pc.VARIANTS:
        for j in (0, 15, 16, 90):
            B, want = pc.failing(A, variant, j)
            assert pc.reference(B, want_inverse=False).info == want
            assert counts_from_zero(B) != want
    B, want = pc.failing(A, "negative", 20)
    B[60, 60] = -1.0
    last_bad = 61
    assert pc.reference(B, want_inverse=False).info == want == 21 != last_bad


def test_top_block_follows_the_recursion_split():
    assert [pc.top_block(n) for n in (256, 384, 512, 640)] == [128, 256, 256, 384]


# ---- the hook's refusals: before the context or a buffer is read
def _arrays(nb, null_at=None):
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    arr = (ctypes.c_void_p * max(nb, 1))(*[p] * max(nb, 1))
    if null_at is not None:
        arr[null_at] = None
    return arr, buf


def _hook(lib, ctx="fake", is_f32=0, nb=2, ld=256, n=256, need=1, halves=0, side_min=0, null=None, null_entry=None):
    names = ("A", "L", "Li", "Tmp", "info")
    keep = []
    args = {}
    for k in names:
        arr, buf = _arrays(nb if 1 <= nb <= 32 else 1, null_at=(null_entry[1] if null_entry and null_entry[0] == k else None))
        keep.append((arr, buf))
        args[k] = None if null == k else arr
    fake = ctypes.cast((ctypes.c_double * 8)(), ctypes.c_void_p)
    rc = lib.gpfit_dev_potrf(fake if ctx == "fake" else ctx, None, is_f32, nb, args["A"], args["L"], args["Li"], args["Tmp"],
                             args["info"], ld, n, need, halves, side_min)
    return rc, lib.gpfit_last_error().decode()


def test_hook_is_declared_listed_and_exported(lib):
    assert "gpfit_dev_potrf" in _lib.exported_symbols() and hasattr(lib, "gpfit_dev_potrf")


@pytest.mark.parametrize("kw", [
    dict(ctx=None), dict(null="A"), dict(null="L"), dict(null="Li"), dict(null="Tmp"), dict(null="info"),
    dict(null_entry=("A", 1)), dict(null_entry=("Li", 0)), dict(null_entry=("info", 1)),
    dict(nb=0), dict(nb=-1), dict(nb=33),
    dict(n=0), dict(n=-128), dict(n=100), dict(n=129), dict(n=192, ld=192),
    dict(ld=255), dict(ld=128), dict(ld=257), dict(is_f32=1, ld=258), dict(is_f32=1, ld=257),
    dict(need=4), dict(need=0x80000000), dict(halves=4), dict(nb=1, need=2), dict(nb=31, need=0x80000000),
    dict(side_min=-1),
])
def test_hook_refuses_bad_arguments_before_anything_is_read(lib, kw):
    rc, msg = _hook(lib, **kw)
    assert rc == -3 and "gpfit_dev_potrf" in msg, kw
