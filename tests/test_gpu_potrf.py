"""The Cholesky recursion (fit.hip:potrf_lockstep) and its 128 x 128 register-resident leaf (chol_leaf_reg.hip) against
the plain longdouble reference of potrf_cases.py, element by element: through the hook gpfit_dev_potrf (fp64 and fp32;
the `need` and `halves` masks, chain batches, the look-ahead side stream, the info word of every pivot of a leaf, the
leaf's square root on its own) and through the public gpfit_potrf (padded sizes, strided layouts, failures and the call
after a failure).  Sizes: 128 (one leaf), 256 (one split), 384 (ragged 256 + 128), 640 (five leaves, three levels), 512
for the side stream only.  Every case is a few launches of milliseconds; the references are computed once per matrix
and shared (potrf_cases.reference).

Bounds.  fp64 forward errors are those test_gpu_dropin.py asserts for the same quantities (L: 1e-12, Linv L_ref - I:
1e-11), the backward error that of test_gpu_stability.py (2e-14 |A|max).  fp32 has no number of its own in the project:
the kernel is held to 10 x the error LAPACK's spotrf / strtri make on the same matrix, computed at run time (the slack
test_gpu_stability.py takes over LAPACK).  Bit identity is asserted as such, never as a tolerance."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.linalg import lapack

import potrf_cases as pc

pytestmark = pytest.mark.gpu
LD = pc.LD
SENTINEL = -777.25


class Device:
    """The two entry points on device buffers of this test's own; numpy in, numpy out."""

    def __init__(self):
        from gaussian_processes_amd import _lib, utils
        self.lib = _lib.load()
        self.last_error = _lib.last_error
        self.ctx = utils.get_engine(640, 1)._ctx
        self.stream = utils._stream

    def hook(self, mats, need=None, halves=0, side_min=0, lower_only=False, dtype=np.float64, pad=0):
        """gpfit_dev_potrf on a batch of equally sized matrices with ld = n + pad.  need: bit mask (default: every chain).
        lower_only: the strict upper triangle of every A is NaN.  L, Li, Tmp and the pad columns of A are prefilled with
        NaN, the info words with 0.  Returns (L[nb, n, ld], Li[nb, n, ld], info[nb])."""
        nb, n = len(mats), mats[0].shape[0]
        A = np.full((nb, n, n + pad), np.nan, dtype=dtype)
        A[:, :, :n] = np.stack([np.asarray(M, dtype=dtype) for M in mats])
        if lower_only:
            A[:, np.triu_indices(n, 1)[0], np.triu_indices(n, 1)[1]] = np.nan
        tdt = torch.float32 if dtype == np.float32 else torch.float64
        dA = torch.from_numpy(A).cuda()
        dL, dLi, dT = (torch.full((nb, n, n + pad), float("nan"), dtype=tdt, device="cuda") for _ in range(3))
        dinfo = torch.zeros(nb, dtype=torch.int32, device="cuda")
        ptrs = lambda t: (ctypes.c_void_p * nb)(*[t[b].data_ptr() for b in range(nb)])
        if need is None:
            need = (1 << nb) - 1
        rc = self.lib.gpfit_dev_potrf(self.ctx, self.stream(), int(dtype == np.float32), nb, ptrs(dA), ptrs(dL), ptrs(dLi),
                                      ptrs(dT), ptrs(dinfo), n + pad, n, need, halves, side_min)
        assert rc == 0, self.last_error()
        torch.cuda.synchronize()
        return dL.cpu().numpy(), dLi.cpu().numpy(), dinfo.cpu().numpy()

    def public(self, A, want_inverse=True, pads=(3, 5, 1)):
        """gpfit_potrf on the lower triangle of A with lda = n + 3, ldl = n + 5, ldi = n + 1; the strict upper triangle and
        the padding columns of A are NaN, the outputs prefilled with SENTINEL.
        Returns (rc, L[n, ldl], Li[n, ldi] or None, logdet, info, message)."""
        n = A.shape[0]
        lda, ldl, ldi = (n + p for p in pads)
        buf = np.full((n, lda), np.nan)
        buf[:, :n] = np.where(np.tril(np.ones((n, n), dtype=bool)), A, np.nan)
        dA = torch.from_numpy(buf).cuda()
        dL = torch.full((n, ldl), SENTINEL, dtype=torch.float64, device="cuda")
        dLi = torch.full((n, ldi), SENTINEL, dtype=torch.float64, device="cuda") if want_inverse else None
        logdet, info = ctypes.c_double(np.nan), ctypes.c_int(-9)
        rc = self.lib.gpfit_potrf(self.ctx, self.stream(), dA.data_ptr(), lda, n, dL.data_ptr(), ldl,
                                  dLi.data_ptr() if want_inverse else None, ldi if want_inverse else 0,
                                  ctypes.byref(logdet), ctypes.byref(info))
        msg = self.last_error() if rc != 0 else ""
        torch.cuda.synchronize()
        return rc, dL.cpu().numpy(), (dLi.cpu().numpy() if want_inverse else None), logdet.value, info.value, msg


@pytest.fixture(scope="module")
def dev():
    return Device()


def err_inverse_block(Li, ref, r0, r1):
    """max |Li[r0:r1, r0:r1] L_ref[r0:r1, r0:r1] - I|: a diagonal block of L^-1 is the inverse of that block of L."""
    P = np.tril(np.asarray(Li[r0:r1, r0:r1], dtype=LD)) @ np.tril(ref.L[r0:r1, r0:r1])
    return float(np.max(np.abs(P - np.eye(r1 - r0, dtype=LD))))


def check_fp64_factor(L, Li, A, ref, scale=1.0, what="", block=128):
    """The fp64 bounds of the module docstring, and exact zeros in the strict upper triangle of every diagonal
    block x block block (the part the recursion writes; None: of the whole matrix)."""
    eL, eI, eB = pc.err_factor(L, ref, scale), pc.err_inverse(Li, ref, scale), pc.err_backward(L, A)
    print(f"{what}: L {eL:.2e} (1e-12)  Linv L_ref - I {eI:.2e} (1e-11)  |L L^T - A| / |A| {eB:.2e} (2e-14)")
    assert eL < 1e-12, what
    assert eI < 1e-11, what
    assert eB <= 2e-14, what
    assert pc.upper_is_zero(L, block), what
    assert pc.upper_is_zero(Li, block), what


# ------------------------------------------------------------------ the hook, fp64
@pytest.mark.parametrize("n,pad", [(128, 0), (256, 0), (384, 2), (640, 0)])
def test_every_element_of_the_factor_and_its_inverse(dev, n, pad):
    """need = 1 on one chain whose strict upper triangle is NaN (only the lower triangle is the input): every element of
    L and L^-1 against the reference, the backward error, and exact zeros above the diagonal of every block written.
    At n = 384 the leading dimension is n + 2 (the smallest step the 16-byte rule allows; n itself at 384 runs in the
    need = 0 test below): the columns beyond n stay as they were."""
    A = pc.spd(n)
    ref = pc.reference(A)
    L, Li, info = dev.hook([A], lower_only=True, pad=pad)
    assert info[0] == 0 == ref.info
    assert np.all(np.isnan(L[0][:, n:])) and np.all(np.isnan(Li[0][:, n:]))
    L, Li = L[0][:, :n], Li[0][:, :n]
    check_fp64_factor(L, Li, A, ref, what=f"n {n} ld {n + pad}")
    assert np.all(np.isfinite(np.tril(L))) and np.all(np.isfinite(np.tril(Li)))


@pytest.mark.parametrize("n", [256, 384, 640])
def test_without_the_full_inverse_the_factor_has_the_same_bits(dev, n):
    """need = 0 (the Linv == NULL route of gpfit_potrf) and need = 0 with halves = 1 (the block-wise callers): the same L
    bit for bit; Li holds the inverse of the top block, with halves that of both diagonal half blocks.  The block that
    is documented as not formed ([L^-1]21) is not looked at."""
    A = pc.spd(n)
    ref = pc.reference(A)
    n1 = pc.top_block(n)
    L1, _, info1 = dev.hook([A])
    L0, Li0, info0 = dev.hook([A], need=0)
    Lh, Lih, infoh = dev.hook([A], need=0, halves=1)
    assert info1[0] == info0[0] == infoh[0] == 0
    assert pc.err_factor(L1[0], ref) < 1e-12
    assert pc.same_bits(np.tril(L0[0]), np.tril(L1[0])) and pc.same_bits(np.tril(Lh[0]), np.tril(L1[0]))
    e_top, e_h1, e_h2 = (err_inverse_block(Li0[0], ref, 0, n1), err_inverse_block(Lih[0], ref, 0, n1),
                         err_inverse_block(Lih[0], ref, n1, n))
    print(f"n {n}: top block {e_top:.2e}, halves {e_h1:.2e} {e_h2:.2e} (1e-11)")
    assert e_top < 1e-11 and e_h1 < 1e-11 and e_h2 < 1e-11


@pytest.fixture(scope="module")
def solo256(dev):
    """Chain b of the chain tests run alone (nb = 1, full inverse), once."""
    out = {}

    def get(b, dtype=np.float64):
        if (b, dtype) not in out:
            L, Li, info = dev.hook([pc.spd(256, seed=b)], dtype=dtype)
            assert info[0] == 0
            out[(b, dtype)] = (np.tril(L[0]), np.tril(Li[0]))
        return out[(b, dtype)]
    return get


@pytest.mark.parametrize("nb", [2, 5, 32])
def test_a_chain_has_the_same_bits_alone_and_in_any_batch(dev, solo256, nb):
    """The invariant fit.hip states above potrf_lockstep: every chain of a batch of different matrices gets the L and
    L^-1 it gets alone, bit for bit."""
    L, Li, info = dev.hook([pc.spd(256, seed=b) for b in range(nb)])
    assert not info.any()
    for b in range(nb):
        Ls, Lis = solo256(b)
        assert pc.same_bits(np.tril(L[b]), Ls), f"L of chain {b} of {nb}"
        assert pc.same_bits(np.tril(Li[b]), Lis), f"Linv of chain {b} of {nb}"
    if nb == 2:   # and the bits are right
        ref = pc.reference(pc.spd(256, seed=1))
        check_fp64_factor(L[1], Li[1], pc.spd(256, seed=1), ref, what="chain 1 of 2")


def test_chains_outside_the_need_mask_keep_their_bits(dev, solo256):
    """need on a strict subset (0b10101 of five): every chain's L as alone, the chains of the mask their whole inverse
    as alone, the others the inverse of their top block."""
    mask = 0b10101
    L, Li, info = dev.hook([pc.spd(256, seed=b) for b in range(5)], need=mask)
    assert not info.any()
    for b in range(5):
        Ls, Lis = solo256(b)
        assert pc.same_bits(np.tril(L[b]), Ls), f"L of chain {b}"
        if mask >> b & 1:
            assert pc.same_bits(np.tril(Li[b]), Lis), f"Linv of chain {b}"
        else:
            assert err_inverse_block(Li[b], pc.reference(pc.spd(256, seed=b)), 0, 128) < 1e-11


def test_side_stream_does_not_change_a_bit(dev):
    """n = 512 with the first merge product of the top node on the side stream (side_min = 256: the top node and both
    256-nodes) against the one-stream form: the same products in another place."""
    A = pc.spd(512)
    L0, Li0, info0 = dev.hook([A], side_min=0)
    L1, Li1, info1 = dev.hook([A], side_min=256)
    assert info0[0] == 0 and info1[0] == 0
    check_fp64_factor(L0[0], Li0[0], A, pc.reference(A), what="n 512 one stream")
    assert pc.same_bits(np.tril(L1[0]), np.tril(L0[0]))
    assert pc.same_bits(np.tril(Li1[0]), np.tril(Li0[0]))


# ---- info
def test_info_of_every_pivot_of_a_leaf(dev):
    """n = 128, 32 chains per launch, four launches: chain b of launch l fails at pivot 32 l + b (negative variant), so
    every pivot of every panel is the first bad one once.  Then 31 failing chains beside one clean chain, which reports
    0 and has the bits of its solo run."""
    A = pc.spd(128)
    ref = pc.reference(A)
    clean_L, clean_Li, _ = dev.hook([A])
    for launch in range(4):
        mats, want = [], []
        for b in range(32):
            B, w = pc.failing(A, "negative", 32 * launch + b, ref.L)
            assert pc.reference(B, want_inverse=False).info == w
            mats.append(B)
            want.append(w)
        _, _, info = dev.hook(mats)
        assert info.tolist() == want, f"launch {launch}"
        clean = (7 * launch + 3) % 32
        mats[clean], want[clean] = A, 0
        L, Li, info = dev.hook(mats)
        assert info.tolist() == want, f"launch {launch} with a clean chain at {clean}"
        assert pc.same_bits(np.tril(L[clean]), np.tril(clean_L[0])) and pc.same_bits(np.tril(Li[clean]), np.tril(clean_Li[0]))


POSITIONS_384 = (0, 15, 16, 17, 127, 128, 129, 143, 255, 256, 257, 383)


@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_info_across_panels_and_leaves(dev, variant):
    """n = 384 (three leaves, info_base 0 / 128 / 256), twelve positions on both sides of every panel and leaf edge, one
    chain each in one launch.  After the first bad pivot (replaced by 1) later pivots go bad too: the first one wins.
    nan_below has no case at the last column (there is no row below it)."""
    A = pc.spd(384)
    L0 = pc.reference(A).L
    mats, want = [], []
    for j in POSITIONS_384:
        if variant == "nan_below" and pc.nan_row(384, j) is None:
            continue
        B, w = pc.failing(A, variant, j, L0)
        assert pc.reference(B, want_inverse=False).info == w
        mats.append(B)
        want.append(w)
    _, _, info = dev.hook(mats)
    assert info.tolist() == want


def test_two_bad_pivots_report_the_first(dev):
    A = pc.spd(384)
    L0 = pc.reference(A).L
    mats, want = [], []
    for j in (0, 100, 120, 250, 343):      # the second one in the same leaf, in the next leaf, in the last panel
        B, w = pc.failing(A, "negative", j, L0)
        B[j + 40, j + 40] = -1.0
        assert pc.reference(B, want_inverse=False).info == w == j + 1
        mats.append(B)
        want.append(w)
    _, _, info = dev.hook(mats)
    assert info.tolist() == want


# ---- the square root of the leaf
# Largest error of Linv_ii = y (v_rsq_f64 and one Newton step, rl_rsqrt_sqrt) against 1 / sqrt(p) in longdouble over the
# 3 x 128 pivots of test_square_root_of_the_leaf, in ulp of the correctly rounded value.  MEASURED on the MI355X
# (2026-10-20), not derived: 6.427 ulp, at p = 3.668016172818685 and at its two scaled copies alike (the error depends on
# the mantissa only); the project records the accuracy of v_rsq_f64 nowhere (6.4 ulp after one Newton step puts it near
# 2^-25.4).  Asserted with a factor of 4 for the mantissas not sampled.  L_ii on the same run: equal to np.sqrt(p) at all
# 384 pivots.
LINV_DIAG_ULP_MEASURED = 6.43


def test_square_root_of_the_leaf(dev):
    """Diagonal matrices: every Schur update is exactly zero, so L_ii is rl_rsqrt_sqrt's root and Linv_ii its reciprocal
    root, alone.  128 pivots over [1, 4) with the exact squares and the neighbours of 1 and 4, and their copies scaled by
    4^250 and 4^-250.
      L_ii: within 2 ulp of the correctly rounded np.sqrt(p).  The last step d + fma(-d, d, p) y / 2 is a Newton step
        with an exact residual: within 1 ulp for any y good to about 2^-27, one more for the rounding of the correction.
      Linv_ii: within 4 x LINV_DIAG_ULP_MEASURED (see there) of 1 / sqrt(p)."""
    p = pc.sqrt_pivots()
    ks = (0, 250, -250)
    ps = [p * np.ldexp(1.0, 2 * k) for k in ks]
    L, Li, info = dev.hook([pc.diagonal_matrix(q) for q in ps])
    assert not info.any()
    worst = 0.0
    for k, q, Lk, Lik in zip(ks, ps, L, Li):
        assert np.all(np.tril(Lk, -1) == 0.0) and np.all(np.tril(Lik, -1) == 0.0), k
        root = np.sqrt(q)
        d_ulp = np.abs(np.diag(Lk) - root) / np.spacing(root)
        wide = np.sqrt(q.astype(LD))
        i_ulp = pc.ulp_error(np.diag(Lik), 1 / wide)
        print(f"4^{k}: L_ii {d_ulp.max():.2f} ulp of np.sqrt ({pc.ulp_error(np.diag(Lk), wide).max():.3f} of the exact root), "
              f"Linv_ii {i_ulp.max():.3f} ulp (pivot {q[np.argmax(i_ulp)]!r})")
        assert d_ulp.max() <= 2.0, (k, q[np.argmax(d_ulp)])
        worst = max(worst, float(i_ulp.max()))
    print(f"Linv_ii: largest error {worst:.3f} ulp")
    assert worst <= 4 * LINV_DIAG_ULP_MEASURED


def test_scaling_by_powers_of_four(dev):
    """A 4^250 and A 4^-250 at n = 256: L is 2^k L_ref and L^-1 is 2^-k Linv_ref within the forward bounds of the unscaled
    matrix, info = 0 (nothing on the way overflows or loses its exponent)."""
    A = pc.spd(256)
    ref = pc.reference(A)
    ks = (0, 250, -250)
    L, Li, info = dev.hook([pc.scaled(A, k) for k in ks])
    assert not info.any()
    for k, Lk, Lik in zip(ks, L, Li):
        check_fp64_factor(Lk, Lik, pc.scaled(A, k), ref, scale=2.0 ** k, what=f"4^{k}")


# ------------------------------------------------------------------ the hook, fp32
def _fp32_case(n):
    A32 = pc.spd(n).astype(np.float32)
    ref = pc.reference(A32.astype(np.float64))
    c, info = lapack.spotrf(np.tril(A32), lower=1)
    assert info == 0 and c.dtype == np.float32
    Ls = np.tril(c)
    Lis, info = lapack.strtri(Ls, lower=1)
    assert info == 0 and Lis.dtype == np.float32
    return A32, ref, Ls, np.tril(Lis)


@pytest.mark.parametrize("n", [128, 256, 384])
def test_fp32_every_element(dev, n):
    """potrf_lockstep<float> / chol_leaf_reg_kernel<float>: every element against the longdouble reference of the
    float32-rounded matrix.  No tolerance of the project's exists for fp32, so each error is held to 10 x the error of
    LAPACK's spotrf (inverse: strtri of spotrf's factor, in fp32) on the same matrix, computed here at run time.
    Measured on the MI355X (2026-10-20), kernel against spotrf / strtri, n = 128 / 256 / 384:
      |L L^T - A| / |A|       3.38e-7 / 5.07e-7 / 5.14e-7   against   1.06e-7 / 1.63e-7 / 1.40e-7
      |L - L_ref| / |L_ref|   2.20e-7 / 2.99e-7 / 2.73e-7   against   6.73e-8 / 9.14e-8 / 8.00e-8
      |Li L - I|              1.25e-7 / 1.24e-7 / 1.20e-7   against   4.07e-8 / 4.12e-8 / 4.21e-8
      |Li L_ref - I|          2.80e-7 / 2.91e-7 / 3.32e-7   against   9.20e-8 / 1.09e-7 / 1.21e-7
    i.e. 3 to 4 x LAPACK throughout."""
    A32, ref, Ls, Lis = _fp32_case(n)
    L, Li, info = dev.hook([A32], dtype=np.float32, lower_only=True)
    assert info[0] == 0 and L.dtype == np.float32
    L, Li = L[0], Li[0]
    A = A32.astype(np.float64)
    rows = (("|L L^T - A| / |A|", pc.err_backward(L, A), pc.err_backward(Ls, A)),
            ("|L - L_ref| / |L_ref|", pc.err_factor(L, ref), pc.err_factor(Ls, ref)),
            ("|Li L - I|", pc.err_product(Li, L), pc.err_product(Lis, Ls)),
            ("|Li L_ref - I|", pc.err_inverse(Li, ref), pc.err_inverse(Lis, ref)))
    for name, mine, theirs in rows:
        print(f"fp32 n {n}: {name}: kernel {mine:.3e}, spotrf/strtri {theirs:.3e}")
    for name, mine, theirs in rows:
        assert mine <= 10 * theirs, (name, mine, theirs)
    assert pc.upper_is_zero(L, 128) and pc.upper_is_zero(Li, 128)


def test_fp32_info_and_chain_independence(dev, solo256):
    A32 = pc.spd(384).astype(np.float32)
    L0 = pc.reference(A32.astype(np.float64)).L
    mats, want = [], []
    for variant in ("negative", "nan_diag"):
        for j in (0, 16, 127, 128, 383):
            B, w = pc.failing(A32, variant, j, L0)
            assert B.dtype == np.float32 and pc.reference(B.astype(np.float64), want_inverse=False).info == w
            mats.append(B)
            want.append(w)
    _, _, info = dev.hook(mats, dtype=np.float32)
    assert info.tolist() == want
    L, Li, info = dev.hook([pc.spd(256, seed=b) for b in range(5)], dtype=np.float32)
    assert not info.any()
    for b in range(5):
        Ls, Lis = solo256(b, np.float32)
        assert pc.same_bits(np.tril(L[b]), Ls) and pc.same_bits(np.tril(Li[b]), Lis), f"chain {b}"


# ------------------------------------------------------------------ the public entry point
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 127, 128, 129, 255, 257])
def test_gpfit_potrf_at_padded_sizes_and_strided_layouts(dev, n):
    """The identity padding of pack_lower and the contract of the header: only the lower triangle of A is read (the rest
    is NaN), lda / ldl / ldi differ from n and from each other, the strict upper parts of L and Linv are exactly zero,
    nothing is written beyond column n, logdet = 2 sum log L_ii; without Linv the same L bits and the same logdet."""
    A = pc.spd(n)
    ref = pc.reference(A)
    rc, L, Li, logdet, info, msg = dev.public(A)
    assert rc == 0 and info == 0, msg
    check_fp64_factor(L[:, :n], Li[:, :n], A, ref, what=f"gpfit_potrf n {n}", block=None)
    assert abs(logdet - ref.logdet) <= 1e-10 * abs(ref.logdet)
    assert np.all(L[:, n:] == SENTINEL) and np.all(Li[:, n:] == SENTINEL)
    rc, L2, _, logdet2, info, msg = dev.public(A, want_inverse=False)
    assert rc == 0 and info == 0, msg
    assert pc.same_bits(L2, L) and logdet2 == logdet


@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_gpfit_potrf_failures_and_the_call_after(dev, variant):
    """n = 300 (padded to 384): the return value is *info_host is the reference's info, the message says why -- and the
    next call on the same context, with a good matrix, is clean: no stale info word.  nan_below has no case at the last
    column."""
    n = 300
    A = pc.spd(n)
    ref = pc.reference(A)
    rc, L_good, Li_good, logdet_good, info, msg = dev.public(A)
    assert rc == 0 and info == 0, msg
    check_fp64_factor(L_good[:, :n], Li_good[:, :n], A, ref, what="n 300", block=None)
    for j in (0, 16, 128, 129, 256, 299):
        if variant == "nan_below" and pc.nan_row(n, j) is None:
            continue
        B, want = pc.failing(A, variant, j, ref.L)
        assert pc.reference(B, want_inverse=False).info == want
        rc, _, _, _, info, msg = dev.public(B)
        assert rc == info == want, (variant, j, rc, info, want)
        assert "not positive definite" in msg
        rc, L, Li, logdet, info, msg = dev.public(A)
        assert rc == 0 and info == 0, (variant, j, msg)
        assert pc.same_bits(L, L_good) and pc.same_bits(Li, Li_good) and logdet == logdet_good
