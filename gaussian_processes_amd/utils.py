"""Drop-in host module for the GP fit path of ``Spatial_GP_repo/utils.py``.

Same function names, argument meaning and error behaviour as the reference for the path
SURVEY.md section 8 scopes (``localker``, ``acosker``, ``lambda_moments``, ``compute_KL_div``,
``Estep``, ``varGP``, ``test`` ...), but every kernel / factorisation / solve runs in the
hand-written HIP library ``libgpfit_mi355x.so`` through ctypes.  torch supplies device
memory, streams, the L-BFGS drivers and, for the eigen-stabilisation of matrices below 256 rows or whenever the
eigh-free routes decline (an eigenvalue on the threshold), ``torch.linalg.eigh``.

There is no CPU fallback: without a GPU or without the built library every entry point raises.
Out of scope (SURVEY.md section 2 rows 10-14,16-19): plotting, persistence (``save_model`` / ``load_model``: the
reference's own functions pickle the ``fit_model`` dict this module returns), the dataset container, and the
reference's dead code (``utility`` / ``get_utility`` scalar variants, ``block_matrix_inverse``, ``updateA``,
``linker``: no caller in the reference's own files).
"""
from __future__ import annotations

import collections
import copy
import ctypes
import math
import threading
import time
import warnings

import torch

from . import _lib
from .engine import GPFitEngine, _grid, theta_vec
from . import eigtop
from .synthetic import THETA_KEYS

torch.set_grad_enabled(False)  # reference utils.py:2 (analytic gradients only)

TORCH_DTYPE = torch.float64          # utils.py:31
torch.set_default_dtype(TORCH_DTYPE)  # utils.py:33 -- the reference makes float64 the global default on
#                                       import and its notebooks rely on it (torch.tensor(0.05) is fp64)
MIN_TOLERANCE = 1.e-11               # utils.py:37
EIGVAL_TOL = 1.e-4                   # utils.py:39 (module global read at call time, as in the reference)
PI32 = 3.1415927410125732            # utils.py:25: float32-rounded pi

# dC dict key order of the reference (utils.py:910) == matrix order of gpfit_localker
DC_KEYS = ("Amp", "-2log2beta", "-log2rho2", "eps_0x", "eps_0y")


_HAVE_GPU = [False]


def _device():
    if not _HAVE_GPU[0]:       # (asked once: torch.cuda.is_available() costs 2 us and this is called 30 000 times per fit)
        if not torch.cuda.is_available():
            raise _lib.GpfitError("gaussian_processes_amd.utils needs an MI355X: there is no CPU fallback")
        _HAVE_GPU[0] = True
    return torch.device("cuda", torch.cuda.current_device())


class _EnginePool:
    """One workspace per (device, host thread): the C context is not re-entrant, and the
    reference's active-learning notebook scores candidates on a second ``threading.Thread`` while
    the main thread fits (one_cell_active_training.ipynb:2446-2461).

    A workspace only ever grows.  Growing allocates a new context and drops the pool's reference
    to the old one, which is destroyed when its last holder lets go -- an engine a caller still
    holds stays valid.  ``varGP`` / ``test`` size the pool once up front (``reserve``), so no
    reallocation happens in the middle of a fit."""

    def __init__(self):
        self.eng = {}
        self.lock = threading.Lock()

    def get(self, n, d, d_full=None):
        dev = _device()
        key = (dev.index, threading.get_ident())
        d_full = int(d_full or d)
        with self.lock:
            e = self.eng.get(key)
            if e is None or e.n_max < n or e.d_max < d or e.d_full_max < d_full:
                n_cap = max(n, e.n_max if e else 0)
                d_cap = max(d, e.d_max if e else 0)
                f_cap = max(d_full, e.d_full_max if e else 0)
                if e is None:
                    alive = {t.ident for t in threading.enumerate()}
                    for k in [k for k in self.eng if k[1] not in alive]:
                        del self.eng[k]          # contexts of threads that have ended
                self.eng[key] = None             # release the old workspace before allocating the new one
                del e                            # (unless a caller still holds it)
                e = GPFitEngine(n_cap, d_cap, f_cap, device=dev.index)
                self.eng[key] = e
            return e


_POOL = _EnginePool()


def get_engine(n, d, d_full=None) -> GPFitEngine:
    return _POOL.get(int(n), int(d), d_full)


def reserve(n, d, d_full=None) -> GPFitEngine:
    """Size this thread's workspace for problems up to ``n`` stimuli and ``d`` (masked) / ``d_full``
    (image) pixels in one allocation."""
    return _POOL.get(int(n), int(d), d_full)


def _scalar(v) -> float:
    return float(v.item()) if hasattr(v, "item") else float(v)


def _cu(t, name="tensor"):
    """float64 contiguous CUDA view of ``t`` (moved if it lives on the host)."""
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t, dtype=TORCH_DTYPE)
    dev = _device()
    if t.dtype != TORCH_DTYPE or t.device != dev:
        t = t.to(device=dev, dtype=TORCH_DTYPE)
    return t.contiguous()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------ kernel functions
def localker(theta, theta_higher_lims, theta_lower_lims, n_px_side, grad=False):
    """Spatial metric ``C`` (reference utils.py:861-914).  Returns ``(C, mask)`` or
    ``(C, mask, dC)`` with dC a dict keyed Amp, -2log2beta, -log2rho2, eps_0x, eps_0y.
    Raises ValueError when a hyperparameter is outside its limits (utils.py:865-867).
    ``n_px_side`` may also be ``(n_rows, n_cols)`` (rectangular generalisation)."""
    lib = _lib.load()
    th = _lib.darr(theta_vec(theta))
    lo = _lib.darr([_scalar(theta_lower_lims[k]) for k in THETA_KEYS])
    up = _lib.darr([_scalar(theta_higher_lims[k]) for k in THETA_KEYS])
    if lib.gpfit_check_limits(th, lo, up) != 0:
        raise ValueError(_lib.last_error())
    rows, cols = _grid(n_px_side)
    mbuf = (ctypes.c_uint8 * (rows * cols))()
    dcount = ctypes.c_int64()
    _lib.check(lib.gpfit_localker_mask(th, rows, cols, mbuf, ctypes.byref(dcount)), "gpfit_localker_mask")
    d = int(dcount.value)
    dev = _device()
    mask = torch.frombuffer(bytearray(mbuf), dtype=torch.uint8).to(torch.bool).to(dev)
    if d == 0:
        raise ValueError("localker: the pixel mask is empty")
    eng = get_engine(1, d, rows * cols)
    C = torch.empty((d, d), dtype=TORCH_DTYPE, device=dev)
    dCbuf = torch.empty((5, d, d), dtype=TORCH_DTYPE, device=dev) if grad else None
    _lib.check(lib.gpfit_localker(eng._ctx, _stream(), th, rows, cols, mbuf, d, C.data_ptr(),
                                  dCbuf.data_ptr() if grad else None), "gpfit_localker")
    if not grad:
        return C, mask
    return C, mask, {k: dCbuf[i] for i, k in enumerate(DC_KEYS)}


def _pack_dC(dC, d, dev):
    """dict of d x d matrices -> contiguous [5][d][d] in the library's order (or None)."""
    if dC is None:
        return None
    if all(k in dC for k in DC_KEYS):
        first = dC[DC_KEYS[0]]
        base = getattr(first, "_base", None)
        if (isinstance(base, torch.Tensor) and base.dim() == 3 and base.shape[0] == 5 and base.is_contiguous()
                and all(dC[k]._base is base and dC[k].data_ptr() == base[i].data_ptr()
                        for i, k in enumerate(DC_KEYS))):
            return base  # exactly what localker returned: no copy
        return torch.stack([_cu(dC[k]) for k in DC_KEYS]).contiguous()
    raise KeyError(f"dC must hold the keys {DC_KEYS}")


def acosker(theta, x1, x2=None, C=None, dC=None, diag=False):
    """Arc-cosine kernel (reference utils.py:939-1050).

    ``x1[n1, nx]``, ``x2[n2, nx]`` already masked; ``C[nx, nx]``.  diag=False returns
    ``K[n1, n2]`` (symmetrised when n1 == n2) and, if dC is given, ``(K, dK)`` with dK a dict
    over the six hyperparameters.  diag=True returns the vector ``x_i C x_i + sigma_0^2``."""
    lib = _lib.load()
    dev = _device()
    s0 = _scalar(theta["sigma_0"])
    x1 = _cu(x1)
    if x1.dim() == 1:
        x1 = x1[None, :]
    n1, d = x1.shape
    if C is None:
        C = torch.eye(n1, dtype=TORCH_DTYPE, device=dev)  # utils.py:973 (only meaningful when n1 == nx)
    C = _cu(C)
    if C.shape != (d, d):
        raise RuntimeError(f"acosker: C is {tuple(C.shape)} but the inputs have {d} pixels")
    dCbuf = _pack_dC(dC, d, dev)
    if diag:
        eng = get_engine(n1, d)
        Kvec = torch.empty(n1, dtype=TORCH_DTYPE, device=dev)
        dKv = torch.empty((6, n1), dtype=TORCH_DTYPE, device=dev) if dC is not None else None
        _lib.check(lib.gpfit_acosker_diag(eng._ctx, _stream(), s0, x1.data_ptr(), x1.stride(0), n1, d,
                                          C.data_ptr(), C.stride(0), dCbuf.data_ptr() if dCbuf is not None else None,
                                          Kvec.data_ptr(), dKv.data_ptr() if dKv is not None else None),
                   "gpfit_acosker_diag")
        if dC is None:
            return Kvec if n1 > 1 else Kvec.squeeze()
        return Kvec, {k: dKv[i] for i, k in enumerate(THETA_KEYS)}
    same = x2 is None or x2 is x1
    x2 = x1 if same else _cu(x2)
    if x2.dim() == 1:
        x2 = x2[None, :]
    if not same and x2.data_ptr() == x1.data_ptr() and x2.shape == x1.shape:
        x2 = x1
    n2 = x2.shape[0]
    if x2.shape[1] != d:
        raise RuntimeError("acosker: x1 and x2 have different numbers of pixels")
    eng = get_engine(max(n1, n2), d)
    K = torch.empty((n1, n2), dtype=TORCH_DTYPE, device=dev)
    dK = torch.empty((6, n1, n2), dtype=TORCH_DTYPE, device=dev) if dC is not None else None
    _lib.check(lib.gpfit_acosker(eng._ctx, _stream(), s0, x1.data_ptr(), x1.stride(0), n1, x2.data_ptr(),
                                 x2.stride(0), n2, d, C.data_ptr(), C.stride(0),
                                 dCbuf.data_ptr() if dCbuf is not None else None, K.data_ptr(), K.stride(0),
                                 dK.data_ptr() if dK is not None else None), "gpfit_acosker")
    if dC is None:
        return K
    return K, {k: dK[i] for i, k in enumerate(THETA_KEYS)}


# ------------------------------------------------------------------ dense helpers on the MFMA GEMM
def _pad2(t, rows, cols):
    if t.shape[0] == rows and t.shape[1] == cols and t.is_contiguous():
        return t
    out = torch.zeros((rows, cols), dtype=TORCH_DTYPE, device=t.device)
    out[: t.shape[0], : t.shape[1]] = t
    return out


def _ceil(x, m):
    return (x + m - 1) // m * m


def matmul(A, B, transA=False, transB=False, alpha=1.0):
    """``alpha * op(A) @ op(B)`` on the fp64 MFMA GEMM (``gpfit_dgemm``): the torch ``@`` call
    sites of the reference's path.  1-D operands are treated as column/row vectors."""
    lib = _lib.load()
    # fast path (the subspace solver and the E-steps issue thousands of these per fit: the wrapper's own checks were a
    # quarter of their cost): 2-D float64 device operands, contiguous, already aligned -- straight to the C ABI
    if (type(A) is torch.Tensor and type(B) is torch.Tensor and A.dim() == 2 and B.dim() == 2 and A.is_cuda and B.is_cuda
            and A.dtype is TORCH_DTYPE and B.dtype is TORCH_DTYPE and A.is_contiguous() and B.is_contiguous()):
        M, K = (A.shape[1], A.shape[0]) if transA else A.shape
        K2, N = (B.shape[1], B.shape[0]) if transB else B.shape
        if K == K2 and not (K & 15) and not (M & 1) and not (N & 1) and A.device == B.device:
            C = torch.empty((M, N), dtype=TORCH_DTYPE, device=A.device)
            _lib.check(lib.gpfit_dgemm(_stream(), 1 if transA else 0, 0 if transB else 1, M, N, K, float(alpha),
                                       A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), 0.0, C.data_ptr(), N, 0, 0, 0),
                       "gpfit_dgemm")
            return C
    A, B = _cu(A), _cu(B)
    va, vb = A.dim() == 1, B.dim() == 1
    if va:
        A = A[None, :] if not transA else A[:, None]
    if vb:
        B = B[:, None] if not transB else B[None, :]
    M, K = (A.shape[1], A.shape[0]) if transA else A.shape
    K2, N = (B.shape[1], B.shape[0]) if transB else B.shape
    if K != K2:
        raise RuntimeError(f"matmul: inner dimensions differ ({K} vs {K2})")
    Kp, Mp, Np = _ceil(K, 16), _ceil(M, 2), _ceil(N, 2)
    Ap = _pad2(A, Kp, Mp) if transA else _pad2(A, Mp, Kp)
    Bp = _pad2(B, Np, Kp) if transB else _pad2(B, Kp, Np)
    Cp = torch.empty((Mp, Np), dtype=TORCH_DTYPE, device=A.device)
    _lib.check(lib.gpfit_dgemm(_stream(), 1 if transA else 0, 0 if transB else 1, Mp, Np, Kp, float(alpha),
                               Ap.data_ptr(), Ap.stride(0), Bp.data_ptr(), Bp.stride(0), 0.0, Cp.data_ptr(),
                               Cp.stride(0), 0, 0, 0), "gpfit_dgemm")
    C = Cp[:M, :N]
    if va and vb:
        return C.reshape(()).clone()
    if vb:
        return C[:, 0].contiguous()   # never hand out strided views: callers pass data_ptr() on
    if va:
        return C[0, :].contiguous()
    return C.contiguous()


def gemm_into(C, A, B, alpha=1.0, beta=0.0, transA=False, transB=False):
    """``C <- alpha op(A) op(B) + beta C`` in place (``gpfit_dgemm`` with its beta): 2-D float64 device tensors, contiguous,
    K a multiple of 16, M and N even.  For iterations that would otherwise allocate and combine (eigtop's sign iteration)."""
    lib = _lib.load()
    M, K = (A.shape[1], A.shape[0]) if transA else A.shape
    K2, N = (B.shape[1], B.shape[0]) if transB else B.shape
    if K != K2 or tuple(C.shape) != (M, N) or (K & 15) or (M & 1) or (N & 1):
        raise RuntimeError("gemm_into: shapes do not fit (K % 16, even M and N, C = [M, N])")
    _lib.check(lib.gpfit_dgemm(_stream(), 1 if transA else 0, 0 if transB else 1, M, N, K, float(alpha), A.data_ptr(),
                               A.stride(0), B.data_ptr(), B.stride(0), float(beta), C.data_ptr(), C.stride(0), 0, 0, 0),
               "gpfit_dgemm")
    return C


def cholesky(M, want_inverse=False):
    """Lower Cholesky factor (and optionally its inverse) by the recursive MFMA algorithm.
    Returns ``(L, Linv_or_None, logdet, info)``; info > 0 = first non-positive pivot (LAPACK)."""
    lib = _lib.load()
    M = _cu(M)
    n = M.shape[0]
    eng = get_engine(n, 1)
    L = torch.empty((n, n), dtype=TORCH_DTYPE, device=M.device)
    Li = torch.empty((n, n), dtype=TORCH_DTYPE, device=M.device) if want_inverse else None
    logdet = ctypes.c_double()
    info = ctypes.c_int()
    rc = lib.gpfit_potrf(eng._ctx, _stream(), M.data_ptr(), M.stride(0), n, L.data_ptr(), L.stride(0),
                         Li.data_ptr() if want_inverse else None, Li.stride(0) if want_inverse else 0,
                         ctypes.byref(logdet), ctypes.byref(info))
    if rc < 0:
        _lib.check(rc, "gpfit_potrf")
    return L, Li, float(logdet.value), int(info.value)


def cholesky_append(L, Linv, kcol, logdet=0.0):
    """Factor of ``[[K, k], [k^T, kappa]]`` from the factor of K in O(n^2) (``gpfit_potrf_append``):
    ``L``, ``Linv`` are (n+1) x (n+1) device tensors whose leading n x n blocks hold the factor of K and
    its inverse (what ``cholesky(K, want_inverse=True)`` returned, embedded); ``kcol`` the n+1 entries of
    the new last column.  Row n of both is written in place; returns ``(logdet_new, info)``.  The closed
    loop of the reference's one_cell_active_training.ipynb adds one stimulus per iteration
    (:1889-1891): with this the refit's factorisation of K~ costs a row, not an N^3 / 3."""
    lib = _lib.load()
    n = L.shape[0] - 1
    if L.shape != (n + 1, n + 1) or Linv.shape != (n + 1, n + 1) or not (L.is_cuda and Linv.is_cuda):
        raise ValueError("cholesky_append: L and Linv must be (n+1) x (n+1) device tensors")
    if L.dtype != TORCH_DTYPE or Linv.dtype != TORCH_DTYPE or L.stride(1) != 1 or Linv.stride(1) != 1:
        raise ValueError("cholesky_append: L and Linv must be row-major float64")
    kcol = _cu(kcol).reshape(-1)
    if kcol.shape[0] != n + 1:
        raise ValueError("cholesky_append: kcol must hold n + 1 entries")
    eng = get_engine(n + 1, 1)
    ld = ctypes.c_double(float(logdet))
    info = ctypes.c_int()
    rc = lib.gpfit_potrf_append(eng._ctx, _stream(), L.data_ptr(), L.stride(0), Linv.data_ptr(), Linv.stride(0), n,
                                kcol.data_ptr(), ctypes.byref(ld), ctypes.byref(info))
    if rc < 0:
        _lib.check(rc, "gpfit_potrf_append")
    return float(ld.value), int(info.value)


APPEND_BLOCK_MAX = 128   # columns of one gpfit_potrf_append_block call


def cholesky_append_block(L, Linv, Kcols, logdet=0.0):
    """Factor of ``[[K, K12], [K12^T, K22]]`` from the factor of K, k rows at once (``gpfit_potrf_append_block``):
    ``L``, ``Linv`` are (n+k) x (n+k) device tensors whose leading n x n blocks hold the factor of K and its
    inverse, ``Kcols`` the (n+k) x k block of the new last k columns (of its bottom k x k block only the lower
    triangle is read).  Rows n .. n+k-1 of both are written in place; returns ``(logdet_new, info)``.  Any k >= 1:
    the columns go to the library at most 128 at a time, each chunk growing the factor the next one starts from;
    a chunk that fails stops the sweep and its ``info`` (the 1-based index of the pivot in the grown matrix) is
    returned with the log-det of the chunks before it.  A closed-loop round that shows b images costs O(n^2 b) in
    two passes over ``L^-1`` and one host wait per chunk, where b ``cholesky_append`` calls wait b times."""
    if not (isinstance(L, torch.Tensor) and isinstance(Linv, torch.Tensor) and isinstance(Kcols, torch.Tensor)):
        raise ValueError("cholesky_append_block: L, Linv and Kcols must be tensors")
    if Kcols.dim() != 2 or Kcols.shape[1] < 1:
        raise ValueError("cholesky_append_block: Kcols must be (n+k) x k with k >= 1")
    nk, k = Kcols.shape
    n = nk - k
    if n < 1 or L.shape != (nk, nk) or Linv.shape != (nk, nk):
        raise ValueError("cholesky_append_block: L and Linv must be (n+k) x (n+k) and Kcols (n+k) x k, n >= 1")
    if not (L.is_cuda and Linv.is_cuda and Kcols.is_cuda):
        raise ValueError("cholesky_append_block: L, Linv and Kcols must be device tensors")
    if L.dtype != TORCH_DTYPE or Linv.dtype != TORCH_DTYPE or L.stride(1) != 1 or Linv.stride(1) != 1:
        raise ValueError("cholesky_append_block: L and Linv must be row-major float64")
    if Kcols.dtype != TORCH_DTYPE or Kcols.stride(1) != 1:
        raise ValueError("cholesky_append_block: Kcols must be row-major float64")
    lib = _lib.load()
    eng = get_engine(nk, 1)
    ld = ctypes.c_double(float(logdet))
    info = ctypes.c_int(0)
    for c0 in range(0, k, APPEND_BLOCK_MAX):
        kc = min(APPEND_BLOCK_MAX, k - c0)
        cols = Kcols[:, c0:]                  # rows 0 .. n + c0 + kc - 1, columns c0 .. c0 + kc - 1 of the grown matrix
        rc = lib.gpfit_potrf_append_block(eng._ctx, _stream(), L.data_ptr(), L.stride(0), Linv.data_ptr(), Linv.stride(0),
                                          n + c0, kc, cols.data_ptr(), Kcols.stride(0), ctypes.byref(ld), ctypes.byref(info))
        if rc < 0:
            _lib.check(rc, "gpfit_potrf_append_block")
        if info.value != 0:
            break
    return float(ld.value), int(info.value)


def spd_inverse(M):
    """M^-1 = L^-T L^-1 for a symmetric positive definite matrix (replaces the LU
    ``torch.linalg.solve(M, I)`` of utils.py:2067)."""
    L, Li, _, info = cholesky(M, want_inverse=True)
    if info != 0:
        raise torch.linalg.LinAlgError(f"spd_inverse: matrix is not positive definite (info={info})")
    return matmul(Li, Li, transA=True)


# ------------------------------------------------------------------ numeric guards (utils.py:633-685)
def is_simmetric(tensor, name='M'):
    difference = (tensor - tensor.T).abs()
    if bool(torch.any(difference > MIN_TOLERANCE)):
        print(f'Matrix {name} is not symmetric, maximum difference is {difference.max()}')
        return False
    return True


def is_posdef(tensor, name='M'):
    if not is_simmetric(tensor, name=name):
        warnings.warn('The matrix is not symmetric, cannot check if it is positive definite')
        return False
    # cheap proof first: a successful Cholesky with 1 / (||L^-1||_1 ||L^-1||_inf) > MIN_TOLERANCE bounds the
    # smallest eigenvalue from below (see _all_eigenvalues_kept); eigvalsh only when that is inconclusive
    t = _cu(tensor)
    L, Li, _, info = cholesky(t, want_inverse=True)
    if info == 0:
        ali = Li.abs()
        if 1.0 / (float(ali.sum(0).max()) * float(ali.sum(1).max())) > MIN_TOLERANCE:
            return True
    smallest = float(torch.linalg.eigvalsh(t).min())
    if smallest <= 0.:
        warnings.warn(f'Matrix {name} is simmetric but has an eigenvalue smaller than 0 ')
        return False
    if smallest <= MIN_TOLERANCE:
        warnings.warn(f'Matrix {name} is simmetric but has an eigenvalue smaller than MIN_TOLERANCE: {MIN_TOLERANCE}')
        return False
    return True


def safe_log(x):
    if bool(torch.any(x <= 0)):
        raise ValueError("Negative or zero input to log detected")
    if bool(torch.any(x < 1e-10)):
        raise ValueError("Very small input to log detected")
    return torch.log(x)


def safe_acos(x):
    if bool(torch.any(x > 1 - 1e-6)) or bool(torch.any(x < -1 + 1e-6)):
        x = torch.clamp(x, -1 + 1e-6, 1 - 1e-6)
    return torch.acos(x)


def log_det(M, name='M', ignore_warning=False):
    """log|M| from the Cholesky factor, with the reference's fallbacks (utils.py:1271-1304):
    failed factorisation + symmetric -> sum of log of the eigenvalues above the truncation
    rule (with warnings); not symmetric -> warning and 0."""
    M = _cu(M)
    L, _, logdet, info = cholesky(M)
    if info == 0:
        safe_log(torch.diagonal(L))  # raises exactly when the reference's safe_log would
        return torch.tensor(logdet, dtype=TORCH_DTYPE, device=M.device)
    if is_simmetric(M, name=name):
        eigenvalues = torch.linalg.eigvalsh(M)
        ikeep = eigenvalues > max(float(eigenvalues.max()) * EIGVAL_TOL, EIGVAL_TOL)
        if not ignore_warning:
            smallest = float(eigenvalues.min())
            warnings.warn(f"Matrix {name} in logdet is simmetric but not posdef, using eigendecomposition to calculate the log determinant")
            if smallest <= 0.:
                warnings.warn(f'Matrix {name} in logdet is simmetric but has an eigenvalue smaller than 0 ')
            elif smallest <= 1.e-10:
                warnings.warn(f'Matrix {name} in logdet is simmetric but has an eigenvalue smaller than 1e-10 ')
        return torch.sum(safe_log(eigenvalues[ikeep]))
    warnings.warn(f"Matrix {name} in logdet is not simmetric in log_det used in KL_divergence")
    return 0


# ------------------------------------------------------------------ moments / likelihood / KL
def lambda_moments(x, K_tilde, KKtilde_inv, Kvec, K, C, m, V, theta, kernfun=None, dK=None, dK_tilde=None,
                   dK_vec=None, K_tilde_inv=None):
    """Mean and variance of lambda at the training points and, optionally, their
    theta-gradients (reference utils.py:1072-1124); every product on the MFMA GEMM."""
    a = _cu(KKtilde_inv)
    K, m, V = _cu(K), _cu(m), _cu(V)
    lambda_m = matmul(a, m)                                                       # :1090
    if Kvec is None:
        Kvec = kernfun(theta, x, x2=None, C=C, dC=None, diag=True)                # :1094
    aV = matmul(a, V)
    lambda_var = _cu(Kvec) + torch.sum(-K * a + a * aV, 1)                        # :1101 (V symmetric)
    if dK is None or dK_tilde is None or dK_vec is None or K_tilde_inv is None:
        return lambda_m, lambda_var
    dlambda_m, dlambda_var = {}, {}
    Kinv = _cu(K_tilde_inv)
    for key in dK.keys():
        da = matmul(_cu(dK[key]) - matmul(a, dK_tilde[key]), Kinv)                # :1114
        dlambda_m[key] = matmul(da, m)                                            # :1117
        dlambda_var[key] = (_cu(dK_vec[key]) + 2 * torch.sum(da * aV, 1) - torch.sum(_cu(dK[key]) * a, 1)
                            - torch.sum(K * da, 1))                               # :1120
    return lambda_m, lambda_var, dlambda_m, dlambda_var


def _lambda0_of(f_params):
    return torch.exp(f_params['loglambda0']) if 'loglambda0' in f_params else f_params['lambda0']


def _fparam_eval(lambda_m, lambda_var, r, logA, closed_form, lambda0=0.0, want_f=True):
    lib = _lib.load()
    lm, lv = _cu(lambda_m), _cu(lambda_var)
    n = lm.shape[0]
    rr = _cu(r) if r is not None else torch.zeros(n, dtype=TORCH_DTYPE, device=lm.device)
    eng = get_engine(n, 1)
    f = torch.empty(n, dtype=TORCH_DTYPE, device=lm.device) if want_f else None
    out = (ctypes.c_double * 7)()
    _lib.check(lib.gpfit_fparam_eval(eng._ctx, _stream(), lm.data_ptr(), lv.data_ptr(), rr.data_ptr(), n,
                                     _scalar(logA), 1 if closed_form else 0, float(lambda0),
                                     f.data_ptr() if want_f else None, out), "gpfit_fparam_eval")
    return f, list(out)


def _fparam_lbfgs(lambda_m, lambda_var, r, f_params, n_steps, i_estep):
    """The rate-parameter optimiser of an E-step (utils.py:1892-1934) as one device call (gpfit_fparam_lbfgs):
    lambda0 at its closed form for the starting logA, ``LBFGS([logA], lr=0.1, max_iter=n_steps, tolerance_change=1e-9,
    tolerance_grad=1e-7, history_size=n_steps, line_search_fn='strong_wolfe').step(closure_f_params)`` and
    ``lambda0_and_rate()``.  Updates ``f_params['logA']`` in place and sets ``f_params['lambda0']``; returns the rate
    at the final (logA, lambda0) and that lambda0.  A non-finite sum f in closure call k raises the closure's
    ValueError and leaves logA at that call's point and lambda0 at its closed form there, as the closure does."""
    lib = _lib.load()
    lm, lv, rr = _cu(lambda_m), _cu(lambda_var), _cu(r)
    n = lm.shape[0]
    eng = get_engine(n, 1)
    f = torch.empty(n, dtype=TORCH_DTYPE, device=lm.device)
    out = (ctypes.c_double * 9)()
    fixed = 'loglambda0' in f_params
    _lib.check(lib.gpfit_fparam_lbfgs(eng._ctx, _stream(), lm.data_ptr(), lv.data_ptr(), rr.data_ptr(), n,
                                      _scalar(f_params['logA']), 1 if fixed else 0,
                                      _scalar(_lambda0_of(f_params)) if fixed else 0.0, int(n_steps), int(n_steps),
                                      0.1, 1.e-7, 1.e-9, f.data_ptr(), out), "gpfit_fparam_lbfgs")
    status = int(out[6])
    with torch.no_grad():
        f_params['logA'].fill_(out[7] if status else out[0])      # the same tensor, as LBFGS's p.add_ leaves it
    f_params['lambda0'] = torch.tensor(out[8] if status else out[1], dtype=TORCH_DTYPE)
    if status:
        raise ValueError(f'Nan in f_mean during f param update in Estep, closure has been called {status} times in '
                         f'estep {i_estep} iteration.')                                                      # :1923
    return f, out[1]


def mean_f_given_lambda_moments(f_params, lambda_m, lambda_var):
    """<f> = exp(A <lambda> + A^2/2 Var(lambda) + lambda0)   (utils.py:1126-1141)."""
    f, _ = _fparam_eval(lambda_m, lambda_var, None, f_params['logA'], False, _scalar(_lambda0_of(f_params)))
    return f


def lambda0_given_logA(logA, r, lambda_m, lambda_var):
    """Closed-form optimum of lambda0 given A (utils.py:1215-1229)."""
    _, out = _fparam_eval(lambda_m, lambda_var, r, logA, True, want_f=False)
    return torch.tensor(out[0], dtype=TORCH_DTYPE)


def mean_f(f_params, calculate_moments, lambda_m=None, lambda_var=None, x=None, K_tilde=None, KKtilde_inv=None,
           Kvec=None, K=None, C=None, m=None, V=None, V_inv=None, theta=None, kernfun=None, dK=None, dK_tilde=None,
           dK_vec=None, K_tilde_inv=None, r=None):
    """utils.py:1143-1213: firing-rate mean, computing the lambda moments first when asked to."""
    def rate(lm, lv):
        if r is not None:
            tmp = {'logA': f_params['logA'], 'lambda0': lambda0_given_logA(f_params['logA'], r, lm, lv)}
            return mean_f_given_lambda_moments(tmp, lm, lv)
        return mean_f_given_lambda_moments(f_params, lm, lv)

    if calculate_moments and (lambda_m is None or lambda_var is None):
        if dK is not None and dK_tilde is not None and dK_vec is not None and K_tilde_inv is not None:
            lambda_m, lambda_var, dlm, dlv = lambda_moments(x, K_tilde, KKtilde_inv, Kvec, K, C, m, V, theta,
                                                            kernfun=kernfun, dK=dK, dK_tilde=dK_tilde, dK_vec=dK_vec,
                                                            K_tilde_inv=K_tilde_inv)
            return rate(lambda_m, lambda_var), lambda_m, lambda_var, dlm, dlv
        lambda_m, lambda_var = lambda_moments(x, K_tilde, KKtilde_inv, Kvec, K, C, m, V, theta, kernfun=kernfun)
        return rate(lambda_m, lambda_var), lambda_m, lambda_var
    return rate(lambda_m, lambda_var)


def compute_loglikelihood(r, f_mean, lambda_m, lambda_var, f_params, compute_grad_for_f_params=False,
                          dlambda_m=None, dlambda_var=None):
    """utils.py:1231-1269.  O(N) reductions of device vectors (host-side glue)."""
    r, f_mean, lambda_m, lambda_var = _cu(r), _cu(f_mean), _cu(lambda_m), _cu(lambda_var)
    A = math.exp(_scalar(f_params['logA']))
    lambda0 = _scalar(_lambda0_of(f_params))
    rlambda_m = torch.dot(r, lambda_m)
    sum_r = torch.sum(r)
    loglikelihood = A * rlambda_m + lambda0 * sum_r - torch.sum(f_mean)           # :1243
    if compute_grad_for_f_params:
        d = {'logA': A * (rlambda_m - torch.dot(lambda_m + A * lambda_var, f_mean))}   # :1253
        if 'loglambda0' in f_params:
            d['loglambda0'] = (sum_r - torch.sum(f_mean)) * lambda0               # :1254
        elif 'lambda0' in f_params:
            d['lambda0'] = sum_r - torch.sum(f_mean)                              # :1255
        return loglikelihood, d
    if dlambda_m is not None and dlambda_var is not None:
        d = {}
        for key in dlambda_m.keys():
            d[key] = (A * torch.dot(r, dlambda_m[key]) - A * torch.dot(f_mean, dlambda_m[key])
                      - 0.5 * A * A * torch.dot(f_mean, dlambda_var[key]))        # :1266
        return loglikelihood, d
    return loglikelihood, rlambda_m, sum_r


def compute_KL_div(m, V, K_tilde, K_tilde_inv, dK_tilde=None, ignore_warning=False):
    """KL(q || p) and its theta-gradients (utils.py:1306-1337); no -n/2 term (:1326)."""
    m, V, K_tilde, K_tilde_inv = _cu(m), _cu(V), _cu(K_tilde), _cu(K_tilde_inv)
    c = matmul(V, K_tilde_inv)                                                    # :1318
    b = matmul(K_tilde_inv, m)                                                    # :1320
    KL = (-0.5 * log_det(V, name='V', ignore_warning=ignore_warning) + 0.5 * log_det(K_tilde, name='K_tilde')
          + 0.5 * torch.dot(m, b) + 0.5 * torch.trace(c))                         # :1326
    if dK_tilde is None:
        return KL
    dKL = {}
    for key in dK_tilde.keys():
        Bk = matmul(dK_tilde[key], K_tilde_inv)                                   # :1331
        dKL[key] = 0.5 * torch.trace(Bk) - 0.5 * torch.sum(c * Bk.T) - 0.5 * torch.dot(b, matmul(Bk, m))  # :1333
    return KL, dKL


def Estep(r, KKtilde_inv, m, f_params, f_mean, K_tilde=None, K_tilde_inv=None, V=None, update_V_inv=False, alpha=1):
    """Newton update of (m, V) -- the update on V of the reference (update_V_inv=False; utils.py:1420-1439), with the
    full step (alpha = 1) or a damped one (0 < alpha < 1, which needs the current ``V``).

    alpha = 1: ``V = (I + K~ G)^-1 K~`` is evaluated in its symmetric form ``L (I + L^T G L)^-1 L^T`` (K~ = L L^T) with
    two MFMA Cholesky factorisations instead of the reference's LU solve.

    alpha != 1 (the remedy the reference's docs.md:18 names first when the E-step misbehaves, :1432-1436): the
    reference's ``V solve((1-a) K~ + a V + a K~ G V, K~)`` is ``V_new^-1 = (1-a) V^-1 + a (K~^-1 + G)``, a convex
    combination of positive definite precisions, and is evaluated as such from Cholesky factors only, as one device
    call (``gpfit_estep_projected_damped``): V_new is exactly symmetric and positive definite whenever V and K~ are.  A V
    that is not raises ``torch.linalg.LinAlgError`` ("Estep: V is not positive definite").  alpha outside (0, 1] is a
    ``ValueError``.

    ``update_V_inv=True`` is documented as not to be used (reference docs.md:5-7) and is not provided; neither is a
    call without ``K_tilde``, nor alpha != 1 without ``V``."""
    if not 0 < alpha <= 1:     # (also refuses NaN)
        raise ValueError(f'Estep: the step size alpha must lie in (0, 1], got {alpha}')
    if update_V_inv or K_tilde is None or (alpha != 1 and V is None):
        warnings.warn('Estep: only the update_V_inv = False update on V is implemented (alpha != 1 needs V)')
        raise NotImplementedError
    K_tilde = _cu(K_tilde)
    if alpha != 1:
        L, Linv, _, info = cholesky(K_tilde, want_inverse=True)
        if info != 0:
            raise torch.linalg.LinAlgError(f"Estep: K_tilde is not positive definite (info={info})")
        a = _cu(KKtilde_inv)
        return _estep_projected_damped(r, a, matmul(a, L), L, Linv, V, m, f_params, f_mean, alpha)
    L, _, _, info = cholesky(K_tilde)
    if info != 0:
        raise torch.linalg.LinAlgError(f"Estep: K_tilde is not positive definite (info={info})")
    return _estep_given_factor(r, KKtilde_inv, m, f_params, f_mean, L)


def _estep_given_factor(r, KKtilde_inv, m, f_params, f_mean, L):
    """The Newton update of ``Estep`` with the Cholesky factor ``L`` of K~ (in the basis in force) supplied: K~ only
    changes with theta, so ``varGP`` factors it once per EM iteration, not once per E-step (utils.py:1864-1881 runs
    ``nEstep`` updates between two kernel rebuilds)."""
    r, a, m, f_mean = _cu(r), _cu(KKtilde_inv), _cu(m), _cu(f_mean)
    A = math.exp(_scalar(f_params['logA']))
    g = A * matmul(a, r - f_mean, transA=True)                                    # :1421
    G = A * A * matmul(a, a * f_mean[:, None], transA=True)                       # :1422
    n = L.shape[0]
    W = matmul(L, matmul(G, L), transA=True)
    W = (W + W.T) * 0.5 + torch.eye(n, dtype=TORCH_DTYPE, device=W.device)
    _, Lwi, _, info = cholesky(W, want_inverse=True)
    if info != 0:
        raise torch.linalg.LinAlgError(f"Estep: I + L^T G L is not positive definite (info={info})")
    P = matmul(L, Lwi, transB=True)
    V_new = matmul(P, P, transB=True)                                             # = solve(I + K~G, K~), :1430
    m_new = matmul(V_new, matmul(G, m) + g)                                       # :1431
    V_new = (V_new + V_new.T) / 2                                                 # :1438
    return m_new, V_new


def _estep_projected(r, KKtilde_inv, aL, L, m, f_params, f_mean, kv0=None):
    """``_estep_given_factor`` as ONE device call (``gpfit_estep_projected``: W = I + (diag(A sqrt f) a L)^T (...),
    its factor and inverse, V = L W^-1 L^T, m = L W^-1 (a L)^T u), with ``aL = a L`` supplied by the caller -- like
    ``L`` it only changes when the kernel is rebuilt.  A lab-shaped fit (3160 / 2100 images, 30 x 10 E-steps) spends
    a third of its time in these updates when they are issued product by product.  With ``kv0 = Kvec - rowsum(K o a)``
    the call also returns the moments of lambda behind the update (what ``lambda_moments`` would compute next)."""
    r, a, aL, L, m, f_mean = _cu(r), _cu(KKtilde_inv), _cu(aL), _cu(L), _cu(m), _cu(f_mean)
    a, aL, L = a.contiguous(), aL.contiguous(), L.contiguous()
    N, nb = a.shape
    m_new = torch.empty(nb, dtype=TORCH_DTYPE, device=a.device)
    V_new = torch.empty((nb, nb), dtype=TORCH_DTYPE, device=a.device)
    eng = get_engine(max(N, nb), 1)
    lam_m = lam_var = None
    if kv0 is not None:
        kv0 = _cu(kv0).contiguous()
        lam_m = torch.empty(N, dtype=TORCH_DTYPE, device=a.device)
        lam_var = torch.empty(N, dtype=TORCH_DTYPE, device=a.device)
    rc = _lib.load().gpfit_estep_projected(eng._ctx, _stream(), a.data_ptr(), a.stride(0), aL.data_ptr(), aL.stride(0),
                                           L.data_ptr(), L.stride(0), N, nb, r.contiguous().data_ptr(),
                                           m.contiguous().data_ptr(), f_mean.contiguous().data_ptr(),
                                           _scalar(f_params['logA']), m_new.data_ptr(), V_new.data_ptr(), V_new.stride(0),
                                           kv0.data_ptr() if kv0 is not None else None,
                                           lam_m.data_ptr() if kv0 is not None else None,
                                           lam_var.data_ptr() if kv0 is not None else None)
    if rc > 0:
        raise torch.linalg.LinAlgError(f"Estep: I + L^T G L is not positive definite (info={rc})")
    if rc != 0:
        raise _lib.GpfitError(f"gpfit_estep_projected: {_lib.last_error()} (rc={rc})")
    if kv0 is not None:
        return m_new, V_new, lam_m, lam_var
    return m_new, V_new


_V_NOT_POSDEF = "Estep: V is not positive definite"


def _estep_projected_damped(r, KKtilde_inv, aL, L, Linv, V, m, f_params, f_mean, alpha):
    """The damped Newton update (``Estep`` with 0 < alpha <= 1, utils.py:1432-1436) as ONE device call
    (``gpfit_estep_projected_damped``): ``V_new^-1 = (1-a) V^-1 + a (K~^-1 + G)`` and ``m_new = (1-a) m + a m_full`` from
    Cholesky factors only, with ``L``, ``Linv = L^-1`` and ``aL = a L`` supplied by the caller (fixed between two kernel
    rebuilds) and the current ``V`` (symmetric; positive definite, or ``torch.linalg.LinAlgError`` beginning
    "Estep: V is not positive definite").  Returns ``(m_new, V_new)``, V_new exactly symmetric."""
    r, a, aL, L, Linv, V, m, f_mean = (_cu(r), _cu(KKtilde_inv), _cu(aL), _cu(L), _cu(Linv), _cu(V), _cu(m),
                                       _cu(f_mean))
    a, aL, L, Linv, V = a.contiguous(), aL.contiguous(), L.contiguous(), Linv.contiguous(), V.contiguous()
    N, nb = a.shape
    m_new = torch.empty(nb, dtype=TORCH_DTYPE, device=a.device)
    V_new = torch.empty((nb, nb), dtype=TORCH_DTYPE, device=a.device)
    eng = get_engine(max(N, nb), 1)
    info_v = ctypes.c_int(0)
    rc = _lib.load().gpfit_estep_projected_damped(
        eng._ctx, _stream(), a.data_ptr(), a.stride(0), aL.data_ptr(), aL.stride(0), L.data_ptr(), L.stride(0),
        Linv.data_ptr(), Linv.stride(0), V.data_ptr(), V.stride(0), N, nb, r.contiguous().data_ptr(),
        m.contiguous().data_ptr(), f_mean.contiguous().data_ptr(), _scalar(f_params['logA']), float(alpha),
        m_new.data_ptr(), V_new.data_ptr(), V_new.stride(0), ctypes.byref(info_v))
    if rc > 0 and info_v.value != 0:
        raise torch.linalg.LinAlgError(f"{_V_NOT_POSDEF}: the damped update needs a positive definite V "
                                       f"(info={info_v.value})")
    if rc > 0:
        raise torch.linalg.LinAlgError(f"Estep: I + L^T G L is not positive definite (info={rc})")
    if rc != 0:
        raise _lib.GpfitError(f"gpfit_estep_projected_damped: {_lib.last_error()} (rc={rc})")
    return m_new, V_new


CHAIN_MAX_STEPS = 1024   # GPFIT_ESTEP_CHAIN_MAX_STEPS of the C header
MAX_CHAIN_UNITS = 16     # GPFIT_ESTEP_CHAIN_MAX_UNITS of the C header
_FPARAM_LBFGS = (0.1, 1.e-7, 1.e-9)   # lr, tol_grad, tol_change of the rate-parameter optimiser inside a chain
_CELLS = threading.local()   # .rendezvous: the _ChainRendezvous of the varGP_cells wave this thread fits in; .engines


# ------------------------------------------------------------------ requests: what a device call of a fit is made of
# A call that the fits of a varGP_cells wave can share is prepared as a request: a dict with its ``kind`` (and, for a
# closure, its ``regime``), the operands on the device, the scalars, and the workspace (``engine``) and stream it runs
# on.  _REQUEST_KINDS (below the closures) describes each kind; the first four helpers here marshal a list of requests
# into the per-unit tables of a batch entry point, the fifth gives a request its workspace and stream.
def _ctx_table(ctxs):
    """The contexts of a batch call, given as engines' ``_ctx`` values or as raw integers."""
    return (ctypes.c_void_p * len(ctxs))(*[c.value if isinstance(c, ctypes.c_void_p) else c for c in ctxs])


def _ptr_table(qs, key):
    """One device pointer per request; a tensor given as None goes in as a null pointer."""
    return (ctypes.c_void_p * len(qs))(*[None if q[key] is None else q[key].data_ptr() for q in qs])


def _ld_table(qs, key, default, override=None):
    """One leading dimension per request: ``q[override]`` where a request has that field, else the tensor's, else
    ``q[default]`` when the tensor is None."""
    return (ctypes.c_int64 * len(qs))(*[q[override] if override in q else (q[default] if q[key] is None else q[key].stride(0))
                                        for q in qs])


def _flat(qs, key):
    """The per-request lists of floats ``q[key]``, one behind the other."""
    return _lib.darr([v for q in qs for v in q[key]])


def _request_place(q, engine, *size):
    """Where the request ``q`` runs: on the workspace ``engine``, or without one on this thread's for ``size`` (``n, d,
    d_full`` of ``get_engine``), and on the requesting thread's stream -- under ``varGP_cells`` another thread may issue
    the call.  Returns ``q``."""
    q["engine"] = engine if engine is not None else get_engine(*size)
    q["stream"] = _stream()
    return q


def _estep_chain(r, KKtilde_inv, aL, L, kv0, m, f_mean, logA0, n_steps, n_fparam_steps, lambda0_fixed=None, V=None,
                 lambda_m=None, lambda_var=None):
    """``n_steps`` E-steps between two kernel rebuilds (utils.py:1864-1934: ``_estep_projected`` with its moments, then
    ``_fparam_lbfgs``) as ONE device call and one wait (``gpfit_estep_chain``): ``logA``, ``lambda0`` and the rate stay
    on the device between the steps.  ``lambda0_fixed``: the optimiser's closure evaluates at this lambda0 (lambda0_mode
    1 of ``gpfit_fparam_lbfgs``); the rate it leaves for the next step is still the one at the closed-form lambda0, as
    that call leaves it, so this is not the host loop of a fit whose f_params carry loglambda0 (``varGP`` keeps the
    loop there).  Returns
    copies ``(m, V, lambda_m, lambda_var, f, records)`` of the state behind the last step that ran -- the arguments are
    left alone -- and one 12-number record per step (include/gpfit_mi355x.h); ``V``, ``lambda_m``, ``lambda_var`` given
    here are what comes back when no step commits.  In a fit of ``varGP_cells`` the device call is the wave's
    (``_submit``).  ``_estep_chain_commit`` turns the records into f_params or into the error of the first failing
    step."""
    return _submit(_chain_prepare(r, KKtilde_inv, aL, L, kv0, m, f_mean, logA0, n_steps, n_fparam_steps, lambda0_fixed, V,
                                  lambda_m, lambda_var))


def _estep_chain_full(r, K_tilde, kv0, m, f_mean, logA0, n_steps, n_fparam_steps, lambda0_fixed=None, V=None,
                      lambda_m=None, lambda_var=None):
    """``_estep_chain`` in the full-rank regime (inducing set = training set, every eigenvalue kept, identity basis):
    ``n_steps`` x (the update of ``gpfit_estep`` in the original basis, the moments ``lambda_m = m``, ``lambda_var =
    kv0 + diag(V)`` with ``kv0 = Kvec - diag(K~)``, then ``_fparam_lbfgs``) as ONE device call and one wait
    (``gpfit_estep_chain_full``).  Returns what ``_estep_chain`` returns: copies ``(m, V, lambda_m, lambda_var, f,
    records)`` of the state behind the last step that committed, the arguments left alone; ``lambda0_fixed`` as there.
    In a fit of ``varGP_cells`` the device call is the wave's (unless ``FULL_RANK_GROUPS`` is off): the request goes to
    the rendezvous and comes back as one unit of a ``gpfit_estep_chain_full_batch`` call, with the same bits.
    ``_estep_chain_full_commit`` turns the records into f_params or into the error of the first failing step."""
    return _submit(_chain_full_prepare(r, K_tilde, kv0, m, f_mean, logA0, n_steps, n_fparam_steps, lambda0_fixed, V,
                                       lambda_m, lambda_var))


def _estep_chain_damped(r, KKtilde_inv, aL, L, Linv, kv0, V, m, f_mean, logA0, alpha, n_steps, n_fparam_steps,
                        lambda0_fixed=None, lambda_m=None, lambda_var=None):
    """``n_steps`` damped E-steps between two kernel rebuilds (``_estep_projected_damped`` with step size ``alpha``, the
    moments of lambda at the committed ``(m, V)``, then ``_fparam_lbfgs``) as ONE device call and one wait
    (``gpfit_estep_chain_damped``).  ``V`` is the current covariance: step 0 reads it, step k what step k - 1 left.  A
    step whose ``V`` is not positive definite takes the full Newton step on the device, as the host loop of ``varGP``
    does, and says so in its record (slot 10 == 2).  Returns what ``_estep_chain`` returns: copies ``(m, V, lambda_m,
    lambda_var, f, records)``, the arguments left alone; ``lambda0_fixed`` as there.  In a fit of ``varGP_cells`` the
    device call is the wave's (``_submit``): the damped chains of equal key meet in one
    ``gpfit_estep_chain_damped_batch``.  ``_estep_chain_damped_commit`` turns the records into f_params, the warnings of
    the full steps and the error of the first failing step."""
    return _submit(_chain_damped_prepare(r, KKtilde_inv, aL, L, Linv, kv0, V, m, f_mean, logA0, alpha, n_steps,
                                         n_fparam_steps, lambda0_fixed, lambda_m, lambda_var))


def _chain_request(kind, operands, N, nv, m, f_mean, logA0, n_steps, n_fparam_steps, lambda0_fixed, V, lambda_m, lambda_var,
                   engine):
    """What the requests of the three chain kinds share: the fixed ``operands`` (name -> tensor, contiguous on the device),
    the scalars, the state ``(m, f, V, lam_m, lam_var)`` as copies of its own -- the call updates them in place, the
    arguments are left alone; ``V`` (nv x nv) and the moments (N) not given start uninitialised -- and the workspace and
    stream the call runs on, this thread's unless an engine is given."""
    dev = operands["r"].device

    def own(t, *shape):
        return torch.empty(shape, dtype=TORCH_DTYPE, device=dev) if t is None else _cu(t).clone().contiguous()
    q = {"kind": kind, **operands, "N": int(N), "logA0": float(logA0), "n_steps": int(n_steps), "nfp": int(n_fparam_steps),
         "lambda0_fixed": None if lambda0_fixed is None else float(lambda0_fixed)}
    q["m"], q["f"] = _cu(m).clone().contiguous(), _cu(f_mean).clone().contiguous()
    q["V"], q["lam_m"], q["lam_var"] = own(V, nv, nv), own(lambda_m, N), own(lambda_var, N)
    return _request_place(q, engine, max(N, nv), 1)


def _chain_prepare(r, KKtilde_inv, aL, L, kv0, m, f_mean, logA0, n_steps, n_fparam_steps, lambda0_fixed=None, V=None,
                   lambda_m=None, lambda_var=None, engine=None):
    """The arguments of ``_estep_chain`` as one request (kind ``"chain"``, ``_chain_request``)."""
    r, a, aL, L, kv0 = (_cu(t).contiguous() for t in (r, KKtilde_inv, aL, L, kv0))
    N, nb = a.shape
    q = _chain_request("chain", {"r": r, "a": a, "aL": aL, "L": L, "kv0": kv0}, N, nb, m, f_mean, logA0, n_steps,
                       n_fparam_steps, lambda0_fixed, V, lambda_m, lambda_var, engine)
    q["nb"] = int(nb)
    return q


def _chain_full_prepare(r, K_tilde, kv0, m, f_mean, logA0, n_steps, n_fparam_steps, lambda0_fixed=None, V=None,
                        lambda_m=None, lambda_var=None, engine=None):
    """The arguments of ``_estep_chain_full`` as one request (kind ``"chain_full"``, ``_chain_request``)."""
    r, K, kv0 = (_cu(t).contiguous() for t in (r, K_tilde, kv0))
    N = int(K.shape[0])
    return _chain_request("chain_full", {"r": r, "K": K, "kv0": kv0}, N, N, m, f_mean, logA0, n_steps, n_fparam_steps,
                          lambda0_fixed, V, lambda_m, lambda_var, engine)


def _chain_damped_prepare(r, KKtilde_inv, aL, L, Linv, kv0, V, m, f_mean, logA0, alpha, n_steps, n_fparam_steps,
                          lambda0_fixed=None, lambda_m=None, lambda_var=None, engine=None):
    """The arguments of ``_estep_chain_damped`` as one request (kind ``"chain_damped"``, ``_chain_request``)."""
    if not 0 < alpha <= 1:     # (also refuses NaN)
        raise ValueError(f'_estep_chain_damped: the step size alpha must lie in (0, 1], got {alpha}')
    r, a, aL, L, Linv, kv0 = (_cu(t).contiguous() for t in (r, KKtilde_inv, aL, L, Linv, kv0))
    N, nb = a.shape
    q = _chain_request("chain_damped", {"r": r, "a": a, "aL": aL, "L": L, "Linv": Linv, "kv0": kv0}, N, nb, m, f_mean, logA0,
                       n_steps, n_fparam_steps, lambda0_fixed, V, lambda_m, lambda_var, engine)
    q["nb"], q["alpha"] = int(nb), float(alpha)
    return q


def _chain_rec_array(q, n_units=1):
    """The array a chain call on ``n_units`` requests like ``q`` fills: one 12-number record (include/gpfit_mi355x.h) per
    step and unit."""
    return (ctypes.c_double * (12 * max(q["n_steps"], 1) * max(n_units, 1)))()


def _chain_result(q, u, rec):
    """What a chain call returns for its unit ``u``: the request's state, and the unit's records cut out of the flat
    array (a single call is unit 0 of its own array)."""
    first, n = 12 * q["n_steps"] * u, q["n_steps"]
    return q["m"], q["V"], q["lam_m"], q["lam_var"], q["f"], [list(rec[first + 12 * k:first + 12 * k + 12]) for k in range(n)]


# The argument lists of the three chain kinds (include/gpfit_mi355x.h) differ in three things: the matrices in front of
# N, a pointer and a leading dimension each; whether nb follows N -- the projected kinds, where it is also the leading
# dimension that goes with a null pointer (the full-rank kind has N for that, and takes a leading dimension given as
# q["ldk"] / q["ldv"] in place of the tensor's); and whether the step size alpha precedes lambda0_mode.
_CHAIN_HEADS = {"chain": (("a", "aL", "L"), True, False), "chain_full": (("K",), False, False),
                "chain_damped": (("a", "aL", "L", "Linv"), True, True)}


def _chain_call(kind, ctxs, qs, rec=None):
    """An entry point of the chain kind ``kind`` on the requests ``qs``: the batch one, ``gpfit_estep_<kind>_batch``, with
    the contexts ``ctxs`` (one per request), or with ``ctxs`` None the single one, ``gpfit_estep_<kind>``, on ``qs[0]``
    and its own workspace.  One list serves both: where the batch call takes a table with an entry per unit, the single
    call takes the entry of its one unit.  Returns the return code and the records, nothing checked here -- the shared
    arguments are those of ``qs[0]``, except that damped requests which disagree on the step size have none (NaN, which
    the entry point refuses).  A tensor given as None goes in as a null pointer; ``rec``: the caller's array instead of a
    new one."""
    heads, has_nb, has_alpha = _CHAIN_HEADS[kind]
    batch, q0, fixed = ctxs is not None, qs[0], qs[0]["lambda0_fixed"] is not None
    rec = _chain_rec_array(q0, len(qs)) if rec is None else rec
    ld_default, ld_given = ("nb", {}) if has_nb else ("N", {"K": "ldk", "V": "ldv"})

    def per_unit(table):
        return table if batch else table[0]

    def ptr(key):
        return per_unit(_ptr_table(qs, key))

    def ld(key):
        return per_unit(_ld_table(qs, key, ld_default, ld_given.get(key)))
    args = [v for key in heads for v in (ptr(key), ld(key))] + [q0["N"]]
    if has_nb:
        args.append(per_unit((ctypes.c_int64 * len(qs))(*[q["nb"] for q in qs])))
    args += [ptr("r"), ptr("kv0"), ptr("m"), ptr("f"), ptr("V"), ld("V"), ptr("lam_m"), ptr("lam_var"),
             per_unit(_lib.darr([q["logA0"] for q in qs]))]
    if has_alpha:
        args.append(q0["alpha"] if all(q["alpha"] == q0["alpha"] for q in qs) else float("nan"))
    args += [1 if fixed else 0, per_unit(_lib.darr([q["lambda0_fixed"] if fixed else 0.0 for q in qs])), q0["n_steps"],
             q0["nfp"], q0["nfp"], *_FPARAM_LBFGS, rec]
    where = (_ctx_table(ctxs), len(qs)) if batch else (q0["engine"]._ctx,)
    entry = getattr(_lib.load(), "gpfit_estep_" + kind + ("_batch" if batch else ""))
    return entry(*where, q0["stream"], *args), rec


def _chain_single(kind, q):
    """``gpfit_estep_<kind>`` on one request, checked: the request's state and its records (``_chain_result``)."""
    rc, rec = _chain_call(kind, None, [q])
    _lib.check(rc, "gpfit_estep_" + kind)
    return _chain_result(q, 0, rec)


def _chain_run_single(q):
    """``gpfit_estep_chain`` on one request."""
    return _chain_single("chain", q)


def _chain_full_run_single(q):
    """``gpfit_estep_chain_full`` on one request."""
    return _chain_single("chain_full", q)


def _chain_damped_run_single(q):
    """``gpfit_estep_chain_damped`` on one request."""
    return _chain_single("chain_damped", q)


def _chain_damped_bucket_key(q):
    """Requests with equal keys may share one ``gpfit_estep_chain_damped_batch`` call: the key of ``"chain"`` and the
    step size, which that call has one of."""
    return _chain_bucket_key(q) + (q["alpha"],)


def _chain_damped_batch_raw(ctxs, qs, rec=None):
    """``gpfit_estep_chain_damped_batch`` on the requests ``qs`` with the contexts ``ctxs`` (one per request): the return
    code and the records, unchecked (``_chain_call``); requests which disagree on the step size go in with NaN."""
    return _chain_call("chain_damped", ctxs, qs, rec)


def _chain_bucket_key(q):
    """Requests with equal keys may share one ``gpfit_estep_chain_batch`` call: what that call shares between its units,
    and the padded basis size (the recursion's split, hence the bits, depend on it)."""
    return (q["a"].device.index, q["stream"].value, q["N"], -(-q["nb"] // 128) * 128, q["n_steps"], q["nfp"],
            q["lambda0_fixed"] is not None)


def _chain_full_bucket_key(q):
    """Requests with equal keys may share one ``gpfit_estep_chain_full_batch`` call: what that call shares between its
    units."""
    return (q["K"].device.index, q["stream"].value, q["N"], q["n_steps"], q["nfp"], q["lambda0_fixed"] is not None)


def _chain_batch_raw(ctxs, qs, rec=None):
    """``gpfit_estep_chain_batch`` on the requests ``qs`` with the contexts ``ctxs`` (one per request): the return code
    and the records, unchecked (``_chain_call``)."""
    return _chain_call("chain", ctxs, qs, rec)


def _chain_full_batch_raw(ctxs, qs, rec=None):
    """``gpfit_estep_chain_full_batch`` on the requests ``qs`` with the contexts ``ctxs`` (one per request): the return
    code and the records, unchecked (``_chain_call``); a leading dimension given as ``q["ldk"]`` / ``q["ldv"]`` replaces
    the tensor's."""
    return _chain_call("chain_full", ctxs, qs, rec)


def _group_engines(count, n, d=1, d_full=1, exact=False):
    """``count`` workspaces of this thread for problems up to ``n`` stimuli (``d`` masked / ``d_full`` image pixels): its
    own (``get_engine``), then kept ones that fit, then new ones, which are kept for the thread's later group calls.
    ``exact``: every workspace of the call has the capacity of one created for exactly these ``n`` stimuli, whatever
    the size of the thread's own (a closure's slab counts and the route of its lift, hence its last bits, depend on the
    capacity)."""
    own = get_engine(n, d, d_full)
    kept = getattr(_CELLS, "engines", [])

    def fits(e):
        n_fits = -(-e.n_max // 128) == -(-n // 128) if exact else e.n_max >= n
        return n_fits and e.d_max >= d and e.d_full_max >= d_full and e.device == own.device
    mine = [own] if fits(own) else []      # without ``exact`` it always fits
    fitting = [e for e in kept if fits(e)]
    new = [GPFitEngine(n, d, d_full, device=own.device) for _ in range(count - len(mine) - len(fitting))]
    # the order of the kept list decides which workspaces a later call of another size meets first: it stays what each
    # rule has always left behind
    _CELLS.engines = kept + new if exact else fitting + new + [e for e in kept if e not in fitting]
    return (mine + fitting + new)[:count]


def _units_group(name, units, size, prepare, steps=None, exact=False, check=None):
    """What the ``*_group(units)`` functions of the request kinds share: 1 .. 16 units (then ``check(units)``, which raises
    for a list the wrapper refuses before any workspace is taken), one workspace each (``size(units)``: ``n, d, d_full``
    of ``_group_engines``, ``exact`` handed on), one request each (``prepare(engine=..., **unit)``) and one device call.
    Chains and the halves of a basis rebuild (``steps`` None) go to the batch entry point whatever their number: what
    ``_request_run_group`` returns.  A closure alone goes to the single entry point, and every closure is finished
    (``_closure_finish`` with ``steps``): a unit whose call would raise has the exception in its place."""
    if not 1 <= len(units) <= MAX_CHAIN_UNITS:
        raise ValueError(f"{name}: 1 .. {MAX_CHAIN_UNITS} units per call")
    if check is not None:
        check(units)
    engines = _group_engines(len(units), *size(units), exact=exact)
    qs = [prepare(engine=e, **u) for u, e in zip(units, engines)]
    if steps is None:
        return _request_run_group(qs)
    res = []
    for q, (rc_, out) in zip(qs, _request_run_group(qs) if len(qs) > 1 else [_request_run_single(qs[0])]):
        try:
            res.append(_closure_finish(q, rc_, out, steps))
        except Exception as err:      # what the closure raises for this unit alone
            res.append(err)
    return res


def _estep_chain_group(units, n_steps, n_fparam_steps):
    """``_estep_chain`` for several independent units (cells, restarts of one cell) as ONE device call
    (``gpfit_estep_chain_batch``).  ``units``: one dict per unit with the arguments of ``_estep_chain`` by name (``r``,
    ``KKtilde_inv``, ``aL``, ``L``, ``kv0``, ``m``, ``f_mean``, ``logA0`` and optionally ``lambda0_fixed``, ``V``,
    ``lambda_m``, ``lambda_var``); 1 .. 16 units with the same number of training points and the same
    ``round_up(nb, 128)``, all with or all without ``lambda0_fixed``.  Returns, per unit, what ``_estep_chain`` returns
    for it, bit for bit: a unit that fails stops alone."""
    return _units_group("_estep_chain_group", units, lambda us: (max(max(u["KKtilde_inv"].shape) for u in us),),
                        lambda **u: _chain_prepare(n_steps=n_steps, n_fparam_steps=n_fparam_steps, **u))


def _estep_chain_damped_group(units, alpha, n_steps, n_fparam_steps):
    """``_estep_chain_damped`` for several independent units as ONE device call (``gpfit_estep_chain_damped_batch``).
    ``units``: one dict per unit with the arguments of ``_estep_chain_damped`` by name (``r``, ``KKtilde_inv``, ``aL``,
    ``L``, ``Linv``, ``kv0``, ``V``, ``m``, ``f_mean``, ``logA0`` and optionally ``lambda0_fixed``, ``lambda_m``,
    ``lambda_var``); the step size ``alpha`` is the call's.  1 .. 16 units with the same number of training points and the
    same ``round_up(nb, 128)``, all with or all without ``lambda0_fixed``.  Returns, per unit, what ``_estep_chain_damped``
    returns for it, bit for bit: a unit that fails stops alone, a unit that takes the full step takes it alone."""
    return _units_group("_estep_chain_damped_group", units, lambda us: (max(max(u["KKtilde_inv"].shape) for u in us),),
                        lambda **u: _chain_damped_prepare(alpha=alpha, n_steps=n_steps, n_fparam_steps=n_fparam_steps, **u))


def _estep_chain_full_group(units, n_steps, n_fparam_steps):
    """``_estep_chain_full`` for several independent units (cells, restarts of one cell) as ONE device call
    (``gpfit_estep_chain_full_batch``).  ``units``: one dict per unit with the arguments of ``_estep_chain_full`` by name
    (``r``, ``K_tilde``, ``kv0``, ``m``, ``f_mean``, ``logA0`` and optionally ``lambda0_fixed``, ``V``, ``lambda_m``,
    ``lambda_var``); 1 .. 16 units with the same number of training points, all with or all without ``lambda0_fixed``.
    Returns, per unit, what ``_estep_chain_full`` returns for it, bit for bit: a unit that fails stops alone."""
    return _units_group("_estep_chain_full_group", units, lambda us: (max(u["K_tilde"].shape[0] for u in us),),
                        lambda **u: _chain_full_prepare(n_steps=n_steps, n_fparam_steps=n_fparam_steps, **u))


# ------------------------------------------------------------------ the sweeps of a basis rebuild as one device call
_SWEEPS_Y_READY, _SWEEPS_WANT_RR = 1, 2   # GPFIT_SWEEPS_Y_READY, GPFIT_SWEEPS_WANT_RR of the C header


def _sweeps_prepare(K, Q, Y=None, shifts=(), want_rr=True, engine=None):
    """The arguments of ``_basis_sweeps`` as one request: ``K`` as it is, the block as a copy of its own (the call updates
    it in place, the caller's ``Q`` is left alone), ``Y`` itself when given (it is the product ``K Q`` the plan formed, and
    the call's work block from then on), the second work block and ``S``, and the workspace and stream the call runs on,
    this thread's unless an engine is given.  float64 tensors on one device."""
    N, k = (int(v) for v in Q.shape)
    for t, shape in ((K, (N, N)), (Q, (N, k))) + (() if Y is None else ((Y, (N, k)),)):
        if t.dtype is not TORCH_DTYPE or tuple(t.shape) != shape or t.device != K.device:
            raise ValueError("_basis_sweeps: K [N, N], Q and Y [N, k] are float64 tensors on one device")
    K, Y = K.contiguous(), None if Y is None else Y.contiguous()

    def block(*shape):
        return torch.empty(shape, dtype=TORCH_DTYPE, device=K.device)
    q = {"kind": "sweeps", "K": K, "Q": Q.contiguous().clone(), "Y": block(N, k) if Y is None else Y, "W": block(N, k),
         "S": block(k, k) if want_rr else None, "N": N, "k": k, "shifts": [float(v) for v in shifts],
         "flags": (0 if Y is None else _SWEEPS_Y_READY) | (_SWEEPS_WANT_RR if want_rr else 0)}
    return _request_place(q, engine, k, 1)


def _sweeps_bucket_key(q):
    """Requests with equal keys may share one ``gpfit_subspace_sweeps_batch`` call: what that call shares between its
    units, and the capacity of their workspaces."""
    return (q["K"].device.index, q["stream"].value, q["N"], q["k"], q["flags"], -(-q["engine"].n_max // 128))


def _sweeps_batch_raw(ctxs, qs, rec=None):
    """``gpfit_subspace_sweeps_batch`` on the requests ``qs`` with the contexts ``ctxs`` (one per request): the return
    code and the ``(step, info)`` pairs, nothing checked here -- the shared arguments are those of ``qs[0]``.  A tensor
    given as None goes in as a null pointer; ``rec``: the caller's array instead of a new one."""
    q0 = qs[0]
    rec = (ctypes.c_int * (2 * len(qs)))() if rec is None else rec
    shifts = [_lib.darr(q["shifts"]) if q["shifts"] else None for q in qs]       # (kept alive until the call returns)
    sigma = (ctypes.c_void_p * len(qs))(*[None if a is None else ctypes.addressof(a) for a in shifts])
    rc = _lib.load().gpfit_subspace_sweeps_batch(
        _ctx_table(ctxs), len(qs), q0["stream"], _ptr_table(qs, "K"), q0["K"].stride(0) if q0["K"] is not None else q0["N"],
        q0["N"], q0["k"], _ptr_table(qs, "Q"), _ptr_table(qs, "Y"), _ptr_table(qs, "W"), _ptr_table(qs, "S"),
        (ctypes.c_int * len(qs))(*[len(q["shifts"]) for q in qs]), sigma, q0["flags"], rec)
    return rc, rec


def _sweeps_result(q, u, rec):
    """What a sweeps call returns for its unit ``u``: ``(Q, Y, S)`` of the request, or None when one of its Gram matrices
    was not positive definite (``rec``: the ``(step, info)`` pairs of the call)."""
    return None if rec[2 * u + 1] != 0 else (q["Q"], q["Y"], q["S"])


def _sweeps_run_single(q):
    """``gpfit_subspace_sweeps`` on one request."""
    rec = (ctypes.c_int * 2)()
    sigma = _lib.darr(q["shifts"]) if q["shifts"] else None
    K, S = q["K"], q["S"]
    _lib.check(_lib.load().gpfit_subspace_sweeps(q["engine"]._ctx, q["stream"], K.data_ptr(), K.stride(0), q["N"], q["k"],
                                                 q["Q"].data_ptr(), q["Y"].data_ptr(), q["W"].data_ptr(),
                                                 None if S is None else S.data_ptr(), len(q["shifts"]), sigma, q["flags"], rec),
               "gpfit_subspace_sweeps")
    return _sweeps_result(q, 0, rec)


def _basis_sweeps(K, Q, Y, shifts, want_rr):
    """The ``sweep_chain`` of ``eigtop.top_eigenpairs`` on the library: the rest of a pass of the subspace iteration --
    per shift ``Y = K Q`` (not for the first when ``Y`` is given), ``Y -= shift Q``, CholeskyQR (twice on the last) -- and
    the inputs of its Rayleigh-Ritz step as ONE device call and one wait (``gpfit_subspace_sweeps``) on the calling
    thread's workspace, with the bits of the loop through ``matmul`` and ``cholesky``.  Returns ``(Q, Y, S)`` as new
    tensors (``Y`` given is overwritten), or None when a Gram matrix was not positive definite.  With ``BASIS_GROUPS`` on,
    in a fit of ``varGP_cells`` the device call is the wave's (``_submit``)."""
    return _submit(_sweeps_prepare(K, Q, Y, shifts, want_rr))


def _basis_sweeps_group(units):
    """``_basis_sweeps`` for several independent units (cells: their kernel matrices and blocks) as ONE device call
    (``gpfit_subspace_sweeps_batch``).  ``units``: one dict per unit with the arguments of ``_basis_sweeps`` by name
    (``K``, ``Q``, ``shifts`` and optionally ``Y``, ``want_rr``); 1 .. 16 units of one ``(device, stream, N, k, flags,
    workspace capacity)`` -- all with or all without ``Y``, the same ``want_rr``; the numbers of shifts may differ --
    otherwise a ValueError before any call.  Returns, per unit, what ``_basis_sweeps`` returns for it, bit for bit: a
    unit whose factorisation fails has None in its place and stops alone."""
    return _units_group("_basis_sweeps_group", units, lambda us: (max(int(u["Q"].shape[1]) for u in us),), _sweeps_prepare,
                        exact=True)


# ------------------------------------------------------------------ the projector step of a basis rebuild as device calls
_SIGN_CAYLEY, _SIGN_X2_READY = 1, 2   # GPFIT_SIGN_CAYLEY, GPFIT_SIGN_X2_READY of the C header


def _sign_prepare(S, tau, X=None, X2=None, cs=(), its0=0, engine=None):
    """The arguments of ``_sign_steps`` as one request: ``S`` as it is (read only), ``X`` and ``X2`` themselves when given
    (the call's work blocks from then on: both are overwritten) or new blocks, the spare block, the schedule, and the
    workspace and stream the call runs on, this thread's unless an engine is given.  Without ``X`` the call forms it (the
    Cayley head); ``X2`` given is the product ``X X`` already.  float64 tensors on one device."""
    k = int(S.shape[0])
    if X is None and X2 is not None:
        raise ValueError("_sign_steps: X2 without X")
    for t in (S, X, X2):
        if t is not None and (t.dtype is not TORCH_DTYPE or tuple(t.shape) != (k, k) or t.device != S.device):
            raise ValueError("_sign_steps: S, X and X2 [k, k] are float64 tensors on one device")
    if (X is not None and not X.is_contiguous()) or (X2 is not None and not X2.is_contiguous()):
        raise ValueError("_sign_steps: X and X2 are contiguous (the call works in them)")

    def block():
        return torch.empty((k, k), dtype=TORCH_DTYPE, device=S.device)
    q = {"kind": "sign", "S": S.contiguous(), "tau": float(tau), "X": block() if X is None else X,
         "X2": block() if X2 is None else X2, "W": block(), "k": k, "c": [float(v) for v in cs], "its0": int(its0),
         "flags": (_SIGN_CAYLEY if X is None else 0) | (0 if X2 is None else _SIGN_X2_READY)}
    return _request_place(q, engine, k, 1)


def _sign_bucket_key(q):
    """Requests with equal keys may share one ``gpfit_sign_steps_batch`` call: what that call shares between its units
    -- the schedule among it -- and the capacity of their workspaces."""
    return (q["S"].device.index, q["stream"].value, q["k"], q["flags"], q["its0"], tuple(q["c"]),
            -(-q["engine"].n_max // 128))


def _sign_batch_raw(ctxs, qs, rec=None):
    """``gpfit_sign_steps_batch`` on the requests ``qs`` with the contexts ``ctxs`` (one per request): the return code and
    the ``(steps, info)`` pairs, nothing checked here -- the shared arguments are those of ``qs[0]``.  A tensor given as
    None goes in as a null pointer; ``rec``: the caller's array instead of a new one."""
    q0 = qs[0]
    rec = (ctypes.c_int * (2 * len(qs)))() if rec is None else rec
    rc = _lib.load().gpfit_sign_steps_batch(
        _ctx_table(ctxs), len(qs), q0["stream"], _ptr_table(qs, "S"), q0["k"], _lib.darr([q["tau"] for q in qs]),
        _ptr_table(qs, "X"), _ptr_table(qs, "X2"), _ptr_table(qs, "W"), len(q0["c"]), _lib.darr(q0["c"]) if q0["c"] else None,
        q0["its0"], q0["flags"], rec)
    return rc, rec


def _sign_result(q, u, rec):
    """What a sign call returns for its unit ``u``: ``(X, X2)``, or None when ``S + tau I`` was not positive definite
    (``rec``: the ``(steps, info)`` pairs of the call).  X and the spare block change places with every step."""
    if rec[2 * u + 1] != 0:
        return None
    return (q["W"] if len(q["c"]) & 1 else q["X"]), q["X2"]


def _sign_run_single(q):
    """``gpfit_sign_steps`` on one request."""
    rec = (ctypes.c_int * 2)()
    _lib.check(_lib.load().gpfit_sign_steps(q["engine"]._ctx, q["stream"], q["S"].data_ptr(), q["k"], q["tau"],
                                            q["X"].data_ptr(), q["X2"].data_ptr(), q["W"].data_ptr(), len(q["c"]),
                                            _lib.darr(q["c"]) if q["c"] else None, q["its0"], q["flags"], rec),
               "gpfit_sign_steps")
    return _sign_result(q, 0, rec)


def _sign_steps(S, tau, X, X2, cs, its0):
    """The ``sign_chain`` of ``eigtop._kept_subspace`` on the library: a stretch of the projector step -- the Cayley
    transform of ``S`` when ``X`` is None, one step of the scaled sign iteration per scaling of ``cs`` (``X2`` given is the
    first step's ``X X``), the symmetrisation where ``its0`` + the step's index is 7 mod 8, and the product ``X X`` behind
    the last step -- as ONE device call and one wait (``gpfit_sign_steps``) on the calling thread's workspace, with the
    bits of the loop through ``cholesky``, ``matmul`` and ``gemm_into``.  Returns ``(X, X2)`` (``X`` and ``X2`` given are
    overwritten; ``S`` is left alone), or None when ``S + tau I`` was not positive definite.  With ``BASIS_GROUPS`` on, in
    a fit of ``varGP_cells`` the device call is the wave's (``_submit``)."""
    return _submit(_sign_prepare(S, tau, X, X2, cs, its0))


def _sign_steps_group(units):
    """``_sign_steps`` for several independent units (cells: their Rayleigh quotient matrices) as ONE device call
    (``gpfit_sign_steps_batch``).  ``units``: one dict per unit with the arguments of ``_sign_steps`` by name (``S``,
    ``tau``, ``cs`` and optionally ``X``, ``X2``, ``its0``); 1 .. 16 units of one ``(device, stream, k, flags, its0, cs,
    workspace capacity)`` -- all with or all without ``X``, all with or all without ``X2``, the same schedule -- otherwise a
    ValueError before any call.  Returns, per unit, what ``_sign_steps`` returns for it, bit for bit: a unit whose
    factorisation fails has None in its place and fails alone."""
    def check(us):
        if len({(int(u["S"].shape[0]), u.get("X") is None, u.get("X2") is None, int(u.get("its0", 0)),
                 tuple(float(v) for v in u["cs"])) for u in us}) != 1:
            raise ValueError("_sign_steps_group: the units of one call share k, the flags (all with or all without X and X2) "
                             "and the schedule (its0 and cs)")
    return _units_group("_sign_steps_group", units, lambda us: (int(us[0]["S"].shape[0]),), _sign_prepare, exact=True,
                        check=check)


# The books: the prefixes of the counters a call of the rendezvous is counted in, each named by the records of
# _REQUEST_KINDS whose calls it counts.
_ALL_BOOKS = ("", "closure_", "full_", "full_closure_", "loss_", "basis_")


class _ChainRendezvous:
    """Where the fits of one ``varGP_cells`` wave meet.  Each of ``parties`` host threads runs one fit; a fit that
    reaches a device call that the wave shares hands its request to ``call`` and waits.  When every fit still alive has
    arrived, the last one to arrive sorts the requests into buckets by ``key`` and issues ``group`` once per bucket (``single`` for a
    bucket of one, ``group`` in slices of ``max_units`` for a larger one), then hands every fit its result.  A fit's
    thread starts with ``enter``; a fit that ends, fails or will never ask (``leave``) is no longer waited for.  An
    exception of a call is raised in every fit whose request was part of that call.  ``group_sizes``: the units of
    every call issued, in order.

    A wave's fits hand in the nine kinds of request of ``_REQUEST_KINDS`` -- the E-step chains, the M-step closures of
    their L-BFGS, whose line searches differ from cell to cell, the loss evaluations, the halves of the basis rebuilds
    -- so at any moment some fits wait with a closure and others with a chain.  The rendezvous does not tell them
    apart: ``single``, ``group`` and ``key`` dispatch on the request's kind, and ``key`` carries the kind, so two kinds
    never share a call.  Only the bookkeeping looks at it: per book of ``_ALL_BOOKS`` there are three counters,
    ``<book>group_sizes`` / ``<book>call_seconds`` / ``seconds_in_<book>call``, and a call is counted in the book of its
    kind -- the projected chains, damped ones among them, in ``""`` (a request without a kind included), the sparse and
    truncated closures in ``"closure_"``, and the full-rank regime in two books of its own, its chains in ``"full_"``
    and its closures in ``"full_closure_"``; the loss evaluations of every regime in ``"loss_"``; the sweeps and the sign
    stretches of the basis rebuilds, when they come here (``BASIS_GROUPS``), in ``"basis_"``."""

    def __init__(self, parties, single, group, key, max_units=MAX_CHAIN_UNITS):
        self.cond = threading.Condition()
        # between two chains only one fit runs at a time (enter / call / leave pass the turn on): the fits then never
        # compete for the interpreter or wait behind each other's launches on the shared stream, and the phase times a
        # fit reports are its own costs
        self.turn = threading.Lock()
        self.alive = int(parties)
        self.single, self.group, self.key, self.max_units = single, group, key, int(max_units)
        self.waiting = {}      # ticket -> request
        self.results = {}      # ticket -> result or exception
        for book in _ALL_BOOKS:
            setattr(self, book + "group_sizes", [])        # the units of every call issued, in order
            setattr(self, book + "call_seconds", [])       # host wall time of each of them (enqueue to results)
            # summed over the fits: time between handing a request in and getting its result
            setattr(self, "seconds_in_" + book + "call", 0.0)

    @staticmethod
    def _book(request):
        """The prefix of the three counters a request is counted in."""
        if not isinstance(request, dict) or request.get("kind") is None:
            return ""
        return _request_kind(request).book

    def enter(self):
        """First statement of a fit's thread: wait for the turn."""
        self.turn.acquire()

    def leave(self):
        self.turn.release()
        with self.cond:
            self.alive -= 1
            if self.waiting and len(self.waiting) >= self.alive:
                self._issue()

    def call(self, request):
        ticket = object()
        t_in = time.perf_counter()
        self.turn.release()
        with self.cond:
            self.waiting[ticket] = request
            if len(self.waiting) >= self.alive:
                self._issue()
            while ticket not in self.results:
                self.cond.wait()
            res = self.results.pop(ticket)
        self.turn.acquire()
        with self.cond:
            name = "seconds_in_" + self._book(request) + "call"
            setattr(self, name, getattr(self, name) + time.perf_counter() - t_in)
        if isinstance(res, BaseException):
            raise res
        return res

    def _issue(self):
        """Run every waiting request (the lock is held: every other live fit is waiting for exactly this)."""
        buckets = {}
        for ticket, q in self.waiting.items():
            buckets.setdefault(self.key(q), []).append(ticket)
        for tickets in buckets.values():
            for i in range(0, len(tickets), self.max_units):
                part = tickets[i:i + self.max_units]
                book = self._book(self.waiting[part[0]])
                getattr(self, book + "group_sizes").append(len(part))
                t_call = time.perf_counter()
                try:
                    if len(part) == 1:
                        out = [self.single(self.waiting[part[0]])]
                    else:
                        out = self.group([self.waiting[t] for t in part])
                        if len(out) != len(part):
                            raise RuntimeError("the group call returned a result list of the wrong length")
                except BaseException as err:      # handed to every participant, also a KeyboardInterrupt
                    out = [err] * len(part)
                getattr(self, book + "call_seconds").append(time.perf_counter() - t_call)
                for t, res in zip(part, out):
                    self.results[t] = res
        self.waiting.clear()
        self.cond.notify_all()


def _cells_withdraw():
    """A fit of a ``varGP_cells`` wave that will never ask for a chain says so: the others stop waiting for it."""
    rendezvous = getattr(_CELLS, "rendezvous", None)
    if rendezvous is not None:
        _CELLS.rendezvous = None
        rendezvous.leave()


_IDLE_ENGINES = []   # workspaces of finished varGP_cells fits (guarded by _POOL.lock), adopted by the fits of the next wave


def release_cell_workspaces():
    """Free the workspaces ``varGP_cells`` keeps between calls."""
    with _POOL.lock:
        _IDLE_ENGINES.clear()


_CELLS_COUNTERS = tuple(name for book in _ALL_BOOKS for name in (book + "group_sizes", book + "call_seconds",
                                                              "seconds_in_" + book + "call"))


def varGP_cells(x, r_list, kwargs_list, max_units=MAX_CHAIN_UNITS):
    """Fit several cells recorded on the same stimuli ``x`` (or several restarts of one cell): returns the list of
    ``(fit_model, err_dict)`` that ``varGP(x, r_list[i], **kwargs_list[i])`` returns, fit by fit.

    The wave.  The fits run ``max_units`` (at most 16) at a time, one host thread each with its own workspace, all on
    the caller's current stream.  ``varGP`` itself is unchanged; where a fit would issue a device call of one of the
    kinds below, it waits until every fit of its wave that is still running waits as well -- some with a closure of
    their L-BFGS, some already with their next chain -- and the waiting requests go out as ONE call per kind and group
    of equal key (``_REQUEST_KINDS``, ``_request_bucket_key``); two kinds never share a call.  Each cell's numbers are
    those of ``varGP`` on its own, bit for bit.  Between two calls the fits of a wave take turns, one running at a
    time, so the phase times a fit prints are its own -- except that its E-step time contains the wait for the others.
    Fits that never chain (f_params carrying ``loglambda0``, ``estep_alpha != 1`` without the damped chain,
    ``GPFIT_ESTEP_CHAIN=0``) run beside the others without being waited for.  A fit that fails returns its ``err_dict`` as ``varGP`` does, and an error of a group call is the
    error of every fit in that call.  Out of the groups stay the fp32 instance and, unless ``BASIS_GROUPS`` is on, the basis
    rebuilds.

    Projected chains (``_estep_chain``: the E-steps of an EM iteration as one device call, truncated and sparse
    regimes): ONE ``gpfit_estep_chain_batch`` call per group of equal ``(N, round_up(nb, 128), nEstep, nFparamstep,
    lambda0 mode)`` -- the small kernels and the bottom of the Cholesky recursions cost one launch for the group
    instead of one per cell.

    Damped chains (``_estep_chain_damped``: ``estep_alpha != 1`` with ``DAMPED_CHAIN`` or the fit's
    ``estep_damped_chain`` on, every regime): ONE ``gpfit_estep_chain_damped_batch`` call per group of equal key of the
    projected chains and equal ``alpha``; counted with the projected chains.

    Full-rank chains (``_estep_chain_full``: inducing set = training set, every eigenvalue kept, identity basis): ONE
    ``gpfit_estep_chain_full_batch`` call per group of equal ``(N, nEstep, nFparamstep, lambda0 mode)``; they never
    share a call with the projected chains.

    Sparse closures (``_closure_sparse``, the M-step closures of a fit with ``ntilde < ntrain``): ONE
    ``gpfit_fit_eval_sparse_batch`` call per group of equal ``_closure_bucket_key``.  A closure that returns the
    infinite loss on the host (theta outside the limits) asks nothing.

    Truncated-rank closures (``_closure_projected``: ``ntilde == ntrain`` with eigenvalues dropped): ONE
    ``gpfit_fit_eval_projected_batch`` call per group of equal key.  The regime is part of the key, so the two never
    share a call; so is the capacity of the fit's workspace.

    Full-rank closures (``_closure_full``): ONE ``gpfit_fit_eval_batch`` call on the fits' own workspaces per group of
    equal ``_closure_full_bucket_key`` -- the ``reuse_V`` flag is part of it, so the first closures of an M-step and
    later ones never share a call; a unit whose factorisation fails is that fit's error alone.  With
    ``FULL_RANK_GROUPS`` off (``GPFIT_FULL_RANK_GROUPS=0``) a full-rank fit issues its chains and closures directly on
    its own workspace and keeps its turn until it ends.

    Loss evaluations (``elbo_terms``: the tracked loss before the first iteration, behind every chain and after a
    roll-back, in every regime): ONE ``gpfit_elbo_batch`` call per group of equal ``(N, round_up(nb, 128))``.  A fit
    that has withdrawn from the wave, and any fit with ``FUSED_LOSS`` off, evaluates its loss on its own.

    Basis rebuilds (``_basis_sweeps``, ``_sign_steps``; only with ``BASIS_GROUPS`` on, ``GPFIT_BASIS_GROUPS=1``): ONE
    ``gpfit_subspace_sweeps_batch`` call per group of equal ``_sweeps_bucket_key`` for the sweeps of a pass, and ONE
    ``gpfit_sign_steps_batch`` call per group of equal ``_sign_bucket_key`` -- the schedule of scalings is part of it, so
    the first stretches of the fits' sign iterations share a call and a straggler's second stretch usually runs alone.
    Off (the default), a wave issues exactly the calls it issues without the switch.

    The counters.  ``varGP_cells.last_group_sizes``: the units of every projected chain call of the last invocation, in
    order (1: the single call); ``last_call_seconds``: the host wall time of each of those calls;
    ``last_seconds_in_call``: summed over the fits, the time between handing a request in and getting its result
    (waiting for the wave plus the call).  ``last_closure_group_sizes``, ``last_closure_call_seconds`` and ``last_seconds_in_closure_call``: the same
    for the sparse and truncated closure calls.  The calls of the full-rank regime are counted apart, in
    ``last_full_group_sizes`` / ``last_full_call_seconds`` / ``last_seconds_in_full_call`` (chains) and
    ``last_full_closure_group_sizes`` / ``last_full_closure_call_seconds`` / ``last_seconds_in_full_closure_call``
    (closures); the loss calls in ``last_loss_group_sizes`` / ``last_loss_call_seconds`` / ``last_seconds_in_loss_call``; the sweeps
    and sign calls of the basis rebuilds in ``last_basis_group_sizes`` / ``last_basis_call_seconds`` /
    ``last_seconds_in_basis_call``.
    The workspaces of the fits (one per concurrent fit, each of the size of a ``varGP`` workspace) are
    kept for the next call; ``release_cell_workspaces()`` frees them."""
    n_fits = len(r_list)
    if len(kwargs_list) != n_fits:
        raise ValueError("varGP_cells: one kwargs dict per response vector")
    max_units = int(max_units)
    if not 1 <= max_units <= MAX_CHAIN_UNITS:
        raise ValueError(f"varGP_cells: max_units must be within 1 .. {MAX_CHAIN_UNITS}")
    dev = _device()
    stream = torch.cuda.current_stream(dev)
    grad = torch.is_grad_enabled()
    results, errors = [None] * n_fits, [None] * n_fits
    counters = {name: 0.0 if name.startswith("seconds_in_") else [] for name in _CELLS_COUNTERS}

    def fit(i, rendezvous):
        key = (dev.index, threading.get_ident())
        _CELLS.rendezvous = rendezvous
        rendezvous.enter()
        try:
            torch.cuda.set_device(dev)
            torch.set_grad_enabled(grad)      # per thread in torch: as in the caller's
            with _POOL.lock:                  # a workspace an earlier fit has left behind, if there is one
                idle = [e for e in _IDLE_ENGINES if e.device == dev.index]
                if idle:
                    _IDLE_ENGINES.remove(idle[-1])
                    _POOL.eng[key] = idle[-1]
            with torch.cuda.stream(stream):
                results[i] = varGP(x, r_list[i], **kwargs_list[i])
        except BaseException as err:          # what varGP itself raises (bad arguments): re-raised in the caller below
            errors[i] = err
        finally:
            _cells_withdraw()
            with _POOL.lock:                  # the thread ends here: its workspace serves the next wave or call
                e = _POOL.eng.pop(key, None)
                if e is not None and len(_IDLE_ENGINES) < MAX_CHAIN_UNITS:
                    _IDLE_ENGINES.append(e)

    for first in range(0, n_fits, max_units):
        wave = range(first, min(n_fits, first + max_units))
        rendezvous = _ChainRendezvous(len(wave), _request_run_single, _request_run_group, _request_bucket_key, max_units)
        threads = [threading.Thread(target=fit, args=(i, rendezvous), name=f"varGP_cells-{i}") for i in wave]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        for name in counters:
            counters[name] += getattr(rendezvous, name)
    for name, value in counters.items():
        setattr(varGP_cells, "last_" + name, value)
    for err in errors:
        if err is not None:
            raise err
    return results


for _name in _CELLS_COUNTERS:
    setattr(varGP_cells, "last_" + _name, 0.0 if _name.startswith("seconds_in_") else [])
del _name


def _estep_chain_commit(records, f_params):
    """Walk the records of ``_estep_chain`` as the host loop would have met them: ``f_params['logA']`` is filled in
    place and ``f_params['lambda0']`` set after every step that ran; the first failing step raises what
    ``_estep_projected`` / ``_fparam_lbfgs`` raise for it.  Returns the last record."""
    for k, rec in enumerate(records):
        if rec[9] != 0:
            raise torch.linalg.LinAlgError(f"Estep: I + L^T G L is not positive definite (info={int(rec[9])})")
        if rec[10] != 1:
            raise _lib.GpfitError(f"gpfit_estep_chain: step {k} was skipped without a failing step before it")
        status = int(rec[6])
        with torch.no_grad():
            f_params['logA'].fill_(rec[7] if status else rec[0])      # the same tensor, as LBFGS's p.add_ leaves it
        f_params['lambda0'] = torch.tensor(rec[8] if status else rec[1], dtype=TORCH_DTYPE)
        if status:
            raise ValueError(f'Nan in f_mean during f param update in Estep, closure has been called {status} times in '
                             f'estep {k} iteration.')                                                        # :1923
    return records[-1]


_FULL_STEP_WARNING = ('varGP: V_b is not positive definite in E-step {} of iteration {}; this update takes the full Newton '
                      'step (alpha = 1)')


def _estep_chain_damped_commit(records, f_params, iteration, full_steps):
    """``_estep_chain_commit`` for the records of ``_estep_chain_damped`` in EM iteration ``iteration``: a record whose
    slot 10 reads 2 was committed as the full Newton step because V_b was not positive definite -- it raises the warning
    the host loop raises for that update and counts in ``full_steps[0]``; the warnings go in step order and precede the
    error of a later step (behind a failing step every record is zero).  Returns the last record."""
    committed = []
    for k, rec in enumerate(records):
        if rec[10] == 2:
            warnings.warn(_FULL_STEP_WARNING.format(k, iteration))
            full_steps[0] += 1
            rec = list(rec[:10]) + [1.0] + list(rec[11:])
        committed.append(rec)
    return _estep_chain_commit(committed, f_params)


def _estep_chain_full_commit(records, f_params, f_mean):
    """``_estep_chain_commit`` for the records of ``_estep_chain_full``: the errors are those of the host loop around
    ``gpfit_estep``.  A step whose I + S K S is not positive definite raises the loop's ValueError when the rate it read
    is not finite (``f_mean``: the rate the chain returns -- a step that commits nothing leaves it as it read it), its
    LinAlgError otherwise; every other step is handed to ``_estep_chain_commit``."""
    for k, rec in enumerate(records):
        if rec[9] != 0:
            if k > 0:
                _estep_chain_commit(records[:k], f_params)
            if not bool(torch.isfinite(f_mean).all()):
                # the reference's LU solve lets NaNs through and reports them one step later, in the rate-parameter
                # closure (utils.py:1923-1924)
                raise ValueError(f'Nan in f_mean during f param update in Estep, closure has been called 1 times in '
                                 f'estep {k} iteration. Try substituting them with inf.')
            raise torch.linalg.LinAlgError("Estep: gpfit_estep: I + S K S is not positive definite (is K_tilde symmetric "
                                           f"positive definite?) (rc={int(rec[9])})")
    return _estep_chain_commit(records, f_params)


# ------------------------------------------------------------------ inference
def lambda_moments_star(xstar, xtilde, C, theta, K_tilde, K_tilde_inv, m, V, B, kernfun):
    """Predictive moments of lambda at test points (utils.py:1476-1500).  ``xstar`` may hold
    several rows: the reference's one-row-at-a-time loop (utils.py:388-397) is batched."""
    if kernfun == 'acosker':
        kernfun = acosker
    elif not callable(kernfun):
        raise Exception('Kernel function not recognized')
    Kvec_star = kernfun(theta, xstar, xtilde, C=C, dC=None, diag=False)          # :1486
    if not _is_identity(B):
        Kvec_star = matmul(Kvec_star, B)                                          # :1487
    a = matmul(Kvec_star, K_tilde_inv)                                            # :1489
    mu_star = matmul(a, m)                                                        # :1491
    K_star = kernfun(theta, xstar, x2=None, C=C, dC=None, diag=True)              # :1494
    sigma_star2 = K_star + torch.sum(matmul(a, _cu(V) - _cu(K_tilde)) * a, 1)     # :1498
    return mu_star, torch.reshape(sigma_star2, (_cu(xstar).reshape(-1, _cu(xstar).shape[-1]).shape[0],))


# Rows of a pool that the workspace of pool_moments / score_pool is sized for (when the model itself is smaller): a
# chunk of the pool is at most as long as the workspace, and short chunks leave the quadratic-form launch too few
# tiles to fill the chip (profiles/r25_score_pool.txt).  ``reserve`` more rows beforehand for longer chunks.
POOL_ROWS = 4096


def fold_posterior(K_tilde, K_tilde_inv, m, V, B):
    """What a prediction needs of the posterior, formed once per model for ``pool_moments`` / ``score_pool``:
    ``w = K~_b^-1 m_b`` and the symmetric ``S = K~_b^-1 (V_b - K~_b) K~_b^-1`` (utils.py:1489-1498 with the products
    re-associated).  ``K_tilde``, ``K_tilde_inv``, ``m`` and ``V`` are in the basis ``B`` (any orthonormal one), exactly
    as ``lambda_moments_star`` takes them.  Returns a dict with ``S``, ``w``, ``B`` (None for the identity) and ``k``;
    ``pool_moments`` / ``score_pool`` keep the pixel list of their ``mask`` (and the masked copy of unmasked inducing
    images) in it under private keys, formed on the first call with that mask and reused while the same tensors are
    passed (a mask changed in place needs a new fold)."""
    Ki = _cu(K_tilde_inv)
    w = matmul(Ki, _cu(m).reshape(-1))
    S = matmul(matmul(Ki, _cu(V) - _cu(K_tilde)), Ki, transB=True)
    S = (0.5 * (S + S.T)).contiguous()
    return {"S": S, "w": w.reshape(-1).contiguous(), "B": None if _is_identity(B) else _cu(B), "k": int(S.shape[0])}


def _score_pool_prepare(xstar, xtilde, C, theta, folded, mask):
    """The operands of one ``gpfit_score_pool`` unit, checked, as a request: the tensors on the device (``pix`` None for
    a pool that is already masked), the sizes and ``sigma0``."""
    dev = _device()
    C = _cu(C)
    d = C.shape[0]
    xtilde_given = xtilde
    xstar, xtilde = _cu(xstar), _cu(xtilde)
    xstar = xstar.reshape(-1, xstar.shape[-1])
    if xtilde.dim() == 1:
        xtilde = xtilde[None, :]
    pix, d_full = None, d
    if mask is not None:
        # the pixel list and the masked inducing images belong to the model: formed on the first call (the one host
        # synchronisation of the mask path, in torch.nonzero) and kept with the folded posterior, keyed on the caller's
        # tensors themselves, so that later calls on the same model enqueue the device call and nothing else
        kept = folded.get("_pixels")
        if kept is None or kept[0] is not mask:
            mk = torch.as_tensor(mask).to(dev).reshape(-1).to(torch.bool)
            kept = folded["_pixels"] = (mask, mk, torch.nonzero(mk).reshape(-1).to(torch.int32).contiguous())
        _, mk, pix = kept
        d_full = mk.numel()
        if pix.numel() != d or xstar.shape[1] != d_full:
            raise RuntimeError(f"score_pool: the mask keeps {pix.numel()} of {d_full} pixels but C is {tuple(C.shape)} and "
                               f"xstar has {xstar.shape[1]} columns")
        if xtilde.shape[1] == d_full and d_full != d:     # inducing images given unmasked as well
            kept = folded.get("_xtilde")
            if kept is None or kept[0] is not xtilde_given or kept[1] is not mask:
                kept = folded["_xtilde"] = (xtilde_given, mask, xtilde[:, mk].contiguous())
            xtilde = kept[2]
    if xstar.shape[1] != d_full or xtilde.shape[1] != d or C.shape != (d, d):
        raise RuntimeError("score_pool: xstar, xtilde and C disagree on the number of pixels")
    S, w, B, k = folded["S"], folded["w"], folded["B"], int(folded["k"])
    nt, P = xtilde.shape[0], xstar.shape[0]
    if tuple(S.shape) != (k, k) or w.numel() != k or (B is None and k != nt) or (B is not None and tuple(B.shape) != (nt, k)):
        raise RuntimeError("score_pool: the folded posterior does not fit the inducing set")
    return {"xstar": xstar, "xtilde": xtilde, "C": C, "pix": pix, "d": d, "d_full": d_full, "nt": nt, "P": P, "S": S, "w": w,
            "B": B, "k": k, "sigma0": _scalar(theta["sigma_0"])}


def _pool_chunk_rows(chunk_rows):
    chunk_rows = int(chunk_rows)
    if chunk_rows < 0 or chunk_rows % 128:
        raise ValueError("chunk_rows must be 0 (the workspace's capacity) or a multiple of 128")
    return chunk_rows


def _pool_workspace_rows(q):
    """Stimuli the workspace of a pool call is sized for (``POOL_ROWS``)."""
    return max(q["nt"], q["k"], min(q["P"], POOL_ROWS))


def _score_pool_call(xstar, xtilde, C, theta, folded, A, lambda0, r_masked, mask, chunk_rows, want_rate, out=None):
    """One ``gpfit_score_pool`` call on this thread's workspace; returns (mu, sigma2, rate or None, utility or None).
    ``out``: the caller's four float64 device vectors of P elements in place of new ones (``score_pool_cells``: rows of
    its tables; the last is ignored without ``r_masked``)."""
    lib = _lib.load()
    dev = _device()
    chunk_rows = _pool_chunk_rows(chunk_rows)
    q = _score_pool_prepare(xstar, xtilde, C, theta, folded, mask)
    xstar, xtilde, C, pix, S, w, B = (q[key] for key in ("xstar", "xtilde", "C", "pix", "S", "w", "B"))
    d, d_full, nt, P, k = (q[key] for key in ("d", "d_full", "nt", "P", "k"))
    r = _cu(r_masked).reshape(-1).contiguous() if r_masked is not None else None
    if out is None:
        mu = torch.empty(P, dtype=TORCH_DTYPE, device=dev)
        sigma2 = torch.empty(P, dtype=TORCH_DTYPE, device=dev)
        rate = torch.empty(P, dtype=TORCH_DTYPE, device=dev) if want_rate else None
        U = torch.empty(P, dtype=TORCH_DTYPE, device=dev) if r is not None else None
    else:
        mu, sigma2, rate, U = out[0], out[1], out[2], out[3] if r is not None else None
    if P == 0:
        return mu, sigma2, rate, U
    eng = get_engine(_pool_workspace_rows(q), d, d_full)
    _lib.check(lib.gpfit_score_pool(eng._ctx, _stream(), q["sigma0"], xstar.data_ptr(), xstar.stride(0), P,
                                    pix.data_ptr() if pix is not None else None, d_full, xtilde.data_ptr(),
                                    xtilde.stride(0), nt, d, C.data_ptr(), C.stride(0),
                                    B.data_ptr() if B is not None else None, B.stride(0) if B is not None else 0, k,
                                    S.data_ptr(), S.stride(0), w.data_ptr(), float(A), float(lambda0),
                                    r.data_ptr() if r is not None else None, r.numel() if r is not None else 0, chunk_rows,
                                    mu.data_ptr(), sigma2.data_ptr(), rate.data_ptr() if rate is not None else None,
                                    U.data_ptr() if U is not None else None), "gpfit_score_pool")
    return mu, sigma2, rate, U


@torch.no_grad()
def pool_moments(xstar, xtilde, C, theta, folded, mask=None, chunk_rows=0):
    """Predictive mean and variance of lambda for every row of ``xstar`` in one device call (``gpfit_score_pool``):
    what ``lambda_moments_star`` returns, from the posterior folded by ``fold_posterior``.  ``xstar`` is already masked,
    or holds whole images together with ``mask`` (``xtilde`` may then be unmasked too); the pool is walked in chunks of
    ``chunk_rows`` rows (0: as many as the workspace holds) without any pool-sized temporary.  Beside the device call the
    wrapper allocates the outputs; the first call with a given ``mask`` also forms the pixel list (``torch.nonzero``: one
    host synchronisation) and keeps it in ``folded``.  The bits of a row do not depend on ``chunk_rows``, on the
    workspace's size or on the row's position.  ``sigma2`` is not clamped."""
    mu, sigma2, _, _ = _score_pool_call(xstar, xtilde, C, theta, folded, 1.0, 0.0, None, mask, chunk_rows, False)
    return mu, sigma2


@torch.no_grad()
def score_pool(xstar, xtilde, C, theta, folded, f_params, r_masked=None, mask=None, chunk_rows=0):
    """Moments, firing rate (utils.py:395) and, with the response counts ``r_masked``, the active-learning utility
    (``nd_utility`` at ``A^2 sigma2``, ``A mu + lambda0``: the same kernel, the same bits) of every row of ``xstar`` in
    one device call.  Returns a dict with ``mu``, ``sigma2``, ``rate`` and ``utility`` (None without ``r_masked``)."""
    A = _scalar(torch.exp(torch.as_tensor(f_params['logA'])))
    lambda0 = _scalar(_lambda0_of(f_params))
    mu, sigma2, rate, U = _score_pool_call(xstar, xtilde, C, theta, folded, A, lambda0, r_masked, mask, chunk_rows, True)
    return {"mu": mu, "sigma2": sigma2, "rate": rate, "utility": U}


# ------------------------------------------------------------------ a pool scored for several cells at once
last_pool_group_sizes = []   # units per device call of the last score_pool_cells, in the order the calls were made


def _link_scalars(f_params):
    return _scalar(torch.exp(torch.as_tensor(f_params['logA']))), _scalar(_lambda0_of(f_params))


def _pool_bucket_key(d, nt, k, with_B):
    """Units with equal keys may share one ``gpfit_score_pool_batch`` call: the three padded sizes and the presence of a
    basis (the true sizes may differ)."""
    return (-(-int(d) // 32) * 32, -(-int(nt) // 128) * 128, -(-int(k) // 128) * 128, bool(with_B))


def _pool_cell_key(cell):
    """``_pool_bucket_key`` of a cell as ``score_pool_cells`` is given it (shapes only, nothing is moved)."""
    folded, xtilde = cell["folded"], cell["xtilde"]
    return _pool_bucket_key(cell["C"].shape[0], 1 if xtilde.dim() == 1 else xtilde.shape[0], folded["k"], folded["B"] is not None)


def _score_pool_batch_raw(ctxs, qs, r, chunk_rows, mu, sigma2, rate, U):
    """``gpfit_score_pool_batch`` on the requests ``qs`` (``_score_pool_prepare`` plus ``A``, ``lambda0``) with the contexts
    ``ctxs`` (one per request) and one output vector per request in each of ``mu``, ``sigma2``, ``rate``, ``U`` (``U``
    None without ``r``): the return code, nothing checked here -- ``P`` is that of ``qs[0]``."""
    n = len(qs)
    i64s = lambda vals: (ctypes.c_int64 * n)(*[int(v) for v in vals])      # noqa: E731
    ptrs = lambda ts: (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])   # noqa: E731
    Bs = [q["B"] for q in qs]
    return _lib.load().gpfit_score_pool_batch(
        _ctx_table(ctxs), n, _stream(), _lib.darr([q["sigma0"] for q in qs]), _ptr_table(qs, "xstar"),
        i64s(q["xstar"].stride(0) for q in qs), qs[0]["P"], _ptr_table(qs, "pix"), i64s(q["d_full"] for q in qs),
        _ptr_table(qs, "xtilde"), i64s(q["xtilde"].stride(0) for q in qs), i64s(q["nt"] for q in qs), i64s(q["d"] for q in qs),
        _ptr_table(qs, "C"), i64s(q["C"].stride(0) for q in qs), ptrs(Bs), i64s(0 if B is None else B.stride(0) for B in Bs),
        i64s(q["k"] for q in qs), _ptr_table(qs, "S"), i64s(q["S"].stride(0) for q in qs), _ptr_table(qs, "w"),
        _lib.darr([q["A"] for q in qs]), _lib.darr([q["lambda0"] for q in qs]), None if r is None else r.data_ptr(),
        0 if r is None else r.numel(), chunk_rows, ptrs(mu), ptrs(sigma2), ptrs(rate), None if U is None else ptrs(U))


@torch.no_grad()
def _score_pool_group(units, r_masked, chunk_rows, out=None):
    """``score_pool`` for several independent units (the cells of a population on one pool) as ONE device call
    (``gpfit_score_pool_batch``).  ``units``: one dict per unit with the arguments of ``score_pool`` by name (``xstar``,
    ``xtilde``, ``C``, ``theta``, ``folded``, ``f_params`` and optionally ``mask``; the mask's pixel list is kept in
    ``folded`` as the single call keeps it); 1 .. 16 units with pools of one length and one ``_pool_bucket_key`` --
    otherwise a ValueError before any call.  ``out``: per unit the four float64 device vectors the call writes (``mu``,
    ``sigma2``, ``rate``, ``utility``) in place of new ones.  Returns, per unit, what ``score_pool`` returns for it, bit
    for bit."""
    if not 1 <= len(units) <= MAX_CHAIN_UNITS:
        raise ValueError(f"_score_pool_group: 1 .. {MAX_CHAIN_UNITS} units per call")
    chunk_rows = _pool_chunk_rows(chunk_rows)
    qs = []
    for u in units:
        q = _score_pool_prepare(u["xstar"], u["xtilde"], u["C"], u["theta"], u["folded"], u.get("mask"))
        q["A"], q["lambda0"] = _link_scalars(u["f_params"])
        qs.append(q)
    if len({q["P"] for q in qs}) != 1 or len({_pool_bucket_key(q["d"], q["nt"], q["k"], q["B"] is not None) for q in qs}) != 1:
        raise ValueError("gpfit_score_pool_batch: the units of one call share the pool's length, round_up(d, 32), "
                         "round_up(nt, 128), round_up(k, 128) and the presence of a basis")
    dev, P = _device(), qs[0]["P"]
    r = _cu(r_masked).reshape(-1).contiguous() if r_masked is not None else None
    if out is None:
        block = torch.empty((len(qs), 4 if r is not None else 3, P), dtype=TORCH_DTYPE, device=dev)
        out = [tuple(block[i]) + (() if r is not None else (None,)) for i in range(len(qs))]
    res = [{"mu": o[0], "sigma2": o[1], "rate": o[2], "utility": o[3] if r is not None else None} for o in out]
    if P == 0:
        return res
    engines = _group_engines(len(qs), max(_pool_workspace_rows(q) for q in qs), max(q["d"] for q in qs),
                             max(q["d_full"] for q in qs))
    _lib.check(_score_pool_batch_raw([e._ctx for e in engines], qs, r, chunk_rows, [o["mu"] for o in res],
                                     [o["sigma2"] for o in res], [o["rate"] for o in res],
                                     None if r is None else [o["utility"] for o in res]), "gpfit_score_pool_batch")
    return res


def _score_pool_single(unit, r_masked, chunk_rows, out):
    """One unit of ``score_pool_cells`` through the single call (``gpfit_score_pool``) into the rows ``out``."""
    A, lambda0 = _link_scalars(unit["f_params"])
    _score_pool_call(unit["xstar"], unit["xtilde"], unit["C"], unit["theta"], unit["folded"], A, lambda0, r_masked,
                     unit.get("mask"), chunk_rows, True, out=out)


def _utility_sum(U, weights=None):
    """``gpfit_utility_sum``: the weighted sum of the rows of ``U`` [n_rows][P] (``weights`` None: ones), rows in ascending
    order."""
    U = _cu(U)
    n_rows, P = U.shape
    w = None if weights is None else _cu(weights).reshape(-1).contiguous()
    if w is not None and w.numel() != n_rows:
        raise ValueError("one weight per row")
    out = torch.empty(P, dtype=TORCH_DTYPE, device=U.device)
    _lib.check(_lib.load().gpfit_utility_sum(_stream(), U.data_ptr(), U.stride(0), n_rows, None if w is None else w.data_ptr(),
                                             P, out.data_ptr()), "gpfit_utility_sum")
    return out


@torch.no_grad()
def score_pool_cells(xstar, cells, r_masked=None, weights=None, chunk_rows=0, max_units=MAX_CHAIN_UNITS):
    """``score_pool`` of one pool for any number of cells, and the utility of the population.  ``cells``: one dict per cell
    with ``xtilde``, ``C``, ``theta``, ``folded`` (``fold_posterior``), ``f_params`` and optionally ``mask`` -- the
    arguments of ``score_pool`` by name; ``xstar`` is the pool all of them are scored on (whole images where the cells
    have masks).  The cells are sorted into buckets by ``_pool_bucket_key`` and every bucket goes out in device calls of at
    most ``max_units`` cells (``gpfit_score_pool_batch``); with ``POOL_GROUPS`` off every cell goes through the single
    call.  Either way each cell has the bits of ``score_pool`` on it alone.

    Returns a dict: ``mu``, ``sigma2``, ``rate``, ``utility`` as tensors [n_cells][P] in the caller's order (``utility``
    None without ``r_masked``), ``population_utility`` [P] = sum over the cells of ``weights[c] * utility[c]`` in the
    caller's order (``gpfit_utility_sum``; ``weights`` None: ones; None without ``r_masked``), and ``errors``: per cell None,
    or the exception its call raised -- that cell's rows are NaN (and so is the sum), the other cells are scored.  The units
    per device call are left in ``last_pool_group_sizes``."""
    global last_pool_group_sizes
    if not 1 <= int(max_units) <= MAX_CHAIN_UNITS:
        raise ValueError(f"score_pool_cells: max_units is 1 .. {MAX_CHAIN_UNITS}")
    chunk_rows = _pool_chunk_rows(chunk_rows)
    dev = _device()
    xstar = _cu(xstar)
    xstar = xstar.reshape(-1, xstar.shape[-1])
    n, P = len(cells), xstar.shape[0]
    keys = ("mu", "sigma2", "rate") + (("utility",) if r_masked is not None else ())
    block = torch.empty((len(keys), n, P), dtype=TORCH_DTYPE, device=dev)
    res = {key: block[i] for i, key in enumerate(keys)}
    rows = [tuple(res[key][c] for key in keys) + (() if r_masked is not None else (None,)) for c in range(n)]
    errors, sizes, buckets = [None] * n, [], collections.OrderedDict()
    for c, cell in enumerate(cells):
        try:
            buckets.setdefault(_pool_cell_key(cell), []).append(c)
        except Exception as err:          # a cell that cannot even be sorted: its own error
            errors[c] = err
    step = int(max_units) if POOL_GROUPS else 1
    for members in buckets.values():
        for a in range(0, len(members), step):
            part = members[a:a + step]
            try:
                if POOL_GROUPS:
                    _score_pool_group([dict(cells[c], xstar=xstar) for c in part], r_masked, chunk_rows,
                                      out=[rows[c] for c in part])
                else:
                    _score_pool_single(dict(cells[part[0]], xstar=xstar), r_masked, chunk_rows, rows[part[0]])
                sizes.append(len(part))
            except Exception as err:
                if len(part) == 1:
                    errors[part[0]] = err
                    continue
                for c in part:            # the group was refused for one of its cells: each on its own, to find which
                    try:
                        _score_pool_single(dict(cells[c], xstar=xstar), r_masked, chunk_rows, rows[c])
                        sizes.append(1)
                    except Exception as own:
                        errors[c] = own
    for c, err in enumerate(errors):
        if err is not None:
            block[:, c] = float("nan")
    last_pool_group_sizes = sizes
    res["utility"] = res.get("utility")
    res["population_utility"] = _utility_sum(res["utility"], weights) if r_masked is not None and n > 0 else None
    res["errors"] = errors
    return res


# ------------------------------------------------------------------ a round picked one by one (batch-aware selection)
SELECT_MAX = 128         # GPFIT_SELECT_MAX of the C header
SHORTLIST = 1024         # select_round's default: 8 MiB of covariance per cell, 16 cells in flight


@torch.no_grad()
def pool_covariance(xstar, xtilde, C, theta, folded, mask=None):
    """Posterior covariance of the latents of a shortlist in one device call (``gpfit_pool_covariance``):
    ``Sigma[i][j] = k(x_i, x_j) + z_i S z_j^T`` as a tensor [M, M], symmetric bit for bit, its diagonal the bits of
    ``pool_moments``' ``sigma2`` on the same rows.  The arguments, their checks and the mask handling are those of
    ``pool_moments``; the whole shortlist must fit this thread's workspace as one chunk (it is sized for it: M^2 doubles
    per work matrix)."""
    q = _score_pool_prepare(xstar, xtilde, C, theta, folded, mask)
    xstar, xtilde, C, pix, S, B = (q[key] for key in ("xstar", "xtilde", "C", "pix", "S", "B"))
    M = q["P"]
    Sigma = torch.empty((M, M), dtype=TORCH_DTYPE, device=_device())
    if M == 0:
        return Sigma
    eng = get_engine(max(q["nt"], q["k"], M), q["d"], q["d_full"])
    _lib.check(_lib.load().gpfit_pool_covariance(
        eng._ctx, _stream(), q["sigma0"], xstar.data_ptr(), xstar.stride(0), M, pix.data_ptr() if pix is not None else None,
        q["d_full"], xtilde.data_ptr(), xtilde.stride(0), q["nt"], q["d"], C.data_ptr(), C.stride(0),
        B.data_ptr() if B is not None else None, B.stride(0) if B is not None else 0, q["k"], S.data_ptr(), S.stride(0),
        Sigma.data_ptr(), Sigma.stride(0)), "gpfit_pool_covariance")
    return Sigma


@torch.no_grad()
def select_batch(Sigmas, mus, f_params_list, r_masked, n_select, weights=None):
    """Pick ``n_select`` rows one by one, each conditioned on those already chosen (``gpfit_select_batch``; DESIGN.md
    section 5): per unit (cell) the covariance ``Sigmas[u]`` [M, M] of ``pool_covariance``, the means ``mus[u]`` [M] and
    the link parameters ``f_params_list[u]``; ``weights`` as in ``score_pool_cells`` (None: ones).  1 .. 16 units,
    ``n_select`` in 1 .. 128.  Everything stays on the device and nothing is synchronised: returns a dict with ``picked``
    (int64 [n_select], row indices in pick order, -1 from the step on at which no row with a finite utility is left),
    ``utility`` ([n_select], the population utility of each pick when it was picked, NaN beside a -1) and ``sigma2`` (per
    unit the conditional variances [M] given all picks)."""
    n, n_select = len(Sigmas), int(n_select)
    if not 1 <= n <= MAX_CHAIN_UNITS or len(mus) != n or len(f_params_list) != n:
        raise ValueError(f"select_batch: 1 .. {MAX_CHAIN_UNITS} units, with one mean vector and one link each")
    if not 1 <= n_select <= SELECT_MAX:
        raise ValueError(f"select_batch: n_select is 1 .. {SELECT_MAX}")
    dev = _device()
    Sigmas = [_cu(S) for S in Sigmas]
    mus = [_cu(m).reshape(-1).contiguous() for m in mus]
    M = mus[0].numel()
    if M < 1 or any(tuple(S.shape) != (M, M) or S.stride(1) != 1 for S in Sigmas) or any(m.numel() != M for m in mus):
        raise ValueError("select_batch: every unit needs a covariance [M, M] and a mean [M] of one M >= 1")
    r = _cu(r_masked).reshape(-1).contiguous()
    w = None if weights is None else [float(v) for v in torch.as_tensor(weights).reshape(-1).tolist()]
    if w is not None and len(w) != n:
        raise ValueError("one weight per unit")
    links = [_link_scalars(fp) for fp in f_params_list]
    work = torch.empty((n, n_select, M), dtype=TORCH_DTYPE, device=dev)
    s2 = torch.empty((n, M), dtype=TORCH_DTYPE, device=dev)
    picked = torch.empty(n_select, dtype=torch.int32, device=dev)
    utility = torch.empty(n_select, dtype=TORCH_DTYPE, device=dev)
    ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])   # noqa: E731
    _lib.check(_lib.load().gpfit_select_batch(
        _stream(), n, ptrs(Sigmas), (ctypes.c_int64 * n)(*[S.stride(0) for S in Sigmas]), M, ptrs(mus),
        _lib.darr([a for a, _ in links]), _lib.darr([l0 for _, l0 in links]), None if w is None else _lib.darr(w), r.data_ptr(),
        r.numel(), n_select, ptrs(list(work)), ptrs(list(s2)), picked.data_ptr(), utility.data_ptr()), "gpfit_select_batch")
    return {"picked": picked.to(torch.int64), "utility": utility, "sigma2": list(s2)}


@torch.no_grad()
def select_round(xstar, cells, n_select, r_masked, weights=None, shortlist=SHORTLIST, chunk_rows=0):
    """The images of one round of the closed loop, picked one by one, each conditioned on those already chosen.
    ``xstar``, ``cells``, ``weights`` and ``chunk_rows`` are those of ``score_pool_cells`` (``cells`` may hold one cell):
      1. the whole pool is scored with ``score_pool_cells``, unchanged;
      2. the ``min(P, shortlist)`` rows of largest population utility are kept, sorted by pool index, so that among equal
         utilities the image that comes first in the pool wins;
      3. ``pool_covariance`` of the shortlist, cell after cell, then one ``select_batch`` for all cells.
    An image outside the shortlist can never be picked: only the shortlist's covariance is formed, M^2 doubles per cell,
    and that is what the shortlist is for.  The default of 1024 keeps it at 8 MiB per cell, 128 MiB with the 16 cells of
    one call in flight, and is eight times the longest round; a shortlist above the workspace's ``POOL_ROWS`` is
    refused.  ``shortlist >= P`` means the whole pool.

    Returns a dict: ``picked`` (int64 device [n_select], POOL indices in pick order, -1 once nothing is left), ``utility``
    ([n_select]), ``shortlist`` (the pool indices kept) and ``scores`` (what ``score_pool_cells`` returned).  The one
    host synchronisation is the sort of the shortlist's indices inside torch."""
    shortlist, n_select = int(shortlist), int(n_select)
    if not 1 <= shortlist <= POOL_ROWS:
        raise ValueError(f"select_round: shortlist is 1 .. {POOL_ROWS} (the rows the pool workspace is sized for)")
    if not 1 <= len(cells) <= MAX_CHAIN_UNITS:
        raise ValueError(f"select_round: 1 .. {MAX_CHAIN_UNITS} cells")
    if not 1 <= n_select <= SELECT_MAX:
        raise ValueError(f"select_round: n_select is 1 .. {SELECT_MAX}")
    xstar = _cu(xstar)
    xstar = xstar.reshape(-1, xstar.shape[-1])
    scores = score_pool_cells(xstar, cells, r_masked=r_masked, weights=weights, chunk_rows=chunk_rows)
    for err in scores["errors"]:
        if err is not None:
            raise err
    P = xstar.shape[0]
    if P == 0:
        raise ValueError("select_round: the pool is empty")
    total = scores["population_utility"]
    if shortlist >= P:
        keep = torch.arange(P, device=total.device)
    else:
        # NaN sorts as the largest value in torch.topk: such rows would only waste the shortlist
        keep = torch.sort(torch.topk(torch.nan_to_num(total, nan=-float("inf")), shortlist).indices).values
    rows = xstar[keep].contiguous()
    Sigmas = [pool_covariance(rows, c["xtilde"], c["C"], c["theta"], c["folded"], c.get("mask")) for c in cells]
    out = select_batch(Sigmas, [scores["mu"][u][keep] for u in range(len(cells))], [c["f_params"] for c in cells], r_masked,
                       n_select, weights)
    local = out["picked"]
    picked = torch.where(local >= 0, keep[local.clamp_min(0)], local)
    return {"picked": picked, "utility": out["utility"], "shortlist": keep, "scores": scores}


# ------------------------------------------------------------------ initialisation (utils.py:705-857)
def generate_xtilde(ntilde, x):
    """Jittered random subset of the first ``ntilde`` stimuli (utils.py:705-711)."""
    x = _cu(x)
    idx = torch.randperm(ntilde, device=x.device)
    first = x[idx, :]
    return first + torch.finfo(TORCH_DTYPE).eps * 10 * torch.randn(first.shape, dtype=TORCH_DTYPE, device=x.device)


def logbetaexpr_to_beta(logbetaexpr):
    return torch.exp(-0.5 * torch.as_tensor(logbetaexpr)) * torch.tensor(0.5)


def logrhoexpr_to_rho(logrhoexpr):
    return torch.exp(-0.5 * torch.as_tensor(logrhoexpr)) / torch.sqrt(torch.tensor(2.0))


def fromlogbetasam_to_logbetaexpr(logbetasam):
    return logbetasam - torch.log(torch.tensor(2.0))


def fromlogrhosam_to_logrhoexpr(logrhosam):
    return logrhosam - torch.log(torch.tensor(2.0))


def get_sta(x, r, n_px_side):
    """Spike-triggered average, its (hand-set) variance and the pixel of its peak (utils.py:736-753)."""
    x, r = _cu(x), _cu(r)
    n = r.shape[0]
    img_mean = matmul(x, torch.ones_like(r), transA=True) / n
    sta = matmul(x, r, transA=True) / n - img_mean
    rows, cols = _grid(n_px_side)
    peak = int(torch.argmax(torch.abs(sta)))
    return sta, torch.tensor(10), (torch.tensor(peak // cols), torch.tensor(peak % cols))


def generate_theta(x, r, n_px_side, display_hyper=False, **kwargs):
    """Initial hyperparameters and their boxes (utils.py:755-857).  As in the reference the
    receptive-field centre starts at (0, 0), the width is the hand-set 10 px^2, and caller
    overrides in ``kwargs`` are applied only when ``display_hyper`` is true (utils.py:829-834)."""
    up_lim, low_lim = 1, -1
    rows, _ = _grid(n_px_side)
    sigma_0 = torch.tensor(1.0, dtype=TORCH_DTYPE, requires_grad=True)
    Amp = torch.tensor(1.0, dtype=TORCH_DTYPE, requires_grad=True)
    get_sta(x, r, n_px_side)  # evaluated for parity of side effects; its peak is not used (utils.py:785-797)
    eps_0x = torch.tensor(0.0, dtype=TORCH_DTYPE, requires_grad=True)
    eps_0y = torch.tensor(0.0, dtype=TORCH_DTYPE, requires_grad=True)
    beta = (torch.sqrt(torch.tensor(10.0, dtype=TORCH_DTYPE)) / rows) * (up_lim - low_lim)
    logbetaexpr = (-2 * safe_log(2 * beta)).requires_grad_(True)
    rho = beta / 2
    logrhoexpr = (-safe_log(torch.tensor(2.0, dtype=TORCH_DTYPE) * (rho * rho))).requires_grad_(True)
    theta = {'sigma_0': sigma_0, 'eps_0x': eps_0x, 'eps_0y': eps_0y, '-2log2beta': logbetaexpr,
             '-log2rho2': logrhoexpr, 'Amp': Amp}
    if display_hyper:
        for key, value in kwargs.items():
            if key in theta:
                theta[key] = value
                print(f'updated {key} to {_scalar(value):.4f}')
        print(f' Dict of learnable hyperparameters : {", ".join(f"{k} = {_scalar(v):.4f}" for k, v in theta.items())}')
        print(f' Hyperparameters from the logexpr  : beta = {float(logbetaexpr_to_beta(logbetaexpr)):.4f}, '
              f'rho = {float(logrhoexpr_to_rho(logrhoexpr)):.4f}')
    inf = float('inf')
    lower = {'sigma_0': 0, 'eps_0x': low_lim, 'eps_0y': low_lim, '-2log2beta': -inf, '-log2rho2': -inf, 'Amp': 0.}
    upper = {'sigma_0': inf, 'eps_0x': up_lim, 'eps_0y': up_lim, '-2log2beta': inf, '-log2rho2': inf, 'Amp': inf}
    return (theta, lower, upper)


def print_hyp(theta):
    for key in theta.keys():
        extra = ''
        if key == '-2log2beta':
            extra = f' --> beta: {float(logbetaexpr_to_beta(theta[key])):8.4f}'
        if key == '-log2rho2':
            extra = f' --> rho : {float(logrhoexpr_to_rho(theta[key])):8.4f}'
        print(f' {key:<12}: {_scalar(theta[key]):>8.4f}{extra}')


# ------------------------------------------------------------------ active-learning utility (utils.py:413-525)
@torch.no_grad()
def nd_utility(sigma2, mu, r_masked):
    """Utility U = H(r|x,D) - <H(r|f,x)> of each candidate stimulus (reference utils.py:498-525
    with nd_p_r_given_xD / nd_lambda_r_mean / nd_mean_noise_entropy, 413-496).  ``sigma2`` and ``mu``
    are the variance and mean of log f for the candidates (0-d or [nstar]); ``r_masked`` the response
    counts of the truncated sum (the notebooks pass ``arange(0, 100)``).  One fused device kernel,
    Lambert W included (the reference goes through scipy on the host, utils.py:464-466)."""
    lib = _lib.load()
    s2, m = _cu(sigma2), _cu(mu)
    if s2.ndim == 0:                                     # utils.py:509-511
        s2, m = s2[None], m[None]
    s2, m = s2.reshape(-1).contiguous(), m.reshape(-1).contiguous()
    if s2.numel() != m.numel():
        raise ValueError("nd_utility: sigma2 and mu must have the same number of entries")
    r = _cu(r_masked).reshape(-1).contiguous()
    U = torch.empty_like(s2)
    _lib.check(lib.gpfit_nd_utility(_stream(), s2.data_ptr(), m.data_ptr(), s2.numel(), r.data_ptr(), r.numel(),
                                    U.data_ptr()), "gpfit_nd_utility")
    return U


# ------------------------------------------------------------------ metric (utils.py:1502-1541)
def explained_variance(rtst, f_pred, sigma=True):
    """Reliability-normalised r^2 between predicted rates and repeated test responses
    (rtst[repetitions, images], utils.py:1502-1541); with ``sigma`` the mean and spread over 1000
    random even/odd splits of the repetitions.  Reporting only (torch RNG, excluded from parity,
    SURVEY 8c G5).  The reference draws and evaluates the 1000 splits one at a time (a few
    thousand tiny kernels on a device: 0.4 s); here they are drawn and evaluated as one batch."""
    rtst, f_pred = _cu(rtst), _cu(f_pred)

    def corr(a, b):                       # Pearson correlation along the last axis (torch.corrcoef)
        a = a - a.mean(-1, keepdim=True)
        b = b - b.mean(-1, keepdim=True)
        return (a * b).sum(-1) / torch.sqrt((a * a).sum(-1) * (b * b).sum(-1))

    def r2_of(reven, rodd):
        rel = torch.abs(corr(reven, rodd))
        return 0.5 * (corr(f_pred, rodd) + corr(f_pred, reven)) / rel

    if not sigma:
        return r2_of(torch.mean(rtst[0::2, :], 0), torch.mean(rtst[1::2, :], 0)), None
    nboot, n = 1000, rtst.shape[0]
    perm = torch.argsort(torch.rand(nboot, n, device=rtst.device), dim=1)      # nboot random permutations
    reven = rtst[perm[:, 0::2]].mean(1)                                         # [nboot, images]
    rodd = rtst[perm[:, 1::2]].mean(1)
    vals = r2_of(reven, rodd)
    return torch.mean(vals), torch.std(vals)


# ------------------------------------------------------------------ fit (utils.py:1568-2316)
def _eigen_stabilise(K_tilde):
    """Spectral truncation of the reference (utils.py:1682-1683): eigh, keep
    lambda > max(lambda_max * EIGVAL_TOL, EIGVAL_TOL).  torch.linalg.eigh is host plumbing here
    (rank decision + basis), not part of the timed path."""
    eigvals, eigvecs = torch.linalg.eigh(K_tilde, UPLO='L')
    ikeep = eigvals > max(float(eigvals.max()) * EIGVAL_TOL, EIGVAL_TOL)
    return eigvals, eigvecs, ikeep


def _mark_identity(B):
    B._gpfit_identity = True       # fast-path hint only: products with B are skipped where it is seen
    return B


def _is_identity(B):
    return bool(getattr(B, '_gpfit_identity', False))


def _all_eigenvalues_kept(K_tilde):
    """Rank decision without an eigendecomposition, for the regime the reference's
    truncation rule (utils.py:1683, 1809) keeps EVERY eigenvalue: lambda_min > max(lambda_max tol, tol).

    From the Cholesky factorisation the fit needs anyway (K~ = L L^T, L^-1 by the MFMA recursion):
        lambda_max <= min(trace K~, ||K~||_inf)                 (SPD; Gershgorin)
        lambda_min  = 1 / ||L^-T L^-1||_2 >= 1 / (||L^-1||_1 ||L^-1||_inf)
    Both bounds are rigorous, so ``True`` is a proof that nothing would be truncated; when they are
    inconclusive (or K~ is not numerically positive definite) the caller falls back to
    ``torch.linalg.eigh``.  Returns ``(decided_all_kept, L, Linv)``."""
    L, Li, logdet, info = cholesky(K_tilde, want_inverse=True)
    if info != 0:
        return False, None, None
    _BASIS.factor_logdet = logdet      # log|K~| of the factor returned here (per host thread; varGP hands it to the loss)
    return _all_kept_given_factor(K_tilde, Li), L, Li


def _all_kept_given_factor(K_tilde, Li):
    """The two rigorous bounds of ``_all_eigenvalues_kept`` for a K~ whose inverse factor ``Li`` is already known
    (the closed loop extends the factor by one row per added image, ``cholesky_append``)."""
    lam_max_ub = min(float(torch.diagonal(K_tilde).sum()), float(K_tilde.abs().sum(1).max()))
    ali = Li.abs()
    lam_min_lb = 1.0 / (float(ali.sum(0).max()) * float(ali.sum(1).max()))
    del ali
    if not (math.isfinite(lam_max_ub) and math.isfinite(lam_min_lb)):
        return False
    return lam_min_lb > max(lam_max_ub * EIGVAL_TOL, EIGVAL_TOL)


def _stabilised_basis(K_tilde, route=None, start=None):
    """Basis the reference works in after its eigen-stabilisation (utils.py:1682-1694): returns
    ``(eigvecs, B, K_tilde_b, K_tilde_inv_b)``.

    When every eigenvalue is provably kept (``_all_eigenvalues_kept``) B is square orthogonal and
    everything the reference computes downstream is basis-invariant, so the
    identity is used: ``B = I``, ``K_tilde_b = K~``, ``K_tilde_inv_b = L^-T L^-1`` -- no ``eigh``
    (0.67 s at N = 8192, five of them in a four-iteration fit).  When eigenvalues are truncated and
    N >= 256, the kept eigenspace comes from ``eigtop`` (block subspace iteration from N = 1792, the spectral projector of K~
    itself below) and the
    first return value holds only those columns; otherwise, and whenever that solver declines, the
    reference's own eigendecomposition + truncation.  A COLD call (no ``start``) is a deterministic function of K~
    alone on every route, so ``test(at_iteration=...)`` rebuilds a basis of the space the tracked ``(m_b, V_b)`` were
    expressed in; a WARM call (``start`` given) agrees with the cold one to the certificate, not to the bit: the same
    count (lambda_max, so the threshold, is certified to 1e-8 relative on both, or the route declines) and the same
    stopping criterion of the sweeps (angle bound 1e-7), so nearly the same kept space and canonical basis -- the
    warm-start tests hold the two bases within 1e-5 of each other, entry by entry.

    The route taken (``'identity'``, ``'subspace'``, ``'eigtop'`` or ``'eigh'``) is left in ``_BASIS.route`` (per host thread);
    ``varGP`` records it with every tracked iteration.  ``route=...`` asks for exactly that route -- what
    ``test(at_iteration=...)`` does with the recorded one, so that a model fitted under one setting
    (``GPFIT_FORCE_EIGH``, another library version) is never evaluated in a different basis: a route that
    cannot be reproduced raises instead of returning numbers in the wrong coordinates.

    ``start``: the solver state a previous call left in ``_BASIS.state`` for a NEARBY kernel matrix (``varGP`` hands the
    state of one EM iteration to the next: theta has moved a little, the kept eigenspace with it): the subspace solver
    then starts from that block and plans only the sweeps the measured distance needs.  Same stopping criterion; a call
    without it is a function of K~ alone (what ``test(at_iteration=...)`` relies on)."""
    n = K_tilde.shape[0]
    _BASIS.state = None

    def truncated_basis(want=None):
        # truncated regime: only the kept eigenspace, by block subspace iteration on the library's GEMM and Cholesky
        # (eigtop.py; 40 ms against 670 ms for the full eigh at N = 8192).  want = "subspace": the canonical
        # orthonormal basis of that space and the dense K~_b = B^T K~ B, no dense eigendecomposition at all;
        # "eigtop": its eigenvectors (one k x k eigh, k = 1024), same eigenvalues to 1e-14 and the same invariant
        # subspace to 1e-13 as the full eigh.  None: inconclusive -> the reference's own eigh.
        want = want or ("subspace" if EIGTOP_BASIS == "subspace" else "eigtop")
        if want == "subspace" and _DENSE_MIN_N <= n < _EIGTOP_MIN_N:
            # small matrices: the spectral projector of K~ itself (Cayley transform + scaled sign iteration on the
            # n x n matrix, no sweeps): 2.6 / 3.8 / 5.6 / 7.7 ms at n = 512 / 1024 / 1280 / 1536 against 12 / 22 / 29 /
            # 35 ms for rocSOLVER's eigh; the same canonical basis as the sweeps route gives for that space
            top = eigtop.kept_eigenspace_dense(K_tilde, EIGVAL_TOL, matmul, cholesky, gemm_into=gemm_into,
                                               sign_chain=_sign_steps if (SIGN_CHAIN or BASIS_GROUPS) else None)
            if top is None:
                return None
            if top[1] is None:
                return "all-kept", None      # the projector is the identity: an exact all-kept proof (identity route)
            return "subspace", (top[1], top[1], top[2]["K_tilde_b"], top[2]["K_tilde_inv_b"])
        if n < _EIGTOP_MIN_N:
            return None
        top = eigtop.top_eigenpairs(K_tilde, EIGVAL_TOL, matmul, cholesky,
                                    basis="subspace" if want == "subspace" else "eigenvectors", gemm_into=gemm_into,
                                    start=start if want == "subspace" else None,
                                    sweep_chain=_basis_sweeps if SWEEP_CHAIN else None,
                                    sign_chain=_sign_steps if (SIGN_CHAIN or BASIS_GROUPS) else None)
        if top is None:
            return None
        vals, vecs, info = top
        if vals is None:
            _BASIS.state = info.get("state")
            return "subspace", (vecs, vecs, info["K_tilde_b"], info["K_tilde_inv_b"])
        # the first entry stands in for the reference's N x N eigenvector matrix: only the kept columns exist
        return "eigtop", (vecs, vecs, torch.diag(vals), torch.diag_embed(1 / vals))

    def identity_basis(Li):
        B = _mark_identity(torch.eye(n, dtype=TORCH_DTYPE, device=K_tilde.device))
        Kinv = matmul(Li, Li, transA=True)
        return None, B, K_tilde, (Kinv + Kinv.T) * 0.5

    def eigh_basis():
        eigvals, eigvecs, ikeep = _eigen_stabilise(K_tilde)
        kept = eigvals[ikeep]
        return eigvecs, eigvecs[:, ikeep].contiguous(), torch.diag(kept), torch.diag_embed(1 / kept)

    if route is not None:
        if route == "identity":
            kept, L, Li = _all_eigenvalues_kept(K_tilde)
            if not kept and L is not None:
                got = truncated_basis("subspace")     # small matrices: the exact count where the norm bounds are not enough
                kept = got is not None and got[0] == "all-kept"
            out = identity_basis(Li) if kept else None
            if kept:
                _BASIS.factor = (L, Li)
        elif route in ("eigtop", "subspace"):
            got = truncated_basis(route)
            out = got[1] if (got is not None and got[0] == route) else None
        elif route == "eigh":
            out = eigh_basis()
        else:
            raise ValueError(f"unknown basis route {route!r}")
        if out is None:
            raise _lib.GpfitError(f"the basis route {route!r} recorded with this model cannot be reproduced for this "
                                  "kernel matrix (EIGVAL_TOL or the library changed since the fit)")
        _BASIS.route = route
        return out
    if not _FORCE_EIGH:
        # The two checks agree on every K~ (a proof that all eigenvalues are kept excludes a truncated count and
        # vice versa), so their order only decides what is paid: a kernel matrix of this size that was truncated
        # last time ON THIS THREAD (the same fit, one EM iteration later) goes to the subspace solver first and
        # skips the Cholesky + inverse + norms of the all-kept proof (~25 ms at N = 8192).
        hints = _BASIS.__dict__.setdefault("regime", {})
        key = (n, float(EIGVAL_TOL))
        exact_all = False        # the small-matrix projector found every eigenvalue above the threshold
        if hints.get(key) == "truncated":
            got = truncated_basis()
            if got is not None and got[0] != "all-kept":
                _BASIS.route = got[0]
                return got[1]
            exact_all = got is not None
        kept, L, Li = _all_eigenvalues_kept(K_tilde)
        if not kept and not exact_all and hints.get(key) != "truncated":
            got = truncated_basis()
            if got is not None and got[0] != "all-kept":
                hints[key] = "truncated"
                _BASIS.route = got[0]
                return got[1]
            exact_all = got is not None
        if (kept or exact_all) and L is not None:
            # proved by the norm bounds of _all_eigenvalues_kept or, where those are inconclusive on a small matrix
            # (BASELINE configs[0]: lambda_min within 2 % of the threshold), by the exact count of the spectral projector
            hints[key] = "full"
            _BASIS.route = "identity"
            _BASIS.factor = (L, Li)      # K~ = L L^T, L^-1: kept by varGP for the closed loop (extend_inducing_set)
            return identity_basis(Li)
    _BASIS.route = "eigh"
    return eigh_basis()


import os as _os_mod
_FORCE_EIGH = bool(_os_mod.environ.get("GPFIT_FORCE_EIGH"))   # tuning / A-B knob: always take the eigh route
_EIGTOP_MIN_N = 1792   # from here up the kept eigenspace comes from block subspace sweeps (warm-started: 10.4 ms at N = 1792,
                       # 10.8 at 2048, 11.7 at 2560); below, down to _DENSE_MIN_N, from the spectral projector of K~ itself
                       # (no sweeps: 9.6 ms at N = 1792, 11.4 at 2048, 22 at 2560) -- profiles/r04_small_n_basis.log.  The
                       # kept count is 530-580 whatever N is, so below ~1800 a block iteration has nothing to discard.
_DENSE_MIN_N = 256     # below this the reference's own eigh (a few ms)
# What the truncated regime's basis B is made of at N >= 256 (module global read at call time, like EIGVAL_TOL):
#   "subspace"     (default) the canonical orthonormal basis of the kept EIGENSPACE: no dense eigendecomposition at
#                  all; K_tilde_b = B^T K~ B is a dense n x n matrix.  Everything downstream is invariant under the
#                  choice of an orthonormal basis of that space (the reference's own formulas only use B^T B = I and the
#                  invariance of span B), but the COLUMNS of B are not eigenvectors;
#   "eigenvectors" the reference's own choice (utils.py:1683-1694): the kept eigenvectors, K_tilde_b diagonal, at the
#                  price of one k x k eigendecomposition (k = 1024) per basis: 16 ms more per EM iteration.
EIGTOP_BASIS = _os_mod.environ.get("GPFIT_EIGTOP_BASIS", "subspace")
# The nEstep updates of an EM iteration as one device call (_estep_chain in the truncated / sparse regimes,
# _estep_chain_full in the full-rank regime with the identity basis) instead of two calls and two waits per update (module global read at call time; GPFIT_ESTEP_CHAIN=0 turns it off).  A = exp(logA)
# is then the device's exp, not the host's: a fit may differ from the loop's by rounding.
ESTEP_CHAIN = _os_mod.environ.get("GPFIT_ESTEP_CHAIN", "1") != "0"
# The nEstep DAMPED updates of an EM iteration (fit_parameters['estep_alpha'] != 1) as one device call
# (_estep_chain_damped) instead of the host loop around _estep_projected_damped.  Opt-in (module global read at call
# time; GPFIT_DAMPED_CHAIN=1 turns it on, fit_parameters['estep_damped_chain'] overrides it for one fit): off, nothing in a
# fit changes.  On, A = exp(logA) is the device's exp and the moments come from the chain's own kernels, so a fit may
# differ from the loop's by rounding.
DAMPED_CHAIN = _os_mod.environ.get("GPFIT_DAMPED_CHAIN", "0") not in ("", "0")
# The sweeps of a pass of the subspace iteration as one device call (_basis_sweeps) instead of one wait per sweep (module
# global read at call time; GPFIT_SWEEP_CHAIN=0 turns it off).  The call has the bits of the loop, so the switch changes
# no number of a fit.
SWEEP_CHAIN = _os_mod.environ.get("GPFIT_SWEEP_CHAIN", "1") != "0"
# The projector step of a basis rebuild (eigtop._kept_subspace: the Cayley transform and the sign iteration up to each of
# its convergence tests) as one device call per stretch (_sign_steps) instead of two launches and a clone per step from
# the host (module global read at call time; GPFIT_SIGN_CHAIN=1 turns it on).  The call has the bits of the loop, so the
# switch changes no number of a fit.  Off by default: the loop's launches already keep the device busy, and alone the call
# measures level with it, a few hundredths of a millisecond above at some sizes (profiles/r24_sign_chain.txt); what pays
# is the group call (BASIS_GROUPS), which takes this route whatever the switch says.
SIGN_CHAIN = _os_mod.environ.get("GPFIT_SIGN_CHAIN", "0") not in ("", "0")
# Under varGP_cells the two halves of a basis rebuild -- the sweeps (_basis_sweeps) and the sign stretches (_sign_steps)
# -- meet at the wave's rendezvous and go out as group calls, one per kind and bucket.  Opt-in (module global read at
# call time; GPFIT_BASIS_GROUPS=1 turns it on): off, a wave issues exactly the calls it issues without it.  On or off,
# each cell's numbers are those of varGP on its own.
BASIS_GROUPS = _os_mod.environ.get("GPFIT_BASIS_GROUPS", "0") not in ("", "0")
# Under varGP_cells the chains (_estep_chain_full) and the M-step closures of fits in the full-rank regime meet at the
# wave's rendezvous and go out as group calls (module global read at call time; GPFIT_FULL_RANK_GROUPS=0 turns it off: such
# a fit then issues its own calls and keeps its turn until it ends).
FULL_RANK_GROUPS = _os_mod.environ.get("GPFIT_FULL_RANK_GROUPS", "1") != "0"
# The tracked loss of an EM iteration (compute_loglikelihood + compute_KL_div) as one device call (elbo_terms:
# gpfit_elbo, under varGP_cells one gpfit_elbo_batch call per wave) instead of two factorisations, the product
# V K~^-1 and half a dozen read-backs (module global read at call time; GPFIT_FUSED_LOSS=0 turns it off).  The loss is
# reported and never fed back: the switch changes no m_b, V_b, theta or rate parameter of a fit, only the last digits
# of the tracked loss.
FUSED_LOSS = _os_mod.environ.get("GPFIT_FUSED_LOSS", "1") != "0"
# score_pool_cells scores the cells of a bucket in group calls (gpfit_score_pool_batch); GPFIT_POOL_GROUPS=0: every cell
# through the single call, with the same bits.
POOL_GROUPS = _os_mod.environ.get("GPFIT_POOL_GROUPS", "1") != "0"
# per host thread (the reference's active-learning notebook fits and scores on two threads): the route the last
# call of _stabilised_basis took, and (N, EIGVAL_TOL) -> "full" | "truncated", which of the two rank checks to try
# first -- a hint only, so one thread's history never changes what another thread's fit costs
_BASIS = threading.local()


def _closure_general(theta, lims, n_px_side, x, xtilde, r, B, m_b, V_b, f_params, ntilde, nt):
    """The M-step closure body in the reference's own B-projected formulation
    (utils.py:2030-2099) on the GPU primitives: used when eigenvalues were truncated
    (n < n_tilde) or n_tilde != n_t, where the original-basis fast path does not apply."""
    lower, upper = lims
    C, mask, dC = localker(theta=theta, theta_higher_lims=upper, theta_lower_lims=lower, n_px_side=n_px_side, grad=True)
    xt_m = xtilde[:, mask].contiguous()
    K_tilde, dK_tilde = acosker(theta, xt_m, xt_m, C=C, dC=dC, diag=False)
    if ntilde != nt:
        x_m = x[:, mask].contiguous()
        K, dK = acosker(theta, x_m, xt_m, C=C, dC=dC, diag=False)
    else:
        x_m = xt_m if x is xtilde else x[:, mask].contiguous()
        K, dK = K_tilde, dK_tilde
    Kvec, dKvec = acosker(theta, x_m, x2=None, C=C, dC=dC, diag=True)
    K_tilde_b = matmul(B, matmul(K_tilde, B), transA=True)                         # :2047
    K_tilde_b = (K_tilde_b + K_tilde_b.T) * 0.5                                    # :2048
    K_b = matmul(K, B)                                                             # :2049
    dK_tilde_b = {k: matmul(B, matmul(dK_tilde[k], B), transA=True) for k in dK_tilde}   # :2061
    dK_b = {k: matmul(dK[k], B) for k in dK}                                       # :2062
    K_tilde_inv_b = spd_inverse(K_tilde_b)                                         # :2067 (Cholesky instead of LU)
    KKtilde_inv_b = matmul(K_b, K_tilde_inv_b) if ntilde != nt else B              # :2068
    f_mean, lambda_m, lambda_var, dlm, dlv = mean_f(
        f_params=f_params, calculate_moments=True, x=x_m, K_tilde=K_tilde_b, KKtilde_inv=KKtilde_inv_b, Kvec=Kvec,
        K=K_b, C=C, m=m_b, V=V_b, theta=theta, kernfun=acosker, dK=dK_b, dK_tilde=dK_tilde_b, dK_vec=dKvec,
        K_tilde_inv=K_tilde_inv_b)                                                 # :2070
    loglik, dloglik = compute_loglikelihood(r, f_mean, lambda_m, lambda_var, f_params, dlambda_m=dlm, dlambda_var=dlv)
    KL, dKL = compute_KL_div(m_b, V_b, K_tilde_b, K_tilde_inv=K_tilde_inv_b, dK_tilde=dK_tilde_b)
    grad = {k: -(_scalar(dloglik[k]) - _scalar(dKL[k])) for k in theta.keys()}      # :2097-2099
    return -(_scalar(loglik) - _scalar(KL)), grad                                  # :2087-2089


def _closure_projected(theta, lims, n_px_side, x, r, B, m_b, V_b, f_params):
    """Truncated-rank M-step closure (utils.py:2030-2099 with n < n_tilde = n_t): ONE call of the fused
    entry point ``gpfit_fit_eval_projected`` (kernel build, projection, the two n x n Cholesky
    factorisations, moments / likelihood / KL, adjoints, lift and pull-back on the device).  When a
    factorisation meets a non-positive pivot the reference's ``log_det`` would take its
    eigen-fallback (utils.py:1279-1304): the step-by-step formulation below (``_closure_projected_steps``)
    reproduces that and is used instead.  In a fit of ``varGP_cells`` the device call is the wave's: the request goes
    to the rendezvous and comes back as one unit of a ``gpfit_fit_eval_projected_batch`` call, with the same bits."""
    q = _closure_projected_prepare(theta, lims, n_px_side, x, r, B, m_b, V_b, f_params)
    return _closure_finish(q, *_submit(q), _closure_projected_steps)


def _closure_prepare(theta, lims, n_px_side, x, r, B, m_b, V_b, f_params, xtilde=None, engine=None):
    """The arguments of ``_closure_sparse`` (``xtilde`` given) or ``_closure_projected`` (no ``xtilde``) as one request: the
    operands on the device, the scalars as floats, and the workspace and stream the call runs on -- this thread's
    unless an engine is given.  A sparse request has ``xt`` / ``Nt`` and no ``regime`` field; a truncated one has ``regime``
    and ``cap``, the padded number of stimuli the workspace was created for, on which the k slabs of the projections and
    the route of the lift depend.  ``args``: what the kind's step-by-step function takes."""
    lower, upper = lims
    sparse = xtilde is not None
    xc, xtc, rc, Bc, mc, Vc = _cu(x), _cu(xtilde) if sparse else None, _cu(r), _cu(B), _cu(m_b), _cu(V_b)
    rows, cols = _grid(n_px_side)
    q = {"kind": "closure", "theta": [float(v) for v in theta_vec(theta)],
         "lower": [_scalar(lower[k]) for k in THETA_KEYS], "upper": [_scalar(upper[k]) for k in THETA_KEYS],
         "rows": rows, "cols": cols, "x": xc, "r": rc, "B": Bc, "m_b": mc, "V_b": Vc, "n_kept": int(Bc.shape[1]),
         "logA": _scalar(f_params['logA']), "lambda0": _scalar(_lambda0_of(f_params))}
    if sparse:
        q.update(xt=xtc, N=int(xc.shape[0]), Nt=int(xtc.shape[0]),
                 args=(theta, lims, n_px_side, x, xtilde, r, B, m_b, V_b, f_params))
        n_max = max(q["N"], q["Nt"])
    else:
        q.update(regime="truncated", N=int(Bc.shape[0]), args=(theta, lims, n_px_side, x, r, B, m_b, V_b, f_params))
        n_max = q["N"]
    _request_place(q, engine, n_max, xc.shape[1], rows * cols)
    if not sparse:
        q["cap"] = -(-q["engine"].n_max // 128) * 128
    return q


def _closure_run_single(q):
    """``gpfit_fit_eval_sparse`` on one sparse request, ``gpfit_fit_eval_projected`` (the same argument list without
    xtilde) on one truncated request: ``(rc, out[16])``."""
    out = (ctypes.c_double * 16)()
    x, B, V = q["x"], q["B"], q["V_b"]
    name = "gpfit_fit_eval_sparse" if "xt" in q else "gpfit_fit_eval_projected"
    xt = (q["xt"].data_ptr(), q["xt"].stride(0), q["Nt"]) if "xt" in q else ()
    rc_ = getattr(_lib.load(), name)(q["engine"]._ctx, q["stream"], _lib.darr(q["theta"]), _lib.darr(q["lower"]),
                                     _lib.darr(q["upper"]), q["rows"], q["cols"], x.data_ptr(), x.stride(0), q["N"], *xt,
                                     q["r"].data_ptr(), B.data_ptr(), B.stride(0), q["n_kept"], q["m_b"].data_ptr(),
                                     V.data_ptr(), V.stride(0), q["logA"], q["lambda0"], out)
    if rc_ < 0 and rc_ != -2:
        _lib.check(rc_, name)
    return rc_, list(out)


def _closure_sparse_bucket_key(q):
    """Sparse requests with equal keys may share one ``gpfit_fit_eval_sparse_batch`` call: what that call shares between
    its units, and the padded basis size (the recursion's split, hence the bits, depend on it)."""
    return (q["x"].device.index, q["stream"].value, q["N"], q["Nt"], q["x"].stride(0), q["xt"].stride(0), q["rows"], q["cols"],
            -(-q["n_kept"] // 128) * 128)


def _closure_projected_bucket_key(q):
    """Truncated requests with equal keys may share one ``gpfit_fit_eval_projected_batch`` call: the regime (the
    regimes never share a call), what that call shares between its units, the padded basis size (the recursion's split,
    hence the bits, depend on it) and the capacity of the workspace (the slab counts and the lift's route depend on it)."""
    return ("truncated", q["x"].device.index, q["stream"].value, q["N"], q["x"].stride(0), q["rows"], q["cols"],
            -(-q["n_kept"] // 128) * 128, q["cap"])


def _closure_bucket_key(q):
    """The bucket key of a closure request of any regime: ``_request_bucket_key`` without its leading kind."""
    return _request_kind(q).key(q)


def _closure_batch_raw(ctxs, qs, out=None, rcs=None):
    """``gpfit_fit_eval_sparse_batch`` on sparse requests ``qs``, ``gpfit_fit_eval_projected_batch`` (the same argument list
    without xtilde) on truncated ones, with the contexts ``ctxs`` (one per request): the return code, the 16 outputs per
    unit and the per-unit codes, nothing checked here -- the shared arguments, and the choice of the entry point, are
    those of ``qs[0]``.  A tensor given as None goes in as a null pointer; ``out`` / ``rcs``: the caller's arrays instead of
    new ones."""
    nu, q0 = len(qs), qs[0]
    out = (ctypes.c_double * (16 * nu))() if out is None else out
    rcs = (ctypes.c_int * nu)() if rcs is None else rcs
    name = "gpfit_fit_eval_sparse_batch" if "xt" in q0 else "gpfit_fit_eval_projected_batch"
    xt = (_ptr_table(qs, "xt"), q0["xt"].stride(0), q0["Nt"]) if "xt" in q0 else ()
    rc = getattr(_lib.load(), name)(
        _ctx_table(ctxs), nu, q0["stream"], _flat(qs, "theta"), _flat(qs, "lower"), _flat(qs, "upper"), q0["rows"], q0["cols"],
        _ptr_table(qs, "x"), q0["x"].stride(0), q0["N"], *xt, _ptr_table(qs, "r"), _ptr_table(qs, "B"),
        _ld_table(qs, "B", "n_kept"), (ctypes.c_int64 * nu)(*[q["n_kept"] for q in qs]), _ptr_table(qs, "m_b"),
        _ptr_table(qs, "V_b"), _ld_table(qs, "V_b", "n_kept"), _lib.darr([q["logA"] for q in qs]),
        _lib.darr([q["lambda0"] for q in qs]), out, rcs)
    return rc, out, rcs


def _closure_unit(q, u, out, rcs):
    """What ``_closure_run_single`` returns, for unit ``u`` of a batch call: ``(rc, out[16])``."""
    return int(rcs[u]), list(out[16 * u:16 * u + 16])


def _closure_finish(q, rc_, out, steps):
    """What ``_closure_sparse`` / ``_closure_projected`` returns or raises for the code and the outputs the device call gave
    its request; a non-positive pivot (``rc_ > 0``) takes the kind's step-by-step formulation ``steps``, in the caller's
    own thread."""
    if rc_ == -2:
        _lib.load().gpfit_check_limits(_lib.darr(q["theta"]), _lib.darr(q["lower"]), _lib.darr(q["upper"]))   # its message
        raise ValueError(_lib.last_error())
    if rc_ == 0:
        return out[0], {k: out[3 + i] for i, k in enumerate(THETA_KEYS)}
    return steps(*q["args"])


# The names under which each regime's entry function reaches the code the two regimes share: the tests call them, and
# count a regime's device calls by wrapping its prepare.
_closure_sparse_prepare = _closure_projected_prepare = _closure_prepare
_closure_projected_run_single = _closure_run_single
_closure_projected_batch_raw = _closure_batch_raw


def _closure_size(units):
    """``n, d, d_full`` of the workspaces a group of closure units needs (``_group_engines``)."""
    rows, cols = _grid(units[0]["n_px_side"])
    n = max(max(u["x"].shape[0], u["xtilde"].shape[0] if "xtilde" in u else 0) for u in units)
    return n, units[0]["x"].shape[1], rows * cols


def _closure_projected_group(units):
    """``_closure_projected`` for several independent units (cells, restarts of one cell) as ONE device call
    (``gpfit_fit_eval_projected_batch``).  ``units``: one dict per unit with the arguments of ``_closure_projected`` by
    name; 1 .. 16 units of one bucket (``_closure_bucket_key``).  Returns, per unit, what ``_closure_projected`` returns
    for it on a workspace created for its number of stimuli, bit for bit (a closure's slab counts and the route of its
    lift, hence its last bits, depend on the capacity of the workspace: the units here run on workspaces of that one
    capacity, whatever the size of the thread's own); a unit whose call would raise has the exception in its place, and
    a unit whose factorisation fails takes the step-by-step formulation alone."""
    return _units_group("_closure_projected_group", units, _closure_size, _closure_prepare, _closure_projected_steps,
                        exact=True)


def _closure_adjoints(K_b, K_tilde_b, Kvec, a, m_b, V_b, r, f_params):
    """The algebra the two step-by-step closures share, from the projected kernel objects to the adjoints of the loss
    (docstring of ``_closure_projected_steps``).  ``a``: the matrix of the moments -- B for the truncated-rank closure, None
    for the sparse one's a = K_b K~_b^-1.  Returns the loss and what the callers lift to their W matrices:
    (loss, g_v, G_Kb, G_Kb~)."""
    A = math.exp(_scalar(f_params['logA']))
    lambda0 = _scalar(_lambda0_of(f_params))
    Ki = spd_inverse(K_tilde_b)                                                     # :2067
    if a is None:
        a = matmul(K_b, Ki)                                                         # :2068
    aV = matmul(a, V_b)
    lambda_m = matmul(a, m_b)                                                       # :1090
    lambda_var = Kvec - torch.sum(a * K_b, 1) + torch.sum(aV * a, 1)                 # :1101
    f_mean = torch.exp(A * lambda_m + 0.5 * A * A * lambda_var + lambda0)            # :1138
    loglik = A * torch.dot(r, lambda_m) + lambda0 * torch.sum(r) - torch.sum(f_mean)  # :1243
    b = matmul(Ki, m_b)
    KiV = matmul(Ki, V_b)
    KL = (-0.5 * log_det(V_b, 'V', ignore_warning=True) + 0.5 * log_det(K_tilde_b, 'K_tilde', ignore_warning=True)
          + 0.5 * torch.dot(m_b, b) + 0.5 * torch.trace(KiV))                        # :1326
    g_m = A * (r - f_mean)
    g_v = -0.5 * A * A * f_mean
    G_a = torch.outer(g_m, m_b) - g_v[:, None] * K_b + 2.0 * g_v[:, None] * aV
    G_aKi = matmul(G_a, Ki)
    G_Kb = g_v[:, None] * a - G_aKi
    G_Ktb = 0.5 * Ki - 0.5 * torch.outer(b, b) - 0.5 * matmul(KiV, Ki) + matmul(a, G_aKi, transA=True)
    return -(_scalar(loglik) - _scalar(KL)), g_v, G_Kb, G_Ktb


def _closure_projected_steps(theta, lims, n_px_side, x, r, B, m_b, V_b, f_params):
    """Truncated-rank M-step closure (utils.py:2030-2099 with n < n_tilde = n_t, inducing set =
    training set) in adjoint form: the same loss as the reference's B-projected formulation, but
    instead of materialising the six dK~_p and projecting each of them (13 + 13 GEMMs of N x N x n),
    the n x n / N x n adjoints of the loss are formed once, lifted to
    ``W = (B G_Kb~ + G_Kb) B^T`` and contracted with the analytic dK~_p by the fused pull-back
    (``gpfit_grad_pullback``).  As in the reference, with n_tilde == n_t the moments use a = B
    (utils.py:2068) while their derivatives use da_p = (dK_b,p - a dK~_b,p) K~_b^-1 (utils.py:1114);
    collecting the coefficients of dK_b,p, dK~_b,p and dKvec_p in dKL_p - dloglik_p
    (utils.py:1117-1120, 1266, 1331-1333) with g_m = A (r - f), g_v = -A^2 f / 2:
      G_a   = g_m m_b^T - diag(g_v) K_b + 2 diag(g_v) B V_b
      G_Kb  = diag(g_v) B - G_a K~_b^-1
      G_Kb~ = 1/2 K~_b^-1 - 1/2 b b^T - 1/2 K~_b^-1 V_b K~_b^-1 + B^T G_a K~_b^-1 ,  gvec = -g_v.
    Validated against the reference on the truncated golden fixture (1e-10) and against the
    literal formulation (``_closure_general``) at scale."""
    lib = _lib.load()
    lower, upper = lims
    th = _lib.darr(theta_vec(theta))
    if lib.gpfit_check_limits(th, _lib.darr([_scalar(lower[k]) for k in THETA_KEYS]),
                              _lib.darr([_scalar(upper[k]) for k in THETA_KEYS])) != 0:
        raise ValueError(_lib.last_error())
    C, mask = localker(theta=theta, theta_higher_lims=upper, theta_lower_lims=lower, n_px_side=n_px_side, grad=False)
    x_m = x[:, mask].contiguous()
    K_tilde = acosker(theta, x_m, x_m, C=C, dC=None, diag=False)
    Kvec = acosker(theta, x_m, x2=None, C=C, dC=None, diag=True)
    K_b = matmul(K_tilde, B)                                                        # :2049
    K_tilde_b = matmul(B, K_b, transA=True)                                         # :2047
    K_tilde_b = (K_tilde_b + K_tilde_b.T) * 0.5                                     # :2048
    loss, g_v, G_Kb, G_Ktb = _closure_adjoints(K_b, K_tilde_b, Kvec, B, m_b, V_b, r, f_params)   # a = B (:2068, n_tilde == n_t)
    W = matmul(matmul(B, G_Ktb) + G_Kb, B, transB=True)
    W = ((W + W.T) * 0.5).contiguous()
    gvec = (-g_v).contiguous()
    rows, cols = _grid(n_px_side)
    xc = _cu(x)
    eng = get_engine(xc.shape[0], int(mask.sum()), rows * cols)
    out = (ctypes.c_double * 6)()
    _lib.check(lib.gpfit_grad_pullback(eng._ctx, _stream(), th, rows, cols, xc.data_ptr(), xc.stride(0), xc.shape[0],
                                       W.data_ptr(), W.stride(0), gvec.data_ptr(), out), "gpfit_grad_pullback")
    grad = {k: out[i] for i, k in enumerate(THETA_KEYS)}
    return loss, grad


def _closure_sparse(theta, lims, n_px_side, x, xtilde, r, B, m_b, V_b, f_params):
    """Sparse M-step closure (n_tilde < n_t; utils.py:2030-2099, 1114-1120): ONE call of the fused entry
    point ``gpfit_fit_eval_sparse``; the step-by-step formulation below (``_closure_sparse_steps``) is
    the path taken when a factorisation meets a non-positive pivot (reference's eigen-fallback of
    ``log_det``, utils.py:1279-1304).  In a fit of ``varGP_cells`` the device call is the wave's: the request goes
    to the rendezvous and comes back as one unit of a ``gpfit_fit_eval_sparse_batch`` call, with the same bits."""
    q = _closure_sparse_prepare(theta, lims, n_px_side, x, r, B, m_b, V_b, f_params, xtilde=xtilde)
    return _closure_finish(q, *_submit(q), _closure_sparse_steps)


def _closure_sparse_group(units):
    """``_closure_sparse`` for several independent units (cells, restarts of one cell) as ONE device call
    (``gpfit_fit_eval_sparse_batch``).  ``units``: one dict per unit with the arguments of ``_closure_sparse`` by name;
    1 .. 16 units of one ``_closure_bucket_key``.  Returns, per unit, what ``_closure_sparse`` returns for it, bit for
    bit; a unit whose call would raise has the exception in its place, and a unit whose factorisation fails takes the
    step-by-step formulation alone."""
    return _units_group("_closure_sparse_group", units, _closure_size, _closure_prepare, _closure_sparse_steps)


def _closure_full(theta, lims, n_px_side, x, r, m, V, f_params, reuse_V):
    """Full-rank M-step closure (``m``, ``V`` in the original basis): ONE ``fit_eval`` call on this thread's workspace,
    which keeps V's factor between the closures of an M-step (``reuse_V``).  In a fit of ``varGP_cells`` the device call
    is the wave's (unless ``FULL_RANK_GROUPS`` is off): the request goes to the rendezvous and comes back as one unit of
    a ``gpfit_fit_eval_batch`` call on the fits' own workspaces, with the same bits.  Returns the result dict of
    ``fit_eval`` or raises what it raises.  ``theta`` is within ``lims``: the caller has checked."""
    lower, upper = lims
    rows, cols = _grid(n_px_side)
    xc = _cu(x)
    q = {"kind": "closure", "regime": "full", "theta": [float(v) for v in theta_vec(theta)],
         "lower": [_scalar(lower[k]) for k in THETA_KEYS], "upper": [_scalar(upper[k]) for k in THETA_KEYS],
         "n_px_side": n_px_side, "rows": rows, "cols": cols, "x": xc, "r": _cu(r), "m": _cu(m), "V": _cu(V),
         "N": int(xc.shape[0]), "logA": _scalar(f_params['logA']), "lambda0": _scalar(_lambda0_of(f_params)),
         "reuse_V": bool(reuse_V)}
    _request_place(q, None, q["N"], xc.shape[1], rows * cols)
    q["cap"] = -(-q["engine"].n_max // 128) * 128
    return _submit(q)


def _closure_full_run_single(q):
    """``fit_eval`` on one full-rank request, on the request's workspace: its result dict (or its exception)."""
    return q["engine"].fit_eval(q["theta"], q["lower"], q["upper"], q["n_px_side"], q["x"], q["r"], q["m"], q["V"], q["logA"],
                                q["lambda0"], want_grad=True, want_vectors=False, reuse_V=q["reuse_V"])


def _closure_full_bucket_key(q):
    """Full-rank requests with equal keys may share one ``gpfit_fit_eval_batch`` call: the regime (the regimes never share
    a call), what that call shares between its units -- the ``reuse_V`` flag among it: the first closures of an M-step
    and later ones never meet in one call -- and the capacity of the workspaces."""
    return ("full", q["x"].device.index, q["stream"].value, q["N"], q["x"].stride(0), q["V"].stride(0), q["rows"], q["cols"],
            q["cap"], q["reuse_V"])


def _closure_full_batch_raw(ctxs, qs, out=None, rcs=None):
    """``gpfit_fit_eval_batch`` on the full-rank requests ``qs`` with the contexts ``ctxs`` (their own workspaces', which
    hold their V factors): the return code, the 16 outputs per unit and the per-unit codes, nothing checked here -- the
    shared arguments are those of ``qs[0]``.  No limits go in: every request's theta has been checked on the host."""
    nu, q0 = len(qs), qs[0]
    out = (ctypes.c_double * (16 * nu))() if out is None else out
    rcs = (ctypes.c_int * nu)() if rcs is None else rcs
    rc = _lib.load().gpfit_fit_eval_batch(
        _ctx_table(ctxs), nu, q0["stream"], _flat(qs, "theta"), None, None, q0["rows"], q0["cols"], _ptr_table(qs, "x"),
        q0["x"].stride(0), q0["N"], _ptr_table(qs, "r"), _ptr_table(qs, "m"), _ptr_table(qs, "V"), q0["V"].stride(0),
        _lib.darr([q["logA"] for q in qs]), _lib.darr([q["lambda0"] for q in qs]), 1 | (2 if q0["reuse_V"] else 0), out, rcs)
    return rc, out, rcs


def _closure_full_unit(q, u, out, rcs):
    """What ``_closure_full_run_single`` returns, for unit ``u`` of a batch call, with the same bits -- or, in its place,
    the exception ``fit_eval`` raises for that unit alone (a failed factorisation).  Every pending unit of the call is
    collected (``fit_eval_finish``), also behind a failed one."""
    ticket = {"rc": int(rcs[u]), "out": (ctypes.c_double * 16)(*out[16 * u:16 * u + 16]), "pending": rcs[u] == 0,
              "lam_m": None, "lam_var": None, "f": None}
    try:
        return q["engine"].fit_eval_finish(ticket)
    except Exception as err:    # this unit's alone
        return err


def _loss_prepare(r, f_mean, lambda_m, f_params, m, V, K_tilde, K_tilde_inv, logdet_K=None, engine=None):
    """The arguments of ``elbo_terms`` as one request (kind ``"loss"``): the operands contiguous on the device, read
    only; ``K`` is left out when ``logdet_K`` is given.  The workspace and stream are this thread's unless an engine is
    given."""
    r, f, lam_m, m, V, Kinv = (_cu(t) for t in (r, f_mean, lambda_m, m, V, K_tilde_inv))
    nb = int(m.shape[0])
    q = {"kind": "loss", "r": r, "f": f, "lam_m": lam_m, "m": m, "V": V, "Kinv": Kinv,
         "K": None if logdet_K is not None else _cu(K_tilde), "N": int(r.shape[0]), "nb": nb,
         "logdet_K": None if logdet_K is None else float(logdet_K), "logA": _scalar(f_params['logA']),
         "lambda0": _scalar(_lambda0_of(f_params))}
    return _request_place(q, engine, nb, 1)


def _loss_result(q, u, out, info):
    """What a loss call returns for its unit ``u``: the ten numbers of ``gpfit_elbo`` and the two info words (V's,
    K~'s)."""
    return list(out[10 * u:10 * u + 10]), (int(info[2 * u]), int(info[2 * u + 1]))


def _loss_run_single(q):
    """``gpfit_elbo`` on one request.  A positive return code (a failed factorisation) is in the info words."""
    out, info = (ctypes.c_double * 10)(), (ctypes.c_int * 2)()
    known, K = q["logdet_K"] is not None, q["K"]
    _lib.check(_lib.load().gpfit_elbo(q["engine"]._ctx, q["stream"], q["m"].data_ptr(), q["V"].data_ptr(), q["V"].stride(0),
                                      None if K is None else K.data_ptr(), q["nb"] if K is None else K.stride(0),
                                      q["Kinv"].data_ptr(), q["Kinv"].stride(0), q["nb"], 1 if known else 0,
                                      q["logdet_K"] if known else 0.0, q["r"].data_ptr(), q["f"].data_ptr(),
                                      q["lam_m"].data_ptr(), q["N"], q["logA"], q["lambda0"], out, info),
               "gpfit_elbo")
    return _loss_result(q, 0, out, info)


def _loss_bucket_key(q):
    """Requests with equal keys may share one ``gpfit_elbo_batch`` call: the device and stream, then what that call
    shares between its units -- N and the padded basis size (the recursion's split, hence the bits, depend on it)."""
    return (q["m"].device.index, q["stream"].value, q["N"], -(-q["nb"] // 128) * 128)


def _loss_batch_raw(ctxs, qs, out=None, info=None):
    """``gpfit_elbo_batch`` on the requests ``qs`` with the contexts ``ctxs`` (one per request): the return code and the
    two output arrays, nothing checked here -- N is that of ``qs[0]``.  A tensor given as None goes in as a null
    pointer, a leading dimension given as ``q["ldv"]`` / ``q["ldk"]`` / ``q["ldki"]`` replaces the tensor's."""
    nu, q0 = len(qs), qs[0]
    out = (ctypes.c_double * (10 * nu))() if out is None else out
    info = (ctypes.c_int * (2 * nu))() if info is None else info
    rc = _lib.load().gpfit_elbo_batch(
        _ctx_table(ctxs), nu, q0["stream"], _ptr_table(qs, "m"), _ptr_table(qs, "V"), _ld_table(qs, "V", "nb", "ldv"),
        _ptr_table(qs, "K"), _ld_table(qs, "K", "nb", "ldk"), _ptr_table(qs, "Kinv"), _ld_table(qs, "Kinv", "nb", "ldki"),
        (ctypes.c_int64 * nu)(*[q["nb"] for q in qs]), (ctypes.c_int * nu)(*[0 if q["logdet_K"] is None else 1 for q in qs]),
        _lib.darr([0.0 if q["logdet_K"] is None else q["logdet_K"] for q in qs]), _ptr_table(qs, "r"), _ptr_table(qs, "f"),
        _ptr_table(qs, "lam_m"), q0["N"], _lib.darr([q["logA"] for q in qs]), _lib.darr([q["lambda0"] for q in qs]), out, info)
    return rc, out, info


def elbo_terms(r, f_mean, lambda_m, f_params, m, V, K_tilde, K_tilde_inv, logdet_K=None, ignore_warning=True, grouped=True):
    """``(loglikelihood, KL_div)`` of the tracked loss -- ``compute_loglikelihood(r, f_mean, lambda_m, ., f_params)[0]``
    and ``compute_KL_div(m, V, K_tilde, K_tilde_inv, ignore_warning=True)`` -- as ONE device call and one wait
    (``gpfit_elbo``): V is factored for its log-determinant, ``tr(V K~^-1)`` and ``m^T K~^-1 m`` are one pass over the
    two matrices in place of the nb^3 product, the three likelihood sums ride along.  ``logdet_K``: log|K~| where the
    caller holds it (from ``cholesky(K_tilde)``); without it the call factors K~ beside V.  In a fit of ``varGP_cells``
    the call is the wave's (``_submit``: one ``gpfit_elbo_batch`` call, the same bits) unless ``grouped`` is off (a
    fit that keeps its turn: the full-rank regime with ``FULL_RANK_GROUPS`` off).  Both results are 0-d fp64
    tensors on the device, as the two functions return them.

    The composite calls are made exactly as ever, with their warnings (``ignore_warning`` is ``compute_KL_div``'s) and
    the eigen fall-back of ``log_det``, when ``FUSED_LOSS`` is off and when a factorisation of the fused call fails."""
    if FUSED_LOSS:
        q = _loss_prepare(r, f_mean, lambda_m, f_params, m, V, K_tilde, K_tilde_inv, logdet_K)
        out, info = _submit(q) if grouped else _loss_run_single(q)
        if info == (0, 0):
            dev = _device()
            return (torch.tensor(out[0], dtype=TORCH_DTYPE, device=dev), torch.tensor(out[1], dtype=TORCH_DTYPE, device=dev))
    loglikelihood = compute_loglikelihood(r, f_mean, lambda_m, lambda_m, f_params)[0]   # (lambda_var: gradients only)
    return loglikelihood, compute_KL_div(m, V, K_tilde, K_tilde_inv, dK_tilde=None, ignore_warning=ignore_warning)


# What the rendezvous of varGP_cells is given: the kinds of request, one record each, keyed by (kind, regime) -- only a
# closure request has a regime.  ``book``: the counters its calls are counted in (one of _ALL_BOOKS); ``switch``: the
# name of the module switch that, off, keeps the kind out of the rendezvous (None: the kind always goes there);
# ``run_single(q)``: the single entry point; ``batch(ctxs, qs)``: the batch entry point ``entry``, unchecked -- its return
# code, then its output arrays; ``unit(q, u, *arrays)``: the result of unit u cut out of them, what run_single returns
# for q alone; ``key(q)``: requests of one kind with equal keys may share a call; ``share``: what that means, for the
# error.
_RequestKind = collections.namedtuple("_RequestKind", "kind regime book switch run_single entry batch unit key share")
_REQUEST_KINDS = {(k.kind, k.regime): k for k in (
    _RequestKind(kind="chain", regime=None, book="", switch=None, run_single=_chain_run_single,
                 entry="gpfit_estep_chain_batch", batch=_chain_batch_raw, unit=_chain_result, key=_chain_bucket_key,
                 share="the requests of one call share N, the padded basis size, the number of steps and the optimiser's "
                 "settings"),
    _RequestKind(kind="chain_damped", regime=None, book="", switch=None, run_single=_chain_damped_run_single,
                 entry="gpfit_estep_chain_damped_batch", batch=_chain_damped_batch_raw, unit=_chain_result,
                 key=_chain_damped_bucket_key,
                 share="the requests of one call share N, the padded basis size, the step size alpha, the number of steps "
                 "and the optimiser's settings"),
    _RequestKind(kind="chain_full", regime=None, book="full_", switch="FULL_RANK_GROUPS", run_single=_chain_full_run_single,
                 entry="gpfit_estep_chain_full_batch", batch=_chain_full_batch_raw, unit=_chain_result,
                 key=_chain_full_bucket_key,
                 share="the requests of one call share N, the number of steps and the optimiser's settings"),
    _RequestKind(kind="closure", regime=None, book="closure_", switch=None, run_single=_closure_run_single,
                 entry="gpfit_fit_eval_sparse_batch", batch=_closure_batch_raw, unit=_closure_unit,
                 key=_closure_sparse_bucket_key,
                 share="the requests of one call share the stimuli's sizes and leading dimensions, the pixel grid and the "
                 "padded basis size"),
    _RequestKind(kind="closure", regime="truncated", book="closure_", switch=None, run_single=_closure_run_single,
                 entry="gpfit_fit_eval_projected_batch", batch=_closure_batch_raw, unit=_closure_unit,
                 key=_closure_projected_bucket_key,
                 share="the truncated requests of one call share the stimuli's size and leading dimension, the pixel grid, "
                 "the padded basis size and the capacity of their workspaces"),
    _RequestKind(kind="closure", regime="full", book="full_closure_", switch="FULL_RANK_GROUPS",
                 run_single=_closure_full_run_single, entry="gpfit_fit_eval_batch", batch=_closure_full_batch_raw,
                 unit=_closure_full_unit, key=_closure_full_bucket_key,
                 share="the full-rank requests of one call share the stimuli's size and leading dimension, the pixel grid, "
                 "the capacity of their workspaces and the reuse_V flag"),
    _RequestKind(kind="loss", regime=None, book="loss_", switch=None, run_single=_loss_run_single,
                 entry="gpfit_elbo_batch", batch=_loss_batch_raw, unit=_loss_result, key=_loss_bucket_key,
                 share="the requests of one call share N and the padded basis size"),
    _RequestKind(kind="sweeps", regime=None, book="basis_", switch="BASIS_GROUPS", run_single=_sweeps_run_single,
                 entry="gpfit_subspace_sweeps_batch", batch=_sweeps_batch_raw, unit=_sweeps_result, key=_sweeps_bucket_key,
                 share="the requests of one call share the device, the stream, N, the block width, the flags and the "
                 "capacity of their workspaces"),
    _RequestKind(kind="sign", regime=None, book="basis_", switch="BASIS_GROUPS", run_single=_sign_run_single,
                 entry="gpfit_sign_steps_batch", batch=_sign_batch_raw, unit=_sign_result, key=_sign_bucket_key,
                 share="the requests of one call share the device, the stream, k, the flags, the schedule and the "
                 "capacity of their workspaces"))}


def _request_kind(q):
    """The record of the request's kind."""
    return _REQUEST_KINDS[q["kind"], q.get("regime")]


def _request_run_single(q):
    return _request_kind(q).run_single(q)


def _request_bucket_key(q):
    return (q["kind"],) + _request_kind(q).key(q)


def _request_run_group(qs):
    """One call of the batch entry point of the requests' kind on requests of one bucket (``_request_bucket_key``), each
    on its own workspace; per request what the kind's ``run_single`` returns, with the same bits."""
    kind = _request_kind(qs[0])
    if len({_request_bucket_key(q) for q in qs}) != 1:
        raise ValueError(f"{kind.entry}: {kind.share}")
    rc, *arrays = kind.batch([q["engine"]._ctx for q in qs], qs)
    _lib.check(rc, kind.entry)
    return [kind.unit(q, u, *arrays) for u, q in enumerate(qs)]


def _submit(q):
    """The result of the request's device call: in a fit of ``varGP_cells`` the call is the wave's -- the request goes to
    the rendezvous and comes back as one unit of a group call -- unless the kind names a module switch
    (``FULL_RANK_GROUPS``, ``BASIS_GROUPS``; read here, at call time) and that switch is off; anywhere else it is the kind's
    single call."""
    kind = _request_kind(q)
    rendezvous = getattr(_CELLS, "rendezvous", None)
    if rendezvous is not None and (kind.switch is None or globals()[kind.switch]):
        return rendezvous.call(q)
    return kind.run_single(q)


def _closure_sparse_steps(theta, lims, n_px_side, x, xtilde, r, B, m_b, V_b, f_params):
    """Sparse M-step closure (n_tilde < n_t: K[n_t, n_tilde] != K~, a = K_b K~_b^-1 with non-zero
    da_p; utils.py:2030-2099, 1114-1120) in adjoint form.  Two adjoint matrices come out of the
    same algebra as in ``_closure_projected`` (with a = K_b K~_b^-1 this time):
      W~ = B G_Kb~ B^T  (n_tilde x n_tilde, contracts with dK~_p)  -> ``gpfit_grad_pullback`` on xtilde,
      W_K = G_Kb B^T    (n_t x n_tilde, contracts with dK_p)       -> rectangular pull-back below:
    with c, delta the cosine / angle matrix of (x, xtilde), A_w = W_K o (pi - delta)/pi,
    B_m = W_K o sqrt(1 - c^2)/pi, u1 = B_m q2, u2 = B_m^T q1,
      sum_ij W_K,ij dK_p,ij = <dC_p, x^T A_w xt + x^T diag(u1 / 2 q1) x + xt^T diag(u2 / 2 q2) xt>
    (sigma_0: 2 s0 sum A_w + s0 sum u1/q1 + s0 sum u2/q2), from utils.py:996-1021; the dKvec term
    adds x^T diag(gvec) x.  Both pull-backs are fused entry points (``gpfit_grad_pullback``,
    ``gpfit_acosker_pullback``); only the five d x d contractions with dC_p stay in torch.
    Validated against the reference on the sparse golden fixture."""
    lib = _lib.load()
    lower, upper = lims
    th = _lib.darr(theta_vec(theta))
    C, mask, dC = localker(theta=theta, theta_higher_lims=upper, theta_lower_lims=lower, n_px_side=n_px_side, grad=True)
    x_m, xt_m = x[:, mask].contiguous(), xtilde[:, mask].contiguous()
    s0 = _scalar(theta['sigma_0'])
    K_tilde = acosker(theta, xt_m, xt_m, C=C, dC=None, diag=False)
    Kvec = acosker(theta, x_m, x2=None, C=C, dC=None, diag=True)
    K = acosker(theta, x_m, xt_m, C=C, dC=None, diag=False)                          # :968-990
    K_b = matmul(K, B)                                                              # :2049
    K_tilde_b = matmul(B, matmul(K_tilde, B), transA=True)                          # :2047
    K_tilde_b = (K_tilde_b + K_tilde_b.T) * 0.5                                     # :2048
    loss, g_v, G_Kb, G_Ktb = _closure_adjoints(K_b, K_tilde_b, Kvec, None, m_b, V_b, r, f_params)   # a = K_b K~_b^-1 (:2068)
    # square part: W~ against dK~_p
    Wt = matmul(matmul(B, G_Ktb), B, transB=True)
    Wt = ((Wt + Wt.T) * 0.5).contiguous()
    rows, cols = _grid(n_px_side)
    xtc = _cu(xtilde)
    eng = get_engine(xtc.shape[0], int(mask.sum()), rows * cols)
    zero = torch.zeros(xtc.shape[0], dtype=TORCH_DTYPE, device=xtc.device)
    out = (ctypes.c_double * 6)()
    _lib.check(lib.gpfit_grad_pullback(eng._ctx, _stream(), th, rows, cols, xtc.data_ptr(), xtc.stride(0), xtc.shape[0],
                                       Wt.data_ptr(), Wt.stride(0), zero.data_ptr(), out), "gpfit_grad_pullback")
    grad = {k: out[i] for i, k in enumerate(THETA_KEYS)}
    # rectangular part: W_K against dK_p, and gvec against dKvec_p (fused pull-back, nothing n_t x n_tilde x 6)
    W_K = matmul(G_Kb, B, transB=True).contiguous()
    gvec = (-g_v).contiguous()
    d = int(mask.sum())
    Cc = _cu(C)
    M = torch.empty((d, d), dtype=TORCH_DTYPE, device=x_m.device)
    out3 = (ctypes.c_double * 3)()
    eng2 = get_engine(max(x_m.shape[0], xt_m.shape[0]), d, rows * cols)
    _lib.check(lib.gpfit_acosker_pullback(eng2._ctx, _stream(), s0, x_m.data_ptr(), x_m.stride(0), x_m.shape[0],
                                          xt_m.data_ptr(), xt_m.stride(0), xt_m.shape[0], d, Cc.data_ptr(), Cc.stride(0),
                                          W_K.data_ptr(), W_K.stride(0), gvec.data_ptr(), M.data_ptr(), M.stride(0), out3),
               "gpfit_acosker_pullback")
    M = (M + M.T) * 0.5
    for k in DC_KEYS:
        grad[k] += _scalar(torch.sum(dC[k] * M))
    grad['sigma_0'] += s0 * (2.0 * out3[0] + out3[1] + out3[2]) + 2 * s0 * _scalar(gvec.sum())
    return loss, grad


@torch.no_grad()
def extend_inducing_set(fit_model, x_new, route=None):
    """One image more in the inducing set of a fitted model: everything ``varGP(..., m=, V=, init_kernel=)`` needs
    to refit from the previous posterior, as the closed loop of ``one_cell_active_training.ipynb`` (:1889-1936)
    prepares it -- K~ grown "by its latest column", the stabilised basis of the grown matrix, the previous
    ``(m, V)`` carried over with a unit variance and the mean of ``m`` for the new point.

    Where the notebook eigendecomposes the grown K~ for every added image (:1900), this uses what the previous fit
    left behind: when its basis was the identity (every eigenvalue kept) and its factor is in
    ``final_kernel['chol']``, ``L`` and ``L^-1`` are extended by one row in O(n^2) (``cholesky_append``,
    ``gpfit_potrf_append``) and the same rigorous bounds that proved "all kept" for the old matrix are evaluated
    for the new one -- no ``eigh``, no refactorisation.  If the bounds no longer prove it (or no factor was kept)
    the grown matrix goes through ``_stabilised_basis`` like any other.

    Returns ``dict(xtilde=, m=, V=, init_kernel=)``; ``x_new`` is one image (any shape with the model's pixel
    count) or the several images of a round (anything that reshapes to ``[-1, n_pixels]``): those are prepared in one
    go, the factor grown by one block step (``_extend_inducing_block``), while one image takes the rank-1 step below
    with the bits it always had.  The caller updates ``fit_parameters['ntilde']``.  PRECONDITION (the closed loop of the notebook, where
    ``in_use_idx == xtilde_idx``): the refit's training set is the grown inducing set, ``x == xtilde`` -- the
    ``init_kernel`` returned here carries ``K = K~`` and ``KKtilde_inv_b = B``, which is only the kernel of THAT
    training set; ``varGP`` refuses it for any other (``init_kernel['square']``).
    ``route='eigh'`` forces the notebook's own step (eigendecomposition of the grown matrix), for A/B timing."""
    xt = _cu(fit_model['xtilde'])
    n, npx = xt.shape
    x_new = _cu(x_new)
    if x_new.numel() == 0 or x_new.numel() % npx != 0:
        raise ValueError(f"extend_inducing_set: the new image has {x_new.numel()} pixels, the model {npx}")
    if x_new.numel() > npx:
        return _extend_inducing_block(fit_model, x_new.reshape(-1, npx), route)
    row = x_new.reshape(1, -1)
    theta = fit_model['hyperparams_tuple'][0]
    fk = fit_model['final_kernel']
    C, mask = _cu(fit_model['C']), fit_model['mask'].to(xt.device)
    K_old, Kvec_old = _cu(fk['K_tilde']), _cu(fk['Kvec'])
    xt_new = torch.cat((xt, row), 0)
    xm = xt_new[:, mask].contiguous()
    col = acosker(theta, xm, xm[n:n + 1].contiguous(), C=C, dC=None, diag=False).reshape(-1)       # latest column, n + 1 entries
    K_new = torch.empty((n + 1, n + 1), dtype=TORCH_DTYPE, device=xt.device)
    K_new[:n, :n] = K_old
    K_new[:n, n] = col[:n]
    K_new[n, :] = col
    Kvec_new = torch.cat((Kvec_old, acosker(theta, xm[n:n + 1].contiguous(), x2=None, C=C, dC=None, diag=True).reshape(-1)))
    # previous posterior in the coordinates of the images, grown by the new point (notebook: identity block, mean of m)
    B_old = fit_model['B']
    if _is_identity(B_old) or fit_model.get('basis_route') == 'identity':
        m_img, V_img = _cu(fit_model['m_b']), _cu(fit_model['V_b'])
    else:
        B_old = _cu(B_old)
        m_img = matmul(B_old, _cu(fit_model['m_b']))
        V_img = matmul(B_old, matmul(_cu(fit_model['V_b']), B_old, transB=True))
    V_new = torch.eye(n + 1, dtype=TORCH_DTYPE, device=xt.device)
    V_new[:n, :n] = (V_img + V_img.T) * 0.5
    m_new = torch.cat((m_img, m_img.mean().reshape(1)))
    # basis of the grown matrix
    forced, route, chol = route, None, None
    if forced is None and fit_model.get('basis_route') == 'identity' and fk.get('chol') is not None:
        L = torch.zeros((n + 1, n + 1), dtype=TORCH_DTYPE, device=xt.device)
        Li = torch.zeros_like(L)
        L[:n, :n] = _cu(fk['chol']['L'])
        Li[:n, :n] = _cu(fk['chol']['Linv'])
        _, info = cholesky_append(L, Li, col)
        if info == 0 and _all_kept_given_factor(K_new, Li):
            route, chol = 'identity', {'L': L, 'Linv': Li}
            B = _mark_identity(torch.eye(n + 1, dtype=TORCH_DTYPE, device=xt.device))
            Kinv = matmul(Li, Li, transA=True)
            K_b_, K_inv_b = K_new, (Kinv + Kinv.T) * 0.5
    if route is None:
        _BASIS.factor = None
        _, B, K_b_, K_inv_b = _stabilised_basis(K_new, route=forced)
        route = _BASIS.route
        if route == 'identity' and _BASIS.factor is not None:
            chol = {'L': _BASIS.factor[0], 'Linv': _BASIS.factor[1]}
        _BASIS.factor = None
    KB = K_new if route == 'identity' else matmul(K_new, B)
    init_kernel = {'C': C, 'mask': mask, 'K_tilde': K_new, 'K': K_new, 'Kvec': Kvec_new, 'B': B, 'K_tilde_b': K_b_, 'K_b': KB,
                   'K_tilde_inv_b': K_inv_b, 'KKtilde_inv_b': B, 'basis_route': route, 'chol': chol, 'square': True}
    return {'xtilde': xt_new, 'm': m_new, 'V': V_new, 'init_kernel': init_kernel}


def _extend_inducing_block(fit_model, rows, route=None):
    """``extend_inducing_set`` for k > 1 images (a closed-loop round that shows a batch): what k successive calls
    prepare, in one go -- the k new columns of K~ from one ``acosker`` call, the grown tensors copied once, every new
    point with the mean of the old ``m`` (appending its own mean does not move the mean of ``m``) and a unit variance,
    the factor grown by ONE block step (``cholesky_append_block``), the all-kept proof and ``K~^-1 = L^-T L^-1``
    evaluated once, on the grown factor.  The single-image step above is kept as it was, line for line, so that its
    results keep their bits; this is the same sequence with k columns."""
    xt = _cu(fit_model['xtilde'])
    n = xt.shape[0]
    k = rows.shape[0]
    theta = fit_model['hyperparams_tuple'][0]
    fk = fit_model['final_kernel']
    C, mask = _cu(fit_model['C']), fit_model['mask'].to(xt.device)
    K_old, Kvec_old = _cu(fk['K_tilde']), _cu(fk['Kvec'])
    xt_new = torch.cat((xt, rows), 0)
    xm = xt_new[:, mask].contiguous()
    xm_new = xm[n:].contiguous()
    cols = acosker(theta, xm, xm_new, C=C, dC=None, diag=False).reshape(n + k, k)                # latest k columns
    K_new = torch.empty((n + k, n + k), dtype=TORCH_DTYPE, device=xt.device)
    K_new[:n, :n] = K_old
    K_new[:n, n:] = cols[:n]
    K_new[n:, :n] = cols[:n].T
    corner = torch.tril(cols[n:])                                                                 # the new diagonal block from its lower triangle
    K_new[n:, n:] = corner + torch.tril(corner, -1).T
    Kvec_new = torch.cat((Kvec_old, acosker(theta, xm_new, x2=None, C=C, dC=None, diag=True).reshape(-1)))
    B_old = fit_model['B']
    if _is_identity(B_old) or fit_model.get('basis_route') == 'identity':
        m_img, V_img = _cu(fit_model['m_b']), _cu(fit_model['V_b'])
    else:
        B_old = _cu(B_old)
        m_img = matmul(B_old, _cu(fit_model['m_b']))
        V_img = matmul(B_old, matmul(_cu(fit_model['V_b']), B_old, transB=True))
    V_new = torch.eye(n + k, dtype=TORCH_DTYPE, device=xt.device)
    V_new[:n, :n] = (V_img + V_img.T) * 0.5
    m_new = torch.cat((m_img, m_img.mean().reshape(1).expand(k)))
    forced, route, chol = route, None, None
    if forced is None and fit_model.get('basis_route') == 'identity' and fk.get('chol') is not None:
        L = torch.zeros((n + k, n + k), dtype=TORCH_DTYPE, device=xt.device)
        Li = torch.zeros_like(L)
        L[:n, :n] = _cu(fk['chol']['L'])
        Li[:n, :n] = _cu(fk['chol']['Linv'])
        _, info = cholesky_append_block(L, Li, K_new[:, n:].contiguous())
        if info == 0 and _all_kept_given_factor(K_new, Li):
            route, chol = 'identity', {'L': L, 'Linv': Li}
            B = _mark_identity(torch.eye(n + k, dtype=TORCH_DTYPE, device=xt.device))
            Kinv = matmul(Li, Li, transA=True)
            K_b_, K_inv_b = K_new, (Kinv + Kinv.T) * 0.5
    if route is None:
        _BASIS.factor = None
        _, B, K_b_, K_inv_b = _stabilised_basis(K_new, route=forced)
        route = _BASIS.route
        if route == 'identity' and _BASIS.factor is not None:
            chol = {'L': _BASIS.factor[0], 'Linv': _BASIS.factor[1]}
        _BASIS.factor = None
    KB = K_new if route == 'identity' else matmul(K_new, B)
    init_kernel = {'C': C, 'mask': mask, 'K_tilde': K_new, 'K': K_new, 'Kvec': Kvec_new, 'B': B, 'K_tilde_b': K_b_, 'K_b': KB,
                   'K_tilde_inv_b': K_inv_b, 'KKtilde_inv_b': B, 'basis_route': route, 'chol': chol, 'square': True}
    return {'xtilde': xt_new, 'm': m_new, 'V': V_new, 'init_kernel': init_kernel}


@torch.no_grad()
def varGP(x, r, **kwargs):
    """Variational-GP fit (EM) with the reference's call signature and ``fit_model`` schema
    (utils.py:1568-2316): ``varGP(x, r, fit_parameters=..., xtilde=..., hyperparams_tuple=...,
    f_params=..., [m, V, init_kernel])`` -> ``(fit_model, err_dict)``.

    State is kept, as in the reference, in the eigenbasis ``B`` of K~ (``m_b``, ``V_b``).  While
    every eigenvalue is kept and the inducing set is the training set (the regime of the
    north-star configurations) the M-step closure is ONE call of the fused HIP unit of work
    (``gpfit_fit_eval``) and the ``nEstep`` E-steps of an EM iteration ONE call in the original basis
    (``gpfit_estep_chain_full``: the update of ``gpfit_estep``, the moments and the rate-parameter optimiser,
    ``nEstep`` times, with one wait); otherwise the same steps run in the reference's projected formulation on
    the GPU primitives, the E-steps again as one call (``gpfit_estep_chain``).  The host loop around single
    updates stays where a chain does not apply: ``f_params`` carrying ``loglambda0``, ``estep_alpha != 1`` (unless the
    damped chain is switched on, below), more than 1024 E-steps,
    ``GPFIT_ESTEP_CHAIN=0``, and the full-rank regime with a square basis that is not the identity (the ``eigh``
    route keeping every eigenvalue), which rotates by ``B`` around every update.

    Deviations from the reference's ``fit_model``, both additive or opt-out:
    * ``final_kernel['eigvecs']`` (utils.py:2241: the N x N eigenvector matrix of K~) is ``None`` when every
      eigenvalue was kept (no eigendecomposition is computed on that route) and holds only the kept columns when
      the subspace solver built the basis (N >= 256, truncated spectrum); ``fit_parameters['full_eigvecs'] =
      True`` asks for the reference's full matrix (one ``torch.linalg.eigh`` of the final K~ at the end of the fit).
    * extra keys: ``fit_model['basis_route']`` and ``values_track['variation_par_track']['basis_route']``
      (``'identity'`` / ``'eigtop'`` / ``'eigh'`` per tracked iteration): the route that built the basis ``(m_b,
      V_b)`` are expressed in, which ``test(at_iteration=...)`` reproduces or refuses.
    * ``fit_parameters['estep_alpha']`` (default 1: nothing changes) in (0, 1): every E-step takes the damped Newton
      update (``Estep``'s alpha, ``gpfit_estep_projected_damped``) in the host loop, in every regime.  An update whose
      reprojected ``V_b`` is not positive definite takes the full step instead, with a warning;
      ``fit_model['estep_full_steps']`` (present only then) counts them.
    * ``fit_parameters['estep_damped_chain']`` (default: the module's ``DAMPED_CHAIN``, off unless
      ``GPFIT_DAMPED_CHAIN=1``): with ``estep_alpha != 1``, ``f_params`` carrying ``lambda0``, at most 1024 E-steps and
      ``ESTEP_CHAIN`` on, the damped E-steps of an EM iteration are one device call (``_estep_chain_damped``,
      ``gpfit_estep_chain_damped``) in every regime; the full step for a ``V_b`` that is not positive definite is taken
      on the device, with the same warning and count.  Off, nothing in a fit changes."""
    import time
    start_time_before_init = time.time()
    err_dict = {'is_error': False, 'error_message': None}
    x, r = _cu(x), _cu(r)
    nt, nx = x.shape
    dev = x.device
    reserve(nt, nx, nx)

    fit_parameters = copy.deepcopy(kwargs['fit_parameters'])
    fit_parameters['min_tolerance'] = MIN_TOLERANCE
    fit_parameters['eigval_tol'] = EIGVAL_TOL
    ntilde = fit_parameters.get('ntilde', 100 if nt > 100 else nt)
    maxiter = fit_parameters.get('maxiter', 50)
    nEstep = fit_parameters.get('nEstep', 50)
    nMstep = fit_parameters.get('nMstep', 20)
    nFparamstep = fit_parameters.get('nFparamstep', 10)
    display_hyper = fit_parameters.get('display_hyper', True)
    n_px_side = fit_parameters.get('n_px_side', math.sqrt(nx))
    if fit_parameters.get('kernfun', 'acosker') != 'acosker':
        raise Exception('Kernel function not recognized')
    kernfun = acosker

    x_given_as_xtilde = 'xtilde' in kwargs and kwargs['xtilde'] is x
    xtilde = _cu(kwargs['xtilde']) if 'xtilde' in kwargs else generate_xtilde(ntilde, x)
    if ntilde != xtilde.shape[0]:
        raise Exception('Number of inducing points does not match ntilde')
    hyperparams_tuple = (copy.deepcopy(kwargs['hyperparams_tuple']) if 'hyperparams_tuple' in kwargs
                         else generate_theta(x, r, n_px_side, display_hyper))
    theta = copy.deepcopy(kwargs.get('theta', hyperparams_tuple[0]))
    theta_lower_lims = copy.deepcopy(kwargs.get('theta_lower_lims', hyperparams_tuple[1]))
    theta_higher_lims = copy.deepcopy(kwargs.get('theta_higher_lims', hyperparams_tuple[2]))
    lims = (theta_lower_lims, theta_higher_lims)
    if 'f_params' not in kwargs:
        raise Exception('f_params not provided')
    f_params = copy.deepcopy(kwargs['f_params'])
    for key in f_params.keys():
        f_params[key] = f_params[key].detach().to(TORCH_DTYPE).requires_grad_(True)

    same_points = (ntilde == nt) and (x_given_as_xtilde or torch.equal(xtilde, x))
    eigvecs = None
    # step size of the E-step's Newton update (Estep's alpha); != 1: the damped update, one device call per E-step
    estep_alpha = fit_parameters.get('estep_alpha', 1)
    if not 0 < estep_alpha <= 1:
        raise ValueError(f"varGP: fit_parameters['estep_alpha'] must lie in (0, 1], got {estep_alpha}")
    damped = estep_alpha != 1
    estep_full_steps = [0]   # damped E-steps that took the full step because the reprojected V_b was not positive definite
    # the damped updates of an iteration as one device call (opt-in: DAMPED_CHAIN, or this fit's own switch), every regime
    damped_chain = bool(damped and fit_parameters.get('estep_damped_chain', DAMPED_CHAIN) and ESTEP_CHAIN
                        and 'lambda0' in f_params and 'loglambda0' not in f_params and nEstep <= CHAIN_MAX_STEPS)
    if (not ESTEP_CHAIN or 'loglambda0' in f_params or not 0 < nEstep <= CHAIN_MAX_STEPS or maxiter <= 1
            or (damped and not damped_chain)):
        _cells_withdraw()     # under varGP_cells: this fit keeps the host loop, nobody waits for its chains

    def build_kernels(th):
        C_, mask_ = localker(theta=th, theta_lower_lims=theta_lower_lims, theta_higher_lims=theta_higher_lims,
                             n_px_side=n_px_side, grad=False)
        xt_m = xtilde[:, mask_].contiguous()
        Kt = kernfun(th, xt_m, xt_m, C=C_, dC=None, diag=False)
        x_m = xt_m if same_points else x[:, mask_].contiguous()
        K_ = kernfun(th, x_m, xt_m, C=C_, dC=None, diag=False) if ntilde != nt else Kt
        Kv = kernfun(th, x_m, x2=None, C=C_, dC=None, diag=True)
        return C_, mask_, Kt, K_, Kv, x_m

    basis_route = [None]   # route of the basis in force (recorded with every tracked iteration)

    chol_factor = [None]   # (L, L^-1) of the K~ in force when its basis is the identity, else None
    estep_factor = [None]  # (K~_b, its Cholesky factor): shared by the E-steps between two kernel rebuilds
    solver_state = [None]  # the subspace solver's converged block of the previous kernel matrix (warm start)
    ktb_logdet = [None]    # (K~_b, log|K~_b|) where a factor of the K~_b in force came with its log-determinant

    def project(Kt, K_):
        _BASIS.factor = None
        _BASIS.factor_logdet = None
        eigvecs_, B_, Ktb, Ktib = _stabilised_basis(Kt, start=solver_state[0])
        solver_state[0] = getattr(_BASIS, "state", None)     # the subspace solver's block, for the next EM iteration
        _BASIS.state = None
        basis_route[0] = _BASIS.route
        chol_factor[0] = _BASIS.factor if _BASIS.route == "identity" else None
        if chol_factor[0] is not None and _BASIS.factor_logdet is not None:
            ktb_logdet[0] = (Ktb, _BASIS.factor_logdet)      # the identity basis: K~_b is K~, factored by the all-kept proof
        _BASIS.factor = None
        if _is_identity(B_):
            Kb = K_
            a_ = matmul(Kb, Ktib) if ntilde != nt else B_
        else:
            Kb = matmul(K_, B_)
            a_ = matmul(Kb, Ktib) if ntilde != nt else B_
        return eigvecs_, B_, Ktb, Ktib, Kb, a_

    def to_basis_vec(B_, v):
        return v.clone() if _is_identity(B_) else matmul(B_, v, transA=True)

    def to_basis_mat(B_, M):
        if _is_identity(B_):
            return M.clone()
        Mb = matmul(B_, matmul(M, B_), transA=True)
        return Mb

    rate_cache = [None]

    def loss_now(ignore_warning=True):
        """The tracked loss of the state in force (``elbo_terms``), with log|K~_b| where the factor of this K~_b has
        been computed already -- by the all-kept proof behind ``project`` or for the E-steps -- so that the call factors
        V_b only."""
        known = ktb_logdet[0] is not None and ktb_logdet[0][0] is K_tilde_b
        return elbo_terms(r, f_mean, lambda_m, f_params, m_b, V_b, K_tilde_b, K_tilde_inv_b,
                          logdet_K=ktb_logdet[0][1] if known else None, ignore_warning=ignore_warning,
                          grouped=FULL_RANK_GROUPS or not full_rank())

    def lambda0_and_rate():
        """``lambda0_given_logA`` (:1874, :1934) and, from the same pass over the training points, the rate at that
        ``(logA, lambda0)`` -- what ``mean_f_given_lambda_moments`` is asked for next (:1877, :1958) with the very same
        inputs: the kernel computes both, so the second call (one launch and one wait per E-step) is answered from here."""
        f, out = _fparam_eval(lambda_m, lambda_var, r, f_params['logA'], True)
        rate_cache[0] = (lambda_m, lambda_var, _scalar(f_params['logA']), out[0], f)
        return torch.tensor(out[0], dtype=TORCH_DTYPE)

    def rate_now():
        c = rate_cache[0]
        if (c is not None and c[0] is lambda_m and c[1] is lambda_var and 'loglambda0' not in f_params
                and c[2] == _scalar(f_params['logA']) and c[3] == _scalar(f_params['lambda0'])):
            return c[4]
        return mean_f_given_lambda_moments(f_params, lambda_m, lambda_var)

    def moments_now():
        """lambda moments of the current state (utils.py:1090, 1101); with a = B = I they reduce to
        lambda_m = m, lambda_var = Kvec - diag(K~) + diag(V) and no N^3 product is formed."""
        if _is_identity(B) and ntilde == nt:
            return m_b.clone(), Kvec - torch.diagonal(K_tilde_b) + torch.diagonal(V_b)
        return lambda_moments(x_m, K_tilde_b, KKtilde_inv_b, Kvec, K_b, C, m_b, V_b, theta, kernfun=kernfun)

    if 'init_kernel' not in kwargs:
        C, mask, K_tilde, K, Kvec, x_m = build_kernels(theta)
        eigvecs, B, K_tilde_b, K_tilde_inv_b, K_b, KKtilde_inv_b = project(K_tilde, K)
    else:
        ik = kwargs['init_kernel']
        if ik.get('square') and (ntilde != nt or tuple(ik['K'].shape) != (nt, ntilde)):
            raise ValueError("varGP: this init_kernel was prepared by extend_inducing_set for a training set equal to the "
                             f"grown inducing set ({tuple(ik['K'].shape)[0]} images); got n_t = {nt}, n_tilde = {ntilde}")
        C, mask, K_tilde, K, Kvec = _cu(ik['C']), ik['mask'].to(dev), _cu(ik['K_tilde']), _cu(ik['K']), _cu(ik['Kvec'])
        B, K_tilde_b, K_b, K_tilde_inv_b = _cu(ik['B']), _cu(ik['K_tilde_b']), _cu(ik['K_b']), _cu(ik['K_tilde_inv_b'])
        # an init_kernel prepared by extend_inducing_set says which route built its basis (and brings the factor of
        # K~ when that basis is the identity); one built the notebook's way (eigh + truncation) carries neither
        basis_route[0] = ik.get('basis_route', 'eigh')
        if basis_route[0] == 'identity':
            B = _mark_identity(B)
            if ik.get('chol') is not None:
                chol_factor[0] = (_cu(ik['chol']['L']), _cu(ik['chol']['Linv']))
        KKtilde_inv_b = _cu(ik['KKtilde_inv_b']) if ntilde != nt else B
        x_m = x[:, mask].contiguous()

    m = _cu(copy.deepcopy(kwargs.get('m', torch.zeros(ntilde, dtype=TORCH_DTYPE))).detach())
    V = _cu(copy.deepcopy(kwargs.get('V', K_tilde)).detach())
    V_b = to_basis_mat(B, V) if 'V' in kwargs else K_tilde_b
    m_b = to_basis_vec(B, m)

    import os as _os
    no_fast = bool(_os.environ.get("GPFIT_NO_FAST"))

    def full_rank():
        return (not no_fast) and same_points and B.shape[0] == B.shape[1]

    lambda_m, lambda_var = moments_now()
    f_mean = mean_f_given_lambda_moments(f_params, lambda_m, lambda_var)
    loglikelihood, KL_div = loss_now()
    logmarginal = loglikelihood - KL_div

    loss_track = {k: torch.zeros(maxiter) for k in ('logmarginal', 'loglikelihood', 'KL')}
    theta_track = {key: torch.zeros(maxiter) for key in theta.keys()}
    l0key = 'lambda0' if 'lambda0' in f_params else 'loglambda0'
    f_par_track = {'logA': torch.zeros(maxiter), l0key: torch.zeros(maxiter)}
    values_track = {'loss_track': loss_track, 'theta_track': theta_track, 'f_par_track': f_par_track,
                    'variation_par_track': {'V_b': (), 'm_b': (), 'basis_route': ()}}

    def record(it):
        loss_track['loglikelihood'][it] = _scalar(loglikelihood)
        loss_track['KL'][it] = _scalar(KL_div)
        loss_track['logmarginal'][it] = _scalar(loglikelihood) - _scalar(KL_div)
        for key in theta.keys():
            theta_track[key][it] = _scalar(theta[key])
        f_par_track['logA'][it] = _scalar(f_params['logA'])
        f_par_track[l0key][it] = _scalar(f_params[l0key])
        values_track['variation_par_track']['V_b'] += (V_b.clone(),)
        values_track['variation_par_track']['m_b'] += (m_b.clone(),)
        values_track['variation_par_track']['basis_route'] += (basis_route[0],)

    times = {'estep': 0.0, 'fparams': 0.0, 'mstep': 0.0, 'kernels': 0.0, 'loss': 0.0}
    start_time_loop = time.time()
    iteration = 0
    try:
        record(0)
        print(f'Initial Loss: {-(_scalar(loglikelihood) - _scalar(KL_div)):.4f}')
        for iteration in range(1, maxiter):
            t0 = time.time()
            if nMstep > 0 and iteration > 1:
                # kernels at the theta of the last M-step, new eigenbasis, (m_b, V_b) re-projected
                C, mask, K_tilde, K, Kvec, x_m = build_kernels(theta)                       # utils.py:1803-1806
                B_old = B
                eigvecs, B, K_tilde_b, K_tilde_inv_b, K_b, KKtilde_inv_b = project(K_tilde, K)   # :1808-1818
                if _is_identity(B) and _is_identity(B_old):
                    pass                                      # B^T B_old = I: (m_b, V_b) unchanged
                else:
                    BtB = B_old if _is_identity(B) else (B.T.contiguous() if _is_identity(B_old)
                                                           else matmul(B, B_old, transA=True))
                    V_b = matmul(BtB, matmul(V_b, BtB, transB=True))                       # :1833
                    m_b = matmul(BtB, m_b)                                                 # :1840
            times['kernels'] += time.time() - t0

            t0 = time.time()
            if nEstep > 0:
                if damped_chain:
                    # the nEstep damped updates of this iteration as one device call, in every regime (the full-rank
                    # one with a = KKtilde_inv_b = B, as in the loop below); the preamble and the factor as there
                    if nMstep > 0:
                        lambda_m, lambda_var = moments_now()                                  # :1871
                        f_params['lambda0'] = lambda0_and_rate()                              # :1874
                    f_mean = rate_now()                                                         # :1877
                    if estep_factor[0] is None or estep_factor[0][0] is not K_tilde_b:
                        L_kb, Li_kb, logdet_kb, info_kb = cholesky(K_tilde_b, want_inverse=True)
                        if info_kb != 0:
                            raise torch.linalg.LinAlgError(f"Estep: K_tilde is not positive definite (info={info_kb})")
                        estep_factor[0] = (K_tilde_b, L_kb, matmul(KKtilde_inv_b, L_kb),
                                           Kvec - torch.sum(K_b * KKtilde_inv_b, 1), Li_kb)
                        ktb_logdet[0] = (K_tilde_b, logdet_kb)
                    m_b, V_b, lambda_m, lambda_var, f_fp, chain_rec = _estep_chain_damped(
                        r, KKtilde_inv_b, estep_factor[0][2], estep_factor[0][1], estep_factor[0][4], estep_factor[0][3],
                        V_b, m_b, f_mean, _scalar(f_params['logA']), estep_alpha, nEstep, nFparamstep,
                        lambda_m=lambda_m, lambda_var=lambda_var)
                    # (the full steps' warnings in step order, then what the first failing step raises)
                    last_rec = _estep_chain_damped_commit(chain_rec, f_params, iteration, estep_full_steps)
                    rate_cache[0] = (lambda_m, lambda_var, _scalar(f_params['logA']), last_rec[1], f_fp)
                elif (ESTEP_CHAIN and nEstep <= CHAIN_MAX_STEPS and 'loglambda0' not in f_params and not damped
                        and not full_rank()):
                    # the nEstep updates of this iteration as one device call (the loop below, enqueued in one go).
                    # The host loop stays (silently: the "E-steps" time is then the loop's) for more updates than the
                    # chain's cap, and for f_params carrying loglambda0: the optimiser leaves the rate at the
                    # closed-form lambda0, which is what the next update reads in the chain, while the loop evaluates
                    # it anew at the fixed lambda0 (rate_now, :1877)
                    if nMstep > 0:
                        lambda_m, lambda_var = moments_now()                                  # :1871
                        f_params['lambda0'] = lambda0_and_rate()                              # :1874
                    f_mean = rate_now()                                                         # :1877
                    if estep_factor[0] is None or estep_factor[0][0] is not K_tilde_b:
                        L_kb, _, logdet_kb, info_kb = cholesky(K_tilde_b)
                        if info_kb != 0:
                            raise torch.linalg.LinAlgError(f"Estep: K_tilde is not positive definite (info={info_kb})")
                        estep_factor[0] = (K_tilde_b, L_kb, matmul(KKtilde_inv_b, L_kb),
                                           Kvec - torch.sum(K_b * KKtilde_inv_b, 1))
                        ktb_logdet[0] = (K_tilde_b, logdet_kb)
                    m_b, V_b, lambda_m, lambda_var, f_fp, chain_rec = _estep_chain(
                        r, KKtilde_inv_b, estep_factor[0][2], estep_factor[0][1], estep_factor[0][3], m_b, f_mean,
                        _scalar(f_params['logA']), nEstep, nFparamstep, V=V_b, lambda_m=lambda_m,
                        lambda_var=lambda_var)
                    last_rec = _estep_chain_commit(chain_rec, f_params)     # raises for the first failing step
                    rate_cache[0] = (lambda_m, lambda_var, _scalar(f_params['logA']), last_rec[1], f_fp)
                    # (the rate-parameter share of the call is not separable: times['fparams'] stays as it is)
                elif (ESTEP_CHAIN and nEstep <= CHAIN_MAX_STEPS and 'loglambda0' not in f_params and not damped
                        and full_rank() and _is_identity(B)):
                    # the full-rank regime in the original basis (a = B = I): the loop below around gpfit_estep as one
                    # device call.  A square B that is not the identity (the eigh route keeping everything) keeps the
                    # loop: it rotates by B around every update
                    if nMstep > 0:
                        lambda_m, lambda_var = moments_now()                                  # :1871
                        f_params['lambda0'] = lambda0_and_rate()                              # :1874
                    f_mean = rate_now()                                                         # :1877
                    kv0 = Kvec - torch.diagonal(K_tilde_b)
                    m_b, V_b, lambda_m, lambda_var, f_fp, chain_rec = _estep_chain_full(
                        r, K_tilde, kv0, m_b, f_mean, _scalar(f_params['logA']), nEstep, nFparamstep, V=V_b,
                        lambda_m=lambda_m, lambda_var=lambda_var)
                    last_rec = _estep_chain_full_commit(chain_rec, f_params, f_fp)     # raises for the first failing step
                    rate_cache[0] = (lambda_m, lambda_var, _scalar(f_params['logA']), last_rec[1], f_fp)
                else:
                    for i_estep in range(nEstep):
                        if i_estep == 0 and nMstep > 0:
                            lambda_m, lambda_var = moments_now()                                  # :1871
                            f_params['lambda0'] = lambda0_and_rate()                              # :1874
                        f_mean = rate_now()                                                         # :1877
                        fused_moments = False
                        if full_rank() and not damped:
                            # fused Newton update in the original basis, then back to the eigenbasis
                            m_orig = m_b if _is_identity(B) else matmul(B, m_b)
                            m_new = torch.empty(nt, dtype=TORCH_DTYPE, device=dev)
                            V_new = torch.empty((nt, nt), dtype=TORCH_DTYPE, device=dev)
                            eng = get_engine(nt, 1)
                            rc = _lib.load().gpfit_estep(eng._ctx, _stream(), K_tilde.data_ptr(), K_tilde.stride(0), nt,
                                                         r.data_ptr(), m_orig.data_ptr(), f_mean.data_ptr(),
                                                         _scalar(f_params['logA']), m_new.data_ptr(), V_new.data_ptr(),
                                                         V_new.stride(0))
                            if rc != 0:
                                if not bool(torch.isfinite(f_mean).all()):
                                    # the reference's LU solve lets NaNs through and reports them one step
                                    # later, in the rate-parameter closure (utils.py:1923-1924)
                                    raise ValueError(f'Nan in f_mean during f param update in Estep, closure has been '
                                                     f'called 1 times in estep {i_estep} iteration. Try substituting '
                                                     f'them with inf.')
                                raise torch.linalg.LinAlgError(f"Estep: {_lib.last_error()} (rc={rc})")
                            if _is_identity(B):
                                m_b, V_b = m_new, V_new            # symmetric by construction (gpfit_estep)
                            else:
                                m_b = matmul(B, m_new, transA=True)
                                V_b = matmul(B, matmul(V_new, B), transA=True)
                                V_b = (V_b + V_b.T) / 2
                        else:
                            # :1880, with the factor of K~_b shared by the E-steps of this iteration
                            # (a damped fit comes here in the full-rank regime too, with a = KKtilde_inv_b = B, and
                            # keeps L^-1 beside the factor)
                            if estep_factor[0] is None or estep_factor[0][0] is not K_tilde_b:
                                L_kb, Li_kb, logdet_kb, info_kb = cholesky(K_tilde_b, want_inverse=damped)
                                if info_kb != 0:
                                    raise torch.linalg.LinAlgError(f"Estep: K_tilde is not positive definite (info={info_kb})")
                                estep_factor[0] = (K_tilde_b, L_kb, matmul(KKtilde_inv_b, L_kb),
                                                   Kvec - torch.sum(K_b * KKtilde_inv_b, 1), Li_kb)
                                ktb_logdet[0] = (K_tilde_b, logdet_kb)
                            if damped:
                                # :1432-1436 as one device call; the moments follow separately (moments_now below)
                                try:
                                    m_b, V_b = _estep_projected_damped(r, KKtilde_inv_b, estep_factor[0][2],
                                                                       estep_factor[0][1], estep_factor[0][4], V_b, m_b,
                                                                       f_params, f_mean, estep_alpha)
                                except torch.linalg.LinAlgError as e:
                                    if not str(e).startswith(_V_NOT_POSDEF):
                                        raise
                                    # the V_b reprojected onto a new basis need not be positive definite (reference
                                    # docs.md:26-30, utils.py:1829): this one update takes the full step, which does
                                    # not read V
                                    warnings.warn(_FULL_STEP_WARNING.format(i_estep, iteration))
                                    estep_full_steps[0] += 1
                                    m_b, V_b = _estep_projected(r, KKtilde_inv_b, estep_factor[0][2],
                                                                estep_factor[0][1], m_b, f_params, f_mean)
                            else:
                                # the update and the moments behind it (:1884) in one device call
                                m_b, V_b, lambda_m, lambda_var = _estep_projected(r, KKtilde_inv_b, estep_factor[0][2],
                                                                                  estep_factor[0][1], m_b, f_params,
                                                                                  f_mean, kv0=estep_factor[0][3])
                                fused_moments = True
                        if not fused_moments:
                            lambda_m, lambda_var = moments_now()                                    # :1884
                        # (the reference evaluates the rate here, :1885; nothing reads it before the closure below overwrites it)
                        tf = time.time()
                        # :1892-1934 (lambda0_given_logA, the LBFGS over logA with its closure, lambda0_and_rate) in one
                        # device call; the rate it leaves is the one rate_now() is asked for next
                        f_fp, lambda0_fp = _fparam_lbfgs(lambda_m, lambda_var, r, f_params, nFparamstep, i_estep)
                        rate_cache[0] = (lambda_m, lambda_var, _scalar(f_params['logA']), lambda0_fp, f_fp)
                        times['fparams'] += time.time() - tf
            else:
                print('No E-step')
            times['estep'] += time.time() - t0

            t0 = time.time()
            f_mean = rate_now()                                                                             # :1958
            loglikelihood, KL_div = loss_now()
            logmarginal = loglikelihood - KL_div
            times['loss'] += time.time() - t0
            record(iteration)
            print(f'Loss iter {iteration}: {-(_scalar(loglikelihood) - _scalar(KL_div)):.4f}')

            t0 = time.time()
            if nMstep > 0 and iteration < maxiter - 1:
                opt_h = torch.optim.LBFGS(theta.values(), lr=0.1, max_iter=nMstep, line_search_fn='strong_wolfe',
                                          tolerance_change=1.e-9, tolerance_grad=1.e-7, history_size=100)     # :2013
                fast = full_rank()
                if fast:
                    # (m, V) are fixed during the M-step: go to the original basis once
                    if _is_identity(B):
                        m_orig, V_orig = m_b, V_b
                    else:
                        m_orig = matmul(B, m_b)
                        V_orig = matmul(B, matmul(V_b, B, transB=True))
                        V_orig = (V_orig + V_orig.T) * 0.5
                mcalls = [0]
                v_factored = [False]

                def closure_hyperparams():
                    mcalls[0] += 1
                    opt_h.zero_grad()
                    outside = False
                    for key, value in theta.items():                                                       # :2022-2028
                        if not (theta_lower_lims[key] <= _scalar(value) <= theta_higher_lims[key]):
                            outside = True
                            print(f"{key} = {_scalar(value):.4f} is not within the limits of {theta_lower_lims[key]} and "
                                  f"{theta_higher_lims[key]}, returning inifinite loss in closure call {mcalls[0]}")
                            if theta[key].requires_grad:
                                theta[key].grad = torch.tensor(float('inf'))
                    if outside:
                        return torch.tensor(float('inf'))
                    if fast:
                        res = _closure_full(theta, lims, n_px_side, x, r, m_orig, V_orig, f_params, v_factored[0])
                        v_factored[0] = True  # V is constant for the rest of this M-step
                        loss, grad = res['loss'], res['grad']
                    elif same_points and not no_fast:
                        loss, grad = _closure_projected(theta, lims, n_px_side, x, r, B, m_b, V_b, f_params)
                    elif ntilde != nt and not no_fast:
                        loss, grad = _closure_sparse(theta, lims, n_px_side, x, xtilde, r, B, m_b, V_b, f_params)
                    else:
                        loss, grad = _closure_general(theta, lims, n_px_side, x, xtilde, r, B, m_b, V_b, f_params,
                                                      ntilde, nt)
                    for key in theta.keys():
                        if theta[key].requires_grad:
                            theta[key].grad = torch.tensor(grad[key], dtype=TORCH_DTYPE)                       # :2098-2099
                    return torch.tensor(loss, dtype=TORCH_DTYPE)

                opt_h.step(closure_hyperparams)                                                             # :2114
            elif iteration < maxiter - 1:
                print(' No M-step')
            times['mstep'] += time.time() - t0

    except (KeyboardInterrupt, Exception) as e:  # utils.py:2127-2189: roll back to the last tracked state
        print(f' ===================  Error During iteration: {iteration} =================== \n')
        fit_parameters['maxiter'] = iteration
        err_dict['is_error'] = True
        err_dict['error'] = e
        err_dict['error_message'] = repr(e)
        if iteration <= 1:
            # utils.py:2134-2138 / 2168-2172 re-raise here, but the `return` inside the reference's
            # `finally` block (utils.py:2316) swallows that exception: what the caller observes is the
            # current (not rolled-back) state with err_dict set.  Reproduced as observed.
            print('Too few iterations iterations were done to save')
        else:
            theta = {k: theta_track[k][iteration - 1].to(TORCH_DTYPE) for k in theta.keys()}
            f_params['logA'] = f_par_track['logA'][iteration - 1].to(TORCH_DTYPE)
            f_params[l0key] = f_par_track[l0key][iteration - 1].to(TORCH_DTYPE)
            V_b = values_track['variation_par_track']['V_b'][iteration - 1]
            m_b = values_track['variation_par_track']['m_b'][iteration - 1]
        # utils.py:2194-2231 (the `finally` block when is_error): kernels at the theta in force, final loss
        C, mask, K_tilde, K, Kvec, x_m = build_kernels(theta)
        eigvecs, B, K_tilde_b, K_tilde_inv_b, K_b, KKtilde_inv_b = project(K_tilde, K)
        lambda_m, lambda_var = moments_now()
        f_mean = mean_f_given_lambda_moments(f_params, lambda_m, lambda_var)
        loglikelihood, KL_div = loss_now(ignore_warning=False)
        logmarginal = loglikelihood - KL_div
        last = fit_parameters['maxiter'] - 1
        loss_track['loglikelihood'][last] = _scalar(loglikelihood)
        loss_track['KL'][last] = _scalar(KL_div)
        loss_track['logmarginal'][last] = _scalar(logmarginal)

    if fit_parameters.get('full_eigvecs', False) and (eigvecs is None or eigvecs.shape[1] != eigvecs.shape[0]):
        eigvecs = torch.linalg.eigh(K_tilde, UPLO='L')[1]     # the reference's N x N matrix, on request (utils.py:2241)
    final_kernel = {'C': C, 'mask': mask, 'K_tilde': K_tilde, 'K': K, 'Kvec': Kvec, 'eigvecs': eigvecs}
    # the factor of the final K~ (identity route only; two more n~ x n~ matrices, so by default only up to the sizes
    # of the closed-loop experiments): what extend_inducing_set grows by one row instead of refactorising
    if chol_factor[0] is not None and fit_parameters.get('keep_factor', ntilde <= 4096):
        final_kernel['chol'] = {'L': chol_factor[0][0], 'Linv': chol_factor[0][1]}
    if not is_simmetric(V_b, 'V_b'):
        print('Final V_b is not simmetric, maximum difference: ', torch.max(torch.abs(V_b - V_b.T)))
        V_b = (V_b + V_b.T) / 2
    if not is_posdef(V_b, 'V_b'):
        print('Final V_b is not posdef, this should not be possible if you are skipping the last M-step')
        V_b = V_b + torch.eye(V_b.shape[0], dtype=TORCH_DTYPE, device=V_b.device) * EIGVAL_TOL

    print(f'\nTime spent for E-steps:       {times["estep"]:.3f}s,')
    print(f'Time spent for f params:      {times["fparams"]:.3f}s')
    print(f'Time spent for m / V update:  {times["estep"] - times["fparams"]:.3f}s')
    print(f'Time spent for M-steps:       {times["mstep"]:.3f}s')
    print(f'Time spent for All-steps:     {times["estep"] + times["mstep"]:.3f}s')
    print(f'Time spent computing Kernels: {times["kernels"]:.3f}s')
    print(f'Time spent computing Loss:    {times["loss"]:.3f}s')
    print(f'\nTime total after init:        {time.time() - start_time_loop:.3f}s')
    print(f'Time total before init:       {time.time() - start_time_before_init:.3f}s')
    print(f'Final Loss: {-_scalar(logmarginal):.4f}')

    nkeep = fit_parameters['maxiter']
    for key in values_track.keys():
        for sub in values_track[key].keys():
            values_track[key][sub] = values_track[key][sub][:nkeep]

    fit_model = {
        'fit_parameters': fit_parameters, 'final_kernel': final_kernel, 'err_dict': err_dict, 'xtilde': xtilde,
        'hyperparams_tuple': (theta, theta_lower_lims, theta_higher_lims), 'f_params': f_params, 'm_b': m_b,
        'V_b': V_b, 'C': C, 'mask': mask, 'K_tilde_b': K_tilde_b, 'K_tilde_inv_b': K_tilde_inv_b, 'K_b': K_b,
        'Kvec': Kvec, 'B': B, 'values_track': values_track, 'basis_route': basis_route[0],
    }
    if damped:
        fit_model['estep_full_steps'] = int(estep_full_steps[0])
    return fit_model, err_dict


@torch.no_grad()
def test(X_test, R_test, xtilde, X_train=None, at_iteration=None, **kwargs):
    """Predict the firing rate of one cell on test images from a ``fit_model`` (utils.py:326-412):
    ``test(X_test, R_test, X_train=X, at_iteration=None, **fit_model)``.  X_test is
    [n_images, n_px, n_px, 1]; all images go through ``lambda_moments_star`` in one batch."""
    fp = kwargs['fit_parameters']
    maxiter, nEstep, nMstep = fp.get('maxiter', 0), fp.get('nEstep', 0), fp.get('nMstep', 0)
    cellid, n_px_side = fp.get('cellid'), fp.get('n_px_side')
    mask, C = kwargs.get('mask'), kwargs.get('C')
    theta, theta_lower_lims, theta_higher_lims = kwargs.get('hyperparams_tuple')
    m, V, B = kwargs.get('m_b'), kwargs.get('V_b'), kwargs.get('B')
    K_tilde, K_tilde_inv = kwargs.get('K_tilde_b'), kwargs.get('K_tilde_inv_b')
    f_params = kwargs.get('f_params')
    xtilde = _cu(xtilde)
    reserve(xtilde.shape[0], xtilde.shape[1], xtilde.shape[1])
    A = math.exp(_scalar(f_params['logA']))
    lambda0 = _scalar(_lambda0_of(f_params))

    if at_iteration is not None and X_train is not None:                                   # utils.py:358-386
        vt = kwargs['values_track']
        theta = {key: val[at_iteration] for key, val in vt['theta_track'].items()}
        m = vt['variation_par_track']['m_b'][at_iteration]
        V = vt['variation_par_track']['V_b'][at_iteration]
        A = math.exp(_scalar(vt['f_par_track']['logA'][at_iteration]))
        lambda0 = (_scalar(vt['f_par_track']['lambda0'][at_iteration]) if 'lambda0' in vt['f_par_track']
                   else math.exp(_scalar(vt['f_par_track']['loglambda0'][at_iteration])))
        C, mask = localker(theta=theta, theta_higher_lims=theta_higher_lims, theta_lower_lims=theta_lower_lims,
                           n_px_side=n_px_side, grad=False)
        xt_m = xtilde[:, mask].contiguous()
        Kt = acosker(theta, xt_m, xt_m, C=C, diag=False)
        routes = vt['variation_par_track'].get('basis_route')     # absent in a dict the reference itself produced
        _, B, K_tilde, K_tilde_inv = _stabilised_basis(Kt, route=routes[at_iteration] if routes else None)

    X_test = _cu(X_test)
    n_img = X_test.shape[0]
    xstar = X_test.reshape(n_img, -1)                                                      # utils.py:389-390
    mask = mask.to(xstar.device)
    mu_star, sigma_star2 = lambda_moments_star(xstar[:, mask].contiguous(), xtilde[:, mask].contiguous(), C, theta,
                                               K_tilde, K_tilde_inv, m, V, B, 'acosker')   # :393
    R_predicted = torch.exp(A * mu_star + 0.5 * A * A * sigma_star2 + lambda0)              # :395
    R_test = _cu(R_test)
    r2, sigma_r2 = explained_variance(R_test[:, :, cellid], R_predicted, sigma=True)        # :400
    print(f"\n\n Pietro's model: R2 = {float(r2):.2f} ± {float(sigma_r2):.2f} Cell: {cellid} maxiter = {maxiter}, "
          f"nEstep = {nEstep}, nMstep = {nMstep} \n")
    return R_test[:, :, cellid], R_predicted, r2, sigma_r2
