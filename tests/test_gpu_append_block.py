"""Block append of the Cholesky factor (gpfit_potrf_append_block behind utils.cholesky_append_block) and the closed-loop
round built on it (utils.extend_inducing_set with several images).  The reference is torch.linalg.cholesky /
torch.logdet of the whole grown matrix in float64; the tolerances are the ones test_cholesky_rank1_append applies to the
same quantities on the same matrix classes (the same algorithm in numpy stays at 1e-14 or below on these inputs: two
orders of margin and more for the order of summation)."""
import contextlib
import functools
import io
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden, relerr
from gaussian_processes_amd import synthetic as syn

pytestmark = pytest.mark.gpu
KEYS = syn.THETA_KEYS
LOWER, UPPER = syn.limits()
TOL_L, TOL_LINV, TOL_LOGDET = 1e-12, 1e-10, 1e-11


def T(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).cuda()


@pytest.fixture(scope="module")
def gp():
    from gaussian_processes_amd import utils
    return utils


@functools.lru_cache(maxsize=None)
def randn_case(n0, k):
    """S = M M^T + N I, its reference factor and log-det, and the factor of the leading n0 x n0 block (never modified)."""
    from gaussian_processes_amd import utils as gp
    N = n0 + k
    M = torch.randn(N, N, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    S = (M @ M.T + N * torch.eye(N, dtype=torch.float64)).cuda()
    return _case(gp, S, n0)


@functools.lru_cache(maxsize=None)
def gram_case(n0, k):
    """The kernel matrix of the real workload: acosker on synthetic stimuli at theta0, 8 x 8 pixels, masked."""
    from gaussian_processes_amd import utils as gp
    th = {key: torch.tensor(float(syn.theta0()[key]), dtype=torch.float64, requires_grad=True) for key in KEYS}
    C, mask = gp.localker(th, UPPER, LOWER, 8)
    X = T(syn.stimuli(n0 + k, 64))[:, mask.to("cuda")].contiguous()
    K = gp.acosker(th, X, X, C=C)
    return _case(gp, ((K + K.T) * 0.5).contiguous(), n0)


def _case(gp, S, n0):
    L0, Li0, logdet0, info = gp.cholesky(S[:n0, :n0].contiguous(), want_inverse=True)
    assert info == 0
    return {"S": S, "n0": n0, "k": S.shape[0] - n0, "L0": L0, "Li0": Li0, "logdet0": logdet0,
            "Lref": torch.linalg.cholesky(S), "logdet_ref": float(torch.logdet(S))}


def embedded(c):
    N = c["n0"] + c["k"]
    L = torch.zeros((N, N), dtype=torch.float64, device="cuda")
    Li = torch.zeros_like(L)
    L[:c["n0"], :c["n0"]], Li[:c["n0"], :c["n0"]] = c["L0"], c["Li0"]
    return L, Li


def check_against_reference(c, L, Li, logdet, rows=None):
    """The three assertions on the leading rows x rows block (default: the whole grown matrix)."""
    N = L.shape[0] if rows is None else rows
    Lref = c["Lref"][:N, :N]
    eL = relerr(L[:N, :N].cpu().numpy(), Lref.cpu().numpy())
    eI = relerr((Li[:N, :N] @ Lref).cpu().numpy(), np.eye(N))
    ref_logdet = c["logdet_ref"] if rows is None else 2.0 * float(torch.log(torch.diagonal(Lref)).sum())
    eD = abs(logdet - ref_logdet) / abs(ref_logdet)
    print(f"n0 {c['n0']} k {c['k']} rows {N}: L {eL:.2e}  Linv Lref - I {eI:.2e}  logdet {eD:.2e}")
    assert eL < TOL_L
    assert eI < TOL_LINV
    assert eD < TOL_LOGDET


def assert_strictly_lower(L, Li):
    assert int(torch.count_nonzero(torch.triu(L, 1))) == 0
    assert int(torch.count_nonzero(torch.triu(Li, 1))) == 0


@pytest.mark.parametrize("n0,k", [(1, 1), (100, 3), (257, 127), (1000, 5), (1000, 128), (1000, 130), (384, 300)])
def test_block_append_randn(gp, n0, k):
    """(a) ragged n against every slab and tile size, k = 1, k = 128 exactly, k just past a chunk and several chunks."""
    c = randn_case(n0, k)
    L, Li = embedded(c)
    logdet, info = gp.cholesky_append_block(L, Li, c["S"][:, n0:].contiguous(), c["logdet0"])
    assert info == 0
    check_against_reference(c, L, Li, logdet)
    assert_strictly_lower(L, Li)


@pytest.mark.parametrize("n0,k", [(300, 40), (700, 64)])
def test_block_append_kernel_matrices(gp, n0, k):
    """(b) the matrices the closed loop grows (condition numbers 5e3 and 2e4)."""
    c = gram_case(n0, k)
    L, Li = embedded(c)
    logdet, info = gp.cholesky_append_block(L, Li, c["S"][:, n0:].contiguous(), c["logdet0"])
    assert info == 0
    check_against_reference(c, L, Li, logdet)
    assert_strictly_lower(L, Li)


def test_block_and_rank1_paths_both_meet_the_reference(gp):
    """(c) k successive cholesky_append calls and one block call on (1000, 5): not bit-equal, both within tolerance."""
    c = randn_case(1000, 5)
    n0, k, S = c["n0"], c["k"], c["S"]
    L1, Li1 = embedded(c)
    logdet1 = c["logdet0"]
    for j in range(k):
        nn = n0 + j
        logdet1, info = gp.cholesky_append(L1[:nn + 1, :nn + 1], Li1[:nn + 1, :nn + 1], S[:nn + 1, nn].contiguous(), logdet1)
        assert info == 0
    Lb, Lib = embedded(c)
    logdetb, info = gp.cholesky_append_block(Lb, Lib, S[:, n0:].contiguous(), c["logdet0"])
    assert info == 0
    check_against_reference(c, L1, Li1, logdet1)
    check_against_reference(c, Lb, Lib, logdetb)


def test_block_append_is_deterministic(gp):
    """(d) no floating-point atomics: the same call on fresh copies gives the same bits."""
    c = randn_case(1000, 128)
    cols = c["S"][:, c["n0"]:].contiguous()
    out = []
    for _ in range(2):
        L, Li = embedded(c)
        logdet, info = gp.cholesky_append_block(L, Li, cols, c["logdet0"])
        assert info == 0
        out.append((L, Li, logdet))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


def test_block_append_reports_the_pivot_in_the_grown_matrix(gp):
    """(e) a non-positive pivot: info counts in the grown matrix, the leading blocks and the log-det stay as they were;
    in the second chunk of a k = 130 call the rows of the first chunk are valid."""
    c = randn_case(1000, 5)
    n0 = c["n0"]
    cols = c["S"][:, n0:].clone()
    cols[n0 + 3, 3] = -1.0
    L, Li = embedded(c)
    logdet, info = gp.cholesky_append_block(L, Li, cols, c["logdet0"])
    assert info == n0 + 4
    assert torch.equal(L[:n0, :n0], c["L0"]) and torch.equal(Li[:n0, :n0], c["Li0"])
    assert logdet == c["logdet0"]
    c = randn_case(1000, 130)
    cols = c["S"][:, n0:].clone()
    cols[n0 + 129, 129] = -1.0
    L, Li = embedded(c)
    logdet, info = gp.cholesky_append_block(L, Li, cols, c["logdet0"])
    assert info == n0 + 130
    assert torch.equal(L[:n0, :n0], c["L0"]) and torch.equal(Li[:n0, :n0], c["Li0"])
    check_against_reference(c, L, Li, logdet, rows=n0 + 128)


def test_nothing_above_the_diagonal_of_the_factors_is_read(gp):
    """(g) (257, 17): with NaN in the strict upper triangle of the leading n0 x n0 blocks of both factors, the block call
    and the rank-1 call return, on and below the diagonal, the bits they return with zeros there -- the claim of
    skinny.hip's header ("what lies beyond the diagonal is never used") and what the rank-1 path's two triangular
    matrix-vector kernels index."""
    c = randn_case(257, 17)
    n0, k, S = c["n0"], c["k"], c["S"]
    above = torch.triu(torch.ones((n0, n0), dtype=torch.bool, device="cuda"), 1)
    bits = lambda X: torch.tril(X).view(torch.int64)

    def start(rows, fill):
        L, Li = embedded(c)
        L[:n0, :n0][above] = fill
        Li[:n0, :n0][above] = fill
        return L[:rows, :rows].contiguous(), Li[:rows, :rows].contiguous()

    out = {}
    for fill in (0.0, float("nan")):
        L, Li = start(n0 + k, fill)
        logdet, info = gp.cholesky_append_block(L, Li, S[:, n0:].contiguous(), c["logdet0"])
        assert info == 0
        L1, Li1 = start(n0 + 1, fill)
        logdet1, info = gp.cholesky_append(L1, Li1, S[:n0 + 1, n0].contiguous(), c["logdet0"])
        assert info == 0
        out[fill == 0.0] = (bits(L), bits(Li), logdet, bits(L1), bits(Li1), logdet1)
    zeros, nans = out[True], out[False]
    for a, b in zip(zeros, nans):
        assert torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b
    assert not bool(torch.isnan(torch.tril(L)).any()) and not bool(torch.isnan(torch.tril(Li)).any())
    check_against_reference(c, torch.tril(L), torch.tril(Li), logdet)


# ---------------------------------------------------------------- (f) extend_inducing_set on fixture g9
def quiet():
    stack = contextlib.ExitStack()
    stack.enter_context(contextlib.redirect_stdout(io.StringIO()))
    w = stack.enter_context(warnings.catch_warnings())
    warnings.simplefilter("ignore")
    return stack


@pytest.fixture(scope="module")
def loop(gp):
    """The start fit of test_closed_loop_step_matches_reference: 48 images, the same settings."""
    g = load_golden("g9_active_step.npz")
    images, spikes = T(g["X"]), T(g["R"])
    n0 = int(g["n_start"])
    settings = {"ntilde": n0, "maxiter": int(g["maxiter"]), "nEstep": 2, "nMstep": 3, "nFparamstep": 3, "kernfun": "acosker",
                "cellid": 0, "n_px_side": 8, "display_hyper": False}
    theta = {k: torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for k, v in syn.theta0().items()}
    link = {"logA": torch.tensor(syn.F_PARAMS["logA"]), "lambda0": torch.tensor(syn.F_PARAMS["lambda0"])}
    with quiet():
        first, err = gp.varGP(images[:n0], spikes[:n0], fit_parameters=settings, xtilde=images[:n0],
                              hyperparams_tuple=(theta, LOWER, UPPER), f_params=link)
    assert not err["is_error"], err
    assert first["basis_route"] == "identity" and first["final_kernel"].get("chol") is not None
    bare = dict(first)
    bare["final_kernel"] = {k: v for k, v in first["final_kernel"].items() if k != "chol"}
    return {"images": images, "spikes": spikes, "n0": n0, "first": first, "bare": bare}


def count_calls(gp, monkeypatch):
    calls = {"rank1": 0, "block": 0}
    one, blk = gp.cholesky_append, gp.cholesky_append_block

    def rank1(*a, **kw):
        calls["rank1"] += 1
        return one(*a, **kw)

    def block(*a, **kw):
        calls["block"] += 1
        return blk(*a, **kw)

    monkeypatch.setattr(gp, "cholesky_append", rank1)
    monkeypatch.setattr(gp, "cholesky_append_block", block)
    return calls


def test_extend_by_eight_images_in_one_call(gp, loop, monkeypatch):
    images, spikes, n0, first = loop["images"], loop["spikes"], loop["n0"], loop["first"]
    k = 8
    calls = count_calls(gp, monkeypatch)
    grown = gp.extend_inducing_set(first, images[n0:n0 + k])
    assert calls == {"rank1": 0, "block": 1}
    ik = grown["init_kernel"]
    assert ik["basis_route"] == "identity" and ik["chol"] is not None
    th, px = first["hyperparams_tuple"][0], first["mask"].to("cuda")
    xm = images[:n0 + k][:, px].contiguous()
    assert relerr(ik["K_tilde"].cpu().numpy(), gp.acosker(th, xm, xm, C=first["C"]).cpu().numpy()) < 1e-12
    assert torch.equal(ik["K_tilde"][n0:, :], ik["K_tilde"][:, n0:].T)      # the new rows mirror the new columns
    L_ref, Li_ref, _, info = gp.cholesky(ik["K_tilde"], want_inverse=True)
    assert info == 0
    assert relerr(ik["chol"]["L"].cpu().numpy(), L_ref.cpu().numpy()) < 1e-12
    assert relerr(ik["chol"]["Linv"].cpu().numpy(), Li_ref.cpu().numpy()) < 1e-10
    # m, V, xtilde by their definitions
    m_old, V_old = first["m_b"].cuda(), first["V_b"].cuda()
    assert torch.equal(grown["m"], torch.cat((m_old, m_old.mean().reshape(1).expand(k))))
    V_def = torch.eye(n0 + k, dtype=torch.float64, device="cuda")
    V_def[:n0, :n0] = (V_old + V_old.T) * 0.5
    assert torch.equal(grown["V"], V_def)
    assert torch.equal(grown["xtilde"], images[:n0 + k])
    assert ik["Kvec"].shape[0] == n0 + k and ik["B"].shape == (n0 + k, n0 + k)
    # the same step without the stored factor
    slow = gp.extend_inducing_set(loop["bare"], images[n0:n0 + k])
    assert calls == {"rank1": 0, "block": 1}
    sk = slow["init_kernel"]
    assert sk["basis_route"] == "identity" and torch.equal(sk["K_tilde"], ik["K_tilde"])
    assert relerr(sk["K_tilde_inv_b"].cpu().numpy(), ik["K_tilde_inv_b"].cpu().numpy()) < 1e-9
    # both preparations refit, and to the same track
    again = dict(first["fit_parameters"], ntilde=n0 + k)
    tracks = []
    for prep in (grown, slow):
        with quiet():
            second, err = gp.varGP(images[:n0 + k], spikes[:n0 + k], fit_parameters=again, xtilde=prep["xtilde"],
                                   hyperparams_tuple=first["hyperparams_tuple"], f_params=first["f_params"], m=prep["m"],
                                   V=prep["V"], init_kernel=prep["init_kernel"])
        assert not err["is_error"], err
        tracks.append(second["values_track"]["loss_track"]["logmarginal"].numpy())
    assert relerr(tracks[0], tracks[1]) < 1e-5


def test_extend_by_all_remaining_images_falls_back(gp, loop, monkeypatch):
    """At 110 images the bounds of the all-kept proof no longer hold on the grown factor: the general route decides."""
    images, n0, first = loop["images"], loop["n0"], loop["first"]
    calls = count_calls(gp, monkeypatch)
    grown = gp.extend_inducing_set(first, images[n0:])
    assert calls == {"rank1": 0, "block": 1}
    slow = gp.extend_inducing_set(loop["bare"], images[n0:])
    gk, sk = grown["init_kernel"], slow["init_kernel"]
    assert gk["K_tilde"].shape[0] == images.shape[0]
    assert gk["basis_route"] == sk["basis_route"] and torch.equal(gk["K_tilde"], sk["K_tilde"])
    assert relerr(gk["K_tilde_inv_b"].cpu().numpy(), sk["K_tilde_inv_b"].cpu().numpy()) < 1e-9


def test_one_image_keeps_the_rank1_path(gp, loop, monkeypatch):
    images, n0, first = loop["images"], loop["n0"], loop["first"]
    calls = count_calls(gp, monkeypatch)
    grown = gp.extend_inducing_set(first, images[n0])
    assert calls == {"rank1": 1, "block": 0}
    ik = grown["init_kernel"]
    # the parent's step by hand: the factor embedded in zeros, one row from the latest column
    L = torch.zeros((n0 + 1, n0 + 1), dtype=torch.float64, device="cuda")
    Li = torch.zeros_like(L)
    L[:n0, :n0], Li[:n0, :n0] = first["final_kernel"]["chol"]["L"].cuda(), first["final_kernel"]["chol"]["Linv"].cuda()
    _, info = gp.cholesky_append(L, Li, ik["K_tilde"][:, n0].contiguous())
    assert info == 0 and torch.equal(ik["chol"]["L"], L) and torch.equal(ik["chol"]["Linv"], Li)
    assert torch.equal(grown["m"], torch.cat((first["m_b"].cuda(), first["m_b"].cuda().mean().reshape(1))))
    assert torch.equal(grown["xtilde"], images[:n0 + 1])
    with pytest.raises(ValueError, match="extend_inducing_set"):
        gp.extend_inducing_set(first, images[n0, :-1])
