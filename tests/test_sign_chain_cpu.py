"""The projector step of ``eigtop._kept_subspace`` by stretches (``sign_chain=``), on torch stand-ins (no GPU): with a hook
that restates the step list of ``gpfit_sign_steps`` (include/gpfit_mi355x.h) in torch, the hooked path must make the
decisions of the host loop and return its bits; and the host side of the group call and of the wave's request kinds."""
import math

import pytest
import torch

from gaussian_processes_amd import eigtop
from gaussian_processes_amd import utils as gp
from test_eigtop_cpu import cpu_cholesky, cpu_matmul

TOL, TAU = 1e-4, 1e-2                     # lambda_max = 100: tau = lambda_max * TOL
SIZES = (48, 160, 256)
# relative distance of the nearest eigenvalue from the threshold -> sign iterations of the host loop (at every k): the 11
# scaled steps from _SIGN_L0 and a failed test, then what the straggler needs
ITERATIONS = {1.0: 12, 4e-4: 15, 1e-5: 21}
KEYS = ("B", "U", "K_tilde_b", "K_tilde_inv_b")


def cpu_gemm_into(C, A, B, alpha=1.0, beta=0.0):
    return C.addmm_(A, B, beta=beta, alpha=alpha)


def gap_spectrum(k, rel, negative=False):
    """k / 4 eigenvalues above the threshold -- logspace(2, 0) and one at tau (1 + rel) -- and the rest far below it,
    logspace(-4, -6); ``negative``: the smallest of them moved to -2 tau (S + tau I is then indefinite)."""
    top = k // 4 - 1
    lam = torch.cat([torch.logspace(2, 0, top, dtype=torch.float64), torch.tensor([TAU * (1.0 + rel)], dtype=torch.float64),
                     torch.logspace(-4, -6, k - top - 1, dtype=torch.float64)])
    if negative:
        lam[-1] = -2.0 * TAU
    return lam


def gap_matrix(k, rel, seed=0, negative=False, scale=1.0):
    """S = Q diag(lambda) Q^T, exactly symmetric; ``scale`` multiplies the spectrum (a unit's own tau)."""
    g = torch.Generator().manual_seed(1000 * k + seed)
    Q, _ = torch.linalg.qr(torch.randn(k, k, dtype=torch.float64, generator=g))
    S = (Q * (scale * gap_spectrum(k, rel, negative))) @ Q.T
    return (S + S.T) * 0.5


class TorchSignHook:
    """The step list of ``gpfit_sign_steps`` restated on ``matmul`` / ``cholesky`` / ``gemm_into`` (the stand-ins by
    default), recording what it was asked for."""

    def __init__(self, matmul=cpu_matmul, cholesky=cpu_cholesky, gemm_into=cpu_gemm_into):
        self.matmul, self.cholesky, self.gemm_into = matmul, cholesky, gemm_into
        self.calls = []

    def __call__(self, S, tau, X, X2, cs, its0):
        self.calls.append({"head": X is None, "x2_ready": X2 is not None, "steps": len(cs), "its0": its0, "cs": list(cs)})
        eye = torch.eye(S.shape[0], device=S.device, dtype=S.dtype)
        if X is None:
            assert X2 is None
            _, Li, _, info = self.cholesky(S + tau * eye, want_inverse=True)
            if info != 0:
                return None
            Sinv = self.matmul(Li, Li, transA=True)
            X = self.matmul(S - tau * eye, Sinv)
            X = (X + X.T) * 0.5
        ready = X2 is not None
        for j, c in enumerate(cs):
            if not (j == 0 and ready):
                X2 = self.matmul(X, X)
            Xn = X.clone()
            self.gemm_into(Xn, X, X2, alpha=-0.5 * c ** 3, beta=1.5 * c)
            X = Xn
            if ((its0 + j) & 7) == 7:
                X = (X + X.T) * 0.5
        return X, self.matmul(X, X)


def kept(S, hook=None, gemm_into=cpu_gemm_into):
    return eigtop._kept_subspace(None, None, S, TOL, 0.0, cpu_matmul, cpu_cholesky, 1e-7, gemm_into=gemm_into, sign_chain=hook)


def assert_same_result(a, b):
    assert a is not None and b is not None
    assert a["n"] == b["n"] and a["sign_iterations"] == b["sign_iterations"]
    for key in KEYS:
        assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize("k", SIZES)
@pytest.mark.parametrize("rel", sorted(ITERATIONS))
def test_hooked_path_has_the_bits_and_the_decisions_of_the_loop(k, rel):
    S = gap_matrix(k, rel)
    loop = kept(S)
    assert loop is not None and loop["n"] == k // 4 and loop["sign_iterations"] == ITERATIONS[rel]
    plain = kept(S, gemm_into=None)                      # (the branch without gemm_into: the same decisions)
    assert plain is not None and plain["n"] == k // 4 and plain["sign_iterations"] == ITERATIONS[rel]
    hook = TorchSignHook()
    assert_same_result(kept(S, hook), loop)
    calls = hook.calls
    assert sum(c["steps"] for c in calls) == ITERATIONS[rel]
    assert calls[0] == {"head": True, "x2_ready": False, "steps": 11, "its0": 0, "cs": eigtop._sign_schedule(eigtop._SIGN_L0, 0, 40)[0]}
    its = 11
    for c in calls[1:]:
        assert not c["head"] and c["x2_ready"] and c["its0"] == its and c["steps"] >= 1
        its += c["steps"]
    # without gemm_into, with the plain iteration and for a k that is no multiple of 16 the hook is never asked
    idle = TorchSignHook()
    assert kept(S, idle, gemm_into=None)["sign_iterations"] == ITERATIONS[rel] and not idle.calls
    eigtop._kept_subspace(None, None, S, TOL, 0.0, cpu_matmul, cpu_cholesky, 1e-7, gemm_into=cpu_gemm_into, scaled=False,
                          sign_chain=idle)
    assert not idle.calls


def test_hook_is_not_asked_for_a_width_that_is_no_multiple_of_16():
    lam = torch.cat([torch.logspace(2, 0, 12, dtype=torch.float64), torch.logspace(-4, -6, 38, dtype=torch.float64)])
    Q, _ = torch.linalg.qr(torch.randn(50, 50, dtype=torch.float64, generator=torch.Generator().manual_seed(5)))
    S = (Q * lam) @ Q.T
    S = (S + S.T) * 0.5
    idle = TorchSignHook()
    out = kept(S, idle)
    assert out is not None and out["n"] == 12 and not idle.calls


def test_both_paths_give_up_at_the_cap():
    """An eigenvalue within 1e-11 of the threshold: the loop runs into its cap of 40 iterations and declines; so does the
    hooked path, having asked for no more than 40 steps."""
    S = gap_matrix(48, 1e-11)
    assert kept(S) is None
    hook = TorchSignHook()
    assert kept(S, hook) is None
    assert hook.calls[0]["head"] and sum(c["steps"] for c in hook.calls) <= 40
    assert all(c["its0"] + c["steps"] <= 40 for c in hook.calls)


def test_both_paths_decline_an_indefinite_head():
    S = gap_matrix(48, 1.0, negative=True)
    assert kept(S) is None
    hook = TorchSignHook()
    assert kept(S, hook) is None
    assert len(hook.calls) == 1 and hook.calls[0]["head"]


def test_sign_schedule_is_the_recurrence_of_the_loop():
    cs, lo_after = eigtop._sign_schedule(eigtop._SIGN_L0, 0, 40)
    assert len(cs) == 11 and round(cs[0], 4) == 1.7312 and round(cs[-1], 4) == 1.0 and lo_after > 1.0 - 1e-9
    # the loop's own lines, from its start and from the figures a failed test resumes with
    for lo0, its0, cap in ((eigtop._SIGN_L0, 0, 40), (0.1, 11, 40), (math.sqrt(1.0 - 0.3), 12, 40), (1.0 - 1e-12, 20, 40),
                           (1e-9, 30, 40), (1e-3, 39, 40), (0.5, 40, 40)):
        lo, its, want, first = lo0, its0, [], True
        while its < cap:
            if lo > 1.0 - 1e-9 and not first:
                break                                     # (the loop tests here)
            first = False
            c = math.sqrt(3.0 / (1.0 + lo + lo * lo)) if lo < 1.0 else 1.0
            want.append(c)
            lo = min(1.0, 0.5 * c * lo * (3.0 - c * c * lo * lo))
            its += 1
        assert eigtop._sign_schedule(lo0, its0, cap) == (want, lo)
        assert its0 + len(want) <= cap


def test_group_refuses_bad_lists_before_any_call(monkeypatch):
    called = []
    monkeypatch.setitem(gp._REQUEST_KINDS, ("sign", None), gp._REQUEST_KINDS["sign", None]._replace(
        batch=lambda *a, **k: called.append("batch")))
    monkeypatch.setattr(gp, "_sign_prepare", lambda *a, **k: called.append("prepare"))
    monkeypatch.setattr(gp, "_group_engines", lambda *a, **k: called.append("engines"))

    def unit(k=32, cs=(1.5, 1.2), its0=0, with_x=False, with_x2=False):
        z = torch.zeros((k, k), dtype=torch.float64)
        u = {"S": z, "tau": 1e-2, "cs": list(cs), "its0": its0}
        if with_x:
            u["X"] = z.clone()
        if with_x2:
            u["X2"] = z.clone()
        return u
    for units in ([], [unit() for _ in range(17)]):
        with pytest.raises(ValueError, match=r"_sign_steps_group: 1 \.\. 16 units"):
            gp._sign_steps_group(units)
    for other in (unit(k=48), unit(with_x=True), unit(with_x=True, with_x2=True), unit(cs=(1.5, 1.3)), unit(cs=(1.5,)),
                  unit(its0=8)):
        with pytest.raises(ValueError, match="_sign_steps_group: the units of one call share"):
            gp._sign_steps_group([unit(), other])
    assert not called


def test_basis_requests_are_kinds_of_their_own():
    for kind, entry in (("sweeps", "gpfit_subspace_sweeps_batch"), ("sign", "gpfit_sign_steps_batch")):
        rec = gp._request_kind({"kind": kind})
        assert rec.kind == kind and rec.book == "basis_" and rec.entry == entry and rec.switch == "BASIS_GROUPS"
        assert rec is gp._REQUEST_KINDS[kind, None] and gp._ChainRendezvous._book({"kind": kind}) == "basis_"
    assert gp._ALL_BOOKS == ("", "closure_", "full_", "full_closure_", "loss_", "basis_")
    assert {key for key, rec in gp._REQUEST_KINDS.items() if rec.book == "basis_"} == {("sweeps", None), ("sign", None)}
    for name in ("last_basis_group_sizes", "last_basis_call_seconds", "last_seconds_in_basis_call"):
        assert hasattr(gp.varGP_cells, name)
    assert gp.BASIS_GROUPS in (False, True) and gp.SIGN_CHAIN in (False, True)
