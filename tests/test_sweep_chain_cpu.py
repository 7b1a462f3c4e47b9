"""The hand-over of a pass of the subspace iteration to a ``sweep_chain`` (eigtop.top_eigenpairs) and the refusals of
``utils._basis_sweeps_group``, without a GPU: on the torch CPU stand-ins of tests/test_eigtop_cpu.py a chain that restates
the step list of include/gpfit_mi355x.h (gpfit_subspace_sweeps) must give the results of the host loop bit for bit, be
asked exactly what that loop would have applied, and pass a failure on; the group wrapper must refuse mixed lists before
any call goes out (stub batch entry)."""
import pytest
import torch

from gaussian_processes_amd import eigtop, utils as gp
from test_eigtop_cpu import cpu_cholesky, cpu_matmul, kernel_like_matrix


class Chain:
    """The step list in torch, with a record of every call."""

    def __init__(self, fail_at_call=None):
        self.calls = []
        self.fail_at_call = fail_at_call

    def __call__(self, K, Q, Y, shifts, want_rr):
        self.calls.append({"Y": Y, "Q": Q, "shifts": list(shifts), "want_rr": want_rr})
        if self.fail_at_call == len(self.calls):
            return None
        for j, sigma in enumerate(shifts):
            if not (j == 0 and Y is not None):
                Y = cpu_matmul(K, Q)
            if sigma != 0.0:
                Y.sub_(Q, alpha=sigma)              # (the host loop's own operation: whatever rounding it has here)
            for _ in range(2 if j == len(shifts) - 1 else 1):
                G = cpu_matmul(Y, Y, transA=True)
                G = (G + G.T) * 0.5
                L, Li, _, info = cpu_cholesky(G, want_inverse=True)
                if info != 0:
                    return None
                Y = cpu_matmul(Y, Li, transB=True)
            Q = Y
        if not want_rr:
            return Q, None, None
        Y = cpu_matmul(K, Q)
        S = cpu_matmul(Q, Y, transA=True)
        return Q, Y, (S + S.T) * 0.5


def problem(n=900, seed=0):
    K, _, _ = kernel_like_matrix(n, seed)
    return ((K + K.T) / 2).contiguous()


def same(a, b):
    """Two results of top_eigenpairs, bit for bit, with the counters of the loop."""
    assert a is not None and b is not None
    for x, y in zip(a[:2], b[:2]):
        assert (x is None and y is None) or torch.equal(x, y)
    for key in ("sweeps", "products", "n", "k", "grown", "rr"):
        assert a[2].get(key) == b[2].get(key), key
    for key in ("K_tilde_b", "K_tilde_inv_b"):
        if key in a[2]:
            assert torch.equal(a[2][key], b[2][key]), key
    if "state" in a[2]:
        assert torch.equal(a[2]["state"]["Q"], b[2]["state"]["Q"]) and torch.equal(a[2]["state"]["U"], b[2]["state"]["U"])


CASES = {
    "cold": dict(k0=160, basis="subspace"),
    "cold eigenpairs": dict(k0=128),
    "grows": dict(k0=32, basis="subspace"),
    "grows eigenpairs": dict(k0=16),
    "plain": dict(k0=128, accelerate=False),
    "plain subspace": dict(k0=160, basis="subspace", accelerate=False),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_chain_that_restates_the_steps_gives_the_bits_of_the_host_loop(case):
    K, kw = problem(), CASES[case]
    ref = eigtop.top_eigenpairs(K, 1e-4, cpu_matmul, cpu_cholesky, **kw)
    chain = Chain()
    got = eigtop.top_eigenpairs(K, 1e-4, cpu_matmul, cpu_cholesky, sweep_chain=chain, **kw)
    same(got, ref)
    assert chain.calls and all(c["want_rr"] for c in chain.calls)
    if case.startswith("grows"):
        assert ref[2]["grown"] >= 1
    # every pass whose block is a multiple of 16 wide went to the chain, once: the sweeps the chain ran and the one
    # unshifted sweep in front of each planned pass add up to the loop's count
    planned = sum(1 for c in chain.calls if c["Y"] is not None)
    assert sum(len(c["shifts"]) for c in chain.calls) + planned <= ref[2]["sweeps"]
    if kw.get("accelerate", True):
        assert chain.calls[0]["Y"] is not None and chain.calls[0]["shifts"][0] != 0.0
    else:
        assert all(c["Y"] is None and set(c["shifts"]) == {0.0} for c in chain.calls)
        assert sum(len(c["shifts"]) for c in chain.calls) == ref[2]["sweeps"]


def test_a_warm_start_hands_over_behind_its_plan_and_keeps_its_counters():
    K = problem()
    cold = eigtop.top_eigenpairs(K, 1e-4, cpu_matmul, cpu_cholesky, k0=160, basis="subspace")
    g = torch.Generator().manual_seed(9)
    E = torch.randn(K.shape, dtype=torch.float64, generator=g)
    K2 = (K * (1 + 1e-4) + 1e-9 * (E + E.T)).contiguous()
    ref = eigtop.top_eigenpairs(K2, 1e-4, cpu_matmul, cpu_cholesky, k0=160, basis="subspace", start=cold[2]["state"])
    chain = Chain()
    got = eigtop.top_eigenpairs(K2, 1e-4, cpu_matmul, cpu_cholesky, k0=160, basis="subspace", start=cold[2]["state"],
                                sweep_chain=chain)
    same(got, ref)
    assert ref[2]["warm"] and got[2]["warm"] and got[2]["start_angle"] == ref[2]["start_angle"]
    # one pass: the unshifted sweep ran on the host (the plan needs its quotients), the rest in one call with its product
    assert len(chain.calls) == 1 and chain.calls[0]["Y"] is not None
    assert len(chain.calls[0]["shifts"]) == ref[2]["sweeps"] - 1
    assert not torch.equal(cold[2]["state"]["Q"], got[2]["state"]["Q"])      # the old block was not written over


def test_the_chain_is_asked_for_the_shifts_the_host_loop_applies(monkeypatch):
    """The loop's shifts, read off its ``Y.sub_(Q, alpha=sigma)`` calls, against the lists the chain was given."""
    K = problem()
    applied = []
    real = torch.Tensor.sub_

    def sub_(self, other, *, alpha=1):
        applied.append(float(alpha))
        return real(self, other, alpha=alpha)
    monkeypatch.setattr(torch.Tensor, "sub_", sub_)
    ref = eigtop.top_eigenpairs(K, 1e-4, cpu_matmul, cpu_cholesky, k0=160, basis="subspace")
    monkeypatch.setattr(torch.Tensor, "sub_", real)
    chain = Chain()
    got = eigtop.top_eigenpairs(K, 1e-4, cpu_matmul, cpu_cholesky, k0=160, basis="subspace", sweep_chain=chain)
    same(got, ref)
    asked = [s for c in chain.calls for s in c["shifts"]]
    assert asked == applied and len(applied) == ref[2]["sweeps"] - 1 and all(s > 0 for s in asked)


def test_a_re_swept_block_goes_at_once_and_without_a_product():
    """A first pass cut short (``first_sweeps=3``) does not converge: the second pass has its interval already and is
    handed over before any product of it, the first behind its plan."""
    K = problem()
    kw = dict(k0=160, basis="subspace", first_sweeps=3)
    ref = eigtop.top_eigenpairs(K, 1e-4, cpu_matmul, cpu_cholesky, **kw)
    chain = Chain()
    got = eigtop.top_eigenpairs(K, 1e-4, cpu_matmul, cpu_cholesky, sweep_chain=chain, **kw)
    same(got, ref)
    assert ref[2]["sweeps"] > 3 and len(chain.calls) >= 2
    assert chain.calls[0]["Y"] is not None and len(chain.calls[0]["shifts"]) == 2
    assert all(c["Y"] is None for c in chain.calls[1:])
    assert 1 + sum(len(c["shifts"]) for c in chain.calls) == ref[2]["sweeps"]


def test_a_block_that_is_no_multiple_of_16_wide_stays_on_the_host():
    K = problem()
    ref = eigtop.top_eigenpairs(K, 1e-4, cpu_matmul, cpu_cholesky, k0=168, basis="subspace")
    chain = Chain()
    got = eigtop.top_eigenpairs(K, 1e-4, cpu_matmul, cpu_cholesky, k0=168, basis="subspace", sweep_chain=chain)
    same(got, ref)
    assert chain.calls == []


def test_a_padded_matrix_hands_the_padded_problem_over():
    K = problem(n=890)
    ref = eigtop.top_eigenpairs(K, 1e-4, cpu_matmul, cpu_cholesky, k0=160, basis="subspace")
    chain = Chain()
    got = eigtop.top_eigenpairs(K, 1e-4, cpu_matmul, cpu_cholesky, k0=160, basis="subspace", sweep_chain=chain)
    same(got, ref)
    assert chain.calls and all(c["Q"].shape == (896, 160) for c in chain.calls)


@pytest.mark.parametrize("call", [1, 2])
def test_a_chain_that_fails_makes_the_solver_decline(call):
    K = problem()
    chain = Chain(fail_at_call=call)
    assert eigtop.top_eigenpairs(K, 1e-4, cpu_matmul, cpu_cholesky, k0=160, basis="subspace", first_sweeps=3,
                                 sweep_chain=chain) is None
    assert len(chain.calls) == call


# ---------------------------------------------------------------------------------------------- the group wrapper
class Engine:
    _ctx = 0
    device = 0

    def __init__(self, n_max=256):
        self.n_max = n_max


def unit(N=64, k=32, with_y=False, want_rr=True, shifts=(0.0, 0.5)):
    u = {"K": torch.eye(N, dtype=torch.float64), "Q": torch.ones(N, k, dtype=torch.float64), "shifts": list(shifts),
         "want_rr": want_rr}
    if with_y:
        u["Y"] = torch.ones(N, k, dtype=torch.float64)
    return u


def set_batch(monkeypatch, batch):
    """The batch entry of the kind "sweeps" replaced (the group wrapper calls what the kind's record names)."""
    key = ("sweeps", None)
    monkeypatch.setitem(gp._REQUEST_KINDS, key, gp._REQUEST_KINDS[key]._replace(batch=batch))


@pytest.fixture
def stubbed(monkeypatch):
    """_basis_sweeps_group with workspaces, stream and batch entry replaced: what it would have sent is recorded."""
    sent = []

    class Stream:
        value = None
    monkeypatch.setattr(gp, "_stream", lambda: Stream())
    monkeypatch.setattr(gp, "_group_engines", lambda count, n, *a, **kw: [Engine() for _ in range(count)])

    def batch(ctxs, qs, rec=None):
        sent.append(qs)
        return 0, [len(q["shifts"]) if i % 2 == 0 else 0 for q in qs for i in range(2)]
    set_batch(monkeypatch, batch)
    return sent


def test_the_group_wrapper_refuses_mixed_keys_before_any_call(stubbed, monkeypatch):
    mixed = {"N": unit(N=80), "k": unit(k=48), "Y_READY": unit(with_y=True), "WANT_RR": unit(want_rr=False)}
    for what, other in mixed.items():
        with pytest.raises(ValueError, match="gpfit_subspace_sweeps_batch: the requests of one call share"):
            gp._basis_sweeps_group([unit(), other])
    assert stubbed == []
    # the capacity of the workspaces is part of the key
    caps = iter([Engine(256), Engine(512)])
    monkeypatch.setattr(gp, "_group_engines", lambda count, n, *a, **kw: [next(caps) for _ in range(count)])
    with pytest.raises(ValueError, match="share"):
        gp._basis_sweeps_group([unit(), unit()])
    assert stubbed == []
    for units in ([], [unit()] * 17):
        with pytest.raises(ValueError, match="_basis_sweeps_group: 1 .. 16 units per call"):
            gp._basis_sweeps_group(units)
    assert stubbed == []


def test_the_group_wrapper_sends_one_call_and_cuts_the_results_per_unit(stubbed, monkeypatch):
    units = [unit(shifts=(0.0,)), unit(shifts=(0.0, 0.3, 0.1)), unit(shifts=())]
    res = gp._basis_sweeps_group(units)
    assert len(stubbed) == 1 and [q["shifts"] for q in stubbed[0]] == [[0.0], [0.0, 0.3, 0.1], []]
    assert all(q["flags"] == 2 and q["N"] == 64 and q["k"] == 32 for q in stubbed[0])
    for u, (q, r) in enumerate(zip(stubbed[0], res)):
        assert r[0] is q["Q"] and r[1] is q["Y"] and r[2] is q["S"]
        assert q["Q"] is not units[u]["Q"] and r[2].shape == (32, 32)
    # a unit whose factorisation failed has None in its place, the others their results
    set_batch(monkeypatch, lambda ctxs, qs, rec=None: (0, [1, 0, 1, 4, 0, 0]))
    res = gp._basis_sweeps_group(units)
    assert res[1] is None and res[0] is not None and res[2] is not None


def test_the_switch_is_a_module_global_read_at_call_time(monkeypatch):
    """_stabilised_basis hands _basis_sweeps to the solver while SWEEP_CHAIN is on, and nothing when it is off."""
    seen = []
    monkeypatch.setattr(gp.eigtop, "top_eigenpairs", lambda *a, **kw: seen.append(kw.get("sweep_chain", "absent")))
    K = torch.zeros(gp._EIGTOP_MIN_N, gp._EIGTOP_MIN_N, dtype=torch.float64)
    for on in (True, False):
        monkeypatch.setattr(gp, "SWEEP_CHAIN", on)
        with pytest.raises(gp._lib.GpfitError, match="cannot be reproduced"):
            gp._stabilised_basis(K, route="subspace")
    assert seen == [gp._basis_sweeps, None]
