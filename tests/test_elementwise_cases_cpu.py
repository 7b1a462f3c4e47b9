"""Pins elementwise_cases.py, the reference behind test_gpu_elementwise.py, so that it cannot be wrong in the same way
as the kernels: every reference against a second, independent formulation.

  trmv, trmv_t, symv, gemv        dense products of numpy.tril / the mirrored matrix
  adjoint, adjoint_rect           torch.autograd (float64) through oracle.arccos_gram contracted with the same W: the
                                  gradient with respect to the stimuli is (A_w x2) C + diag(u / q1) x1 C, with respect to
                                  sigma_0 it is 2 sigma_0 (sum A_w + (sum u1/q1 + sum u2/q2) / 2) -- the definition of
                                  A_w, u, v and of the three sums.  (The oracle divides by qq + 1e-7 where the adjoint
                                  formulas take the cosine as given: agreement to 1e-6 of the terms, not to rounding.)
  metric_contract                 the oracle's five dC contracted with M
  dk_sigma0, dk_metric, dq        the oracle's six dK, with H, dq1, dq2 formed from the oracle's dC
  moments, estep_prep             oracle.latent_moments / rate_mean with a = I; oracle.newton_estep and estep_cholesky
                                  on K~ = I, where V = diag(1 / (1 + s^2)) and m_new = V rhs give s and rhs back
  pack, unpack, mirror, pad ops   numpy.tril / triu / eye expressions
(wl of the moments has no counterpart in the oracle; it is restated in float64 torch from the oracle's J and f.)

It also measures the floor of every formula op -- the largest scaled error of ``plain`` against ``reference`` -- and
asserts the table ``FLOOR`` from which the GPU module takes its bars."""
import math

import numpy as np
import pytest
import torch

import elementwise_cases as ec
from gaussian_processes_amd import synthetic as syn
from oracle import gp_oracle as orc

LD = ec.LD
LOWER, UPPER = syn.limits()
F = lambda a: np.asarray(a, dtype=np.float64)


def close(a, b, scale, tol):
    return float(np.max(np.abs(F(a) - F(b)) / np.maximum(F(scale), 1e-300))) <= tol


# ------------------------------------------------------------------ the table of floors
@pytest.mark.parametrize("op", sorted(ec.FLOOR))
def test_floor_table_holds_the_measured_floor(op):
    """Within a factor of two on either side (another libm moves the figure; that variation is absorbed here, not in the
    kernel's bar); figures below one rounding of fp64 count as one rounding."""
    measured, recorded = ec.floor_of(op), ec.FLOOR[op]
    print(f"floor {op}: measured {measured:.3e} recorded {recorded:.3e}")
    lo = ec.U53
    assert max(recorded, lo) / 2.0 <= max(measured, lo) <= 2.0 * max(recorded, lo)
    assert 16.0 * max(recorded, lo) < 1e-13


def test_every_formula_op_has_a_floor_and_every_op_its_cases():
    for op, cases in ec.CASES.items():
        kinds = {o.kind for case in cases for o in ec.plain(op, ec.inputs(op, case)).values()}
        assert ("formula" in kinds) == (op in ec.FLOOR), op
    assert set(ec.F32_CASES) <= set(ec.CASES) and set(ec.GROUP_CASES) <= set(ec.CASES)


@pytest.mark.parametrize("op", sorted(ec.CASES))
def test_plain_lies_within_the_bounds_and_nothing_unread_leaks(op):
    """The fp64 evaluation of the same formula meets the bounds the kernels are held to (a-priori for sums, bit for bit
    for exact outputs), in fp64 and from fp32 inputs; no NaN of the unread parts reaches a result."""
    for case in ec.CASES[op]:
        for dtype in (np.float64, np.float32)[:2 if ec.F32_CASES.get(op) == case else 1]:
            inp = ec.inputs(op, case, dtype)
            ref, pl = ec.reference(op, inp), ec.plain(op, inp)
            for name, o in ref.items():
                assert np.all(np.isfinite(F(o.val))), (op, case, name)
                if o.kind == "formula":
                    continue
                ratio, msg = ec.check(op, name, pl[name].val, o, np.where(o.own, 0, F(o.val)))
                assert msg is None, msg


# ------------------------------------------------------------------ matrix-vector products
@pytest.mark.parametrize("op", ["trmv_lower", "trmv_lower_t", "symv_lower", "gemv_sub", "gemv_t_sub"])
def test_products_against_dense_numpy(op):
    for case in ec.CASES[op]:
        i = ec.inputs(op, case)
        (name, o), = ec.reference(op, i).items()
        if op.startswith("trmv"):
            L = np.tril(np.nan_to_num(i["L"][:, :i["np"]]))
            want = L @ i["x"] if op == "trmv_lower" else L.T @ i["x"]
        elif op == "symv_lower":
            A = np.tril(np.nan_to_num(i["A"][:, :i["n"]]))
            want = (A + np.tril(A, -1).T) @ i["x"]
        else:
            M = i["M"][:, :i["cols"]]
            want = i["y"] - (M @ i["x"] if op == "gemv_sub" else M.T @ i["x"])
        assert np.all(np.abs(F(o.val) - want) <= F((o.k + 3) * ec.U53 * o.S)), (op, case)
        assert np.all(o.k == (np.arange(len(want)) + 1 if op == "trmv_lower" else o.k))


# ------------------------------------------------------------------ layout ops
def test_pack_and_mirror_ops_against_tril_triu_eye():
    for n in ec.CASES["pack_lower"]:
        i = ec.inputs("pack_lower", n)
        o = ec.reference("pack_lower", i)["dst"]
        npad = i["np"]
        want = np.eye(npad)
        want[:n, :n] = i["A"][:, :n]
        t = np.kron(np.tril(np.ones((npad // 128, npad // 128))), np.ones((128, 128))).astype(bool)
        assert np.array_equal(o.own[:, :npad], t) and not o.own[:, npad:].any()
        assert np.array_equal(F(o.val[:, :npad])[t], want[t]) and np.all(F(o.val[:, :npad])[~t] == ec.SENTINEL)
    for n in ec.N3:
        A = np.nan_to_num(ec.inputs("pack_tri", n)["A"][:, :n])
        npad = ec.round_up(n, 128)
        want = np.eye(npad)
        want[:n, :n] = np.tril(A)
        o = ec.reference("pack_tri", ec.inputs("pack_tri", n))["dst"]
        assert np.array_equal(F(o.val[:, :npad]), want) and o.own[:, :npad].all()
        A = np.nan_to_num(ec.inputs("unpack_sym", n)["A"][:, :n])
        o = ec.reference("unpack_sym", ec.inputs("unpack_sym", n))["dst"]
        assert np.array_equal(F(o.val[:, :n]), np.tril(A) + np.triu(A.T, 1))
        A = np.nan_to_num(ec.inputs("unpack_tri", n)["A"][:, :n])
        o = ec.reference("unpack_tri", ec.inputs("unpack_tri", n))["dst"]
        assert np.array_equal(F(o.val[:, :n]), np.tril(A))
    for n in ec.CASES["symmetrize"]:
        i = ec.inputs("symmetrize", n)
        o = ec.reference("symmetrize", i)["A"]
        A = i["A"][:, :n]
        assert np.array_equal(F(o.val[:, :n]), np.tril(A) + np.triu(A.T, 1))
        assert np.array_equal(o.own[:, :n], np.triu(np.ones((n, n), bool), 1)) and np.all(F(o.val[:, n:]) == ec.SENTINEL)
    for n in ec.CASES["symmetrize_avg"]:
        i = ec.inputs("symmetrize_avg", n)
        o = ec.reference("symmetrize_avg", i)["A"]
        A = i["A"][:, :n]
        assert np.array_equal(F(o.val[:, :n]), (A + A.T) / 2) and np.array_equal(F(o.val[:, :n]), F(o.val[:, :n]).T)
    for c in ec.CASES["pad_copy"]:
        i = ec.inputs("pad_copy", c)
        o = ec.reference("pad_copy", i)["dst"]
        want = np.zeros((c[2], c[3]))
        want[:c[0], :c[1]] = i["src"][:, :c[1]]
        assert np.array_equal(F(o.val[:, :c[3]]), want)
    for c in ec.CASES["gather"]:
        i = ec.inputs("gather", c)
        o = ec.reference("gather", i)
        n, d = i["n"], i["d"]
        assert np.array_equal(F(o["Xt"].val[:d, :n]), i["X"][:n][:, i["pix"]].T)
        assert np.all(F(o["Xt"].val[d:, :i["np"]]) == 0) and np.all(F(o["Xt"].val[:, n:i["np"]]) == 0)
    for n in ec.CASES["estep_build"]:
        i = ec.inputs("estep_build", n)
        o = ec.reference("estep_build", i)
        npad, s, K = i["np"], i["sv"][:n], i["K"][:, :n]
        M = np.eye(npad)
        M[:n, :n] += s[:, None] * K * s[None, :]
        t = ec.tile_lower_mask(npad)
        assert np.allclose(F(o["Mb"].val[:, :npad])[t], M[t], rtol=1e-15, atol=1e-15)
        assert np.array_equal(F(o["Kl"].val[:n, :n])[t[:n, :n]], K[t[:n, :n]]) and np.all(F(o["Kl"].val[n:, :npad])[t[n:]] == 0)
        assert np.all(F(o["SK"].val[n:, :npad]) == 0) and np.all(F(o["SK"].val[:, n:npad]) == 0)


# ------------------------------------------------------------------ the adjoint passes
def _oracle_metric():
    C = ec.metric_terms(ec.theta8(), np.arange(25), 5, 5, np.float64)[0]
    return torch.from_numpy(C)


def _autograd(x1, x2, Wc, same):
    """d/dx1 and d/dx2 of sum(Wc o K) with K of oracle.arccos_gram (x2 is x1 itself when ``same``); C, q1, q2."""
    C = _oracle_metric()
    s0 = ec.THETA["sigma_0"]
    with torch.enable_grad():      # (other modules of the suite switch gradients off for the process)
        a = torch.tensor(x1, requires_grad=True)
        b = a if same else torch.tensor(x2, requires_grad=True)
        K = orc.arccos_gram({"sigma_0": s0}, a, b, C)
        loss = (torch.from_numpy(Wc) * K).sum()
        ga, = torch.autograd.grad(loss, a, retain_graph=True)
        gb = None if same else torch.autograd.grad(loss, b)[0].numpy()
    q = lambda x: torch.sqrt(((x.detach() @ C) * x.detach()).sum(1) + s0 * s0).numpy()      # :978
    return ga.numpy(), gb, C.numpy(), q(a), q(b)


@pytest.mark.parametrize("case", [c for c in ec.CASES["adjoint_rect"] if c[4] == 0])
def test_adjoint_rect_is_the_gradient_of_the_oracle_gram(case):
    n1, n2 = case[0], case[1]
    i = ec.inputs("adjoint_rect", case)
    o = ec.reference("adjoint_rect", i)
    W = i["W"][:, :n2]
    x1, x2 = syn.stimuli(n1, 25, 7), syn.stimuli(n2, 25, 7 + 101)
    g1, g2, C, q1, q2 = _autograd(x1, x2, W, same=False)      # (1 x 1: the oracle's symmetrised K is K itself)
    assert np.allclose(q1, i["q1"][:n1], rtol=1e-14) and np.allclose(q2, i["q2"][:n2], rtol=1e-14)
    Aw, uq1, uq2 = F(o["Aout"].val[:n1, :n2]), F(o["uq1"].val[:n1]), F(o["uq2"].val[:n2])
    want1 = (Aw @ x2) @ C.T + uq1[:, None] * (x1 @ C)
    want2 = (Aw.T @ x1) @ C + uq2[:, None] * (x2 @ C)
    s1 = (np.abs(Aw) @ np.abs(x2)) @ np.abs(C) + np.abs(uq1)[:, None] * np.abs(x1 @ C)
    s2 = (np.abs(Aw.T) @ np.abs(x1)) @ np.abs(C) + np.abs(uq2)[:, None] * np.abs(x2 @ C)
    assert close(g1, want1, s1 + 1e-300, 1e-6) and close(g2, want2, s2 + 1e-300, 1e-6)
    # t = u / (2 q), and the three sums are those of the outputs
    assert close(o["t1"].val[:n1], 0.5 * uq1, np.abs(uq1), 1e-15) and close(o["t2"].val[:n2], 0.5 * uq2, np.abs(uq2), 1e-15)
    assert close(o["scal3"].val, [Aw.sum(), uq1.sum(), uq2.sum()], o["scal3"].S, 1e-14)
    assert np.all(F(o["Aout"].val[n1:, :case[3]]) == 0) and np.all(F(o["Aout"].val[:, n2:case[3]]) == 0)


def test_adjoint_rect_adds_extra1():
    for case in ec.CASES["adjoint_rect"]:
        if case[4]:
            i = ec.inputs("adjoint_rect", case)
            o = ec.reference("adjoint_rect", i)
            n1 = case[0]
            assert close(o["t1"].val[:n1], 0.5 * F(o["uq1"].val[:n1]) + i["extra1"][:n1], o["t1"].S[:n1], 1e-15)


@pytest.mark.parametrize("case", ec.CASES["adjoint"])
def test_adjoint_is_the_gradient_of_the_oracle_gram(case):
    """sum_{i != j} w_ij K_ij with w = W - b b^T / 2 (the diagonal of the cosine is exactly 1 in the inputs and 1 - 1e-7 / q^2
    in the oracle: the diagonal term is checked by its formula, 1/2 w_ii, instead)."""
    n, npad = case
    i = ec.inputs("adjoint", case)
    o = ec.reference("adjoint", i)
    sym = lambda a: np.tril(a) + np.tril(a, -1).T
    W = sym(np.nan_to_num(i["W"][:n, :n]))
    b, q, wl = i["b"][:n], i["q"][:n], i["wl"][:n]
    w = W - 0.5 * np.outer(b, b)
    lam = F(o["Aout"].val[:n, :n])
    own = o["Aout"].own[:n, :n]
    assert np.all(np.triu(lam, 1)[own] == 0) and np.all(np.triu(lam, 1)[~own] == ec.SENTINEL)   # untouched tiles above
    lam = np.tril(lam)
    assert close(np.diag(lam), 0.5 * np.diag(w), np.abs(np.diag(W)) + 0.5 * b * b, 1e-15)      # c = 1: (pi - acos 1) / pi = 1
    Aw_off = np.tril(lam, -1) + np.tril(lam, -1).T
    uq = F(o["uq"].val[:n])
    x = syn.stimuli(n, 25, 5)
    w_off = w - np.diag(np.diag(w))
    g, _, C, q1, _ = _autograd(x, x, w_off, same=True)
    assert np.allclose(q1, q, rtol=1e-14)
    want = 2.0 * ((Aw_off @ x) @ C) + 2.0 * uq[:, None] * (x @ C)      # both roles of x: twice the one-sided gradient
    scale = 2.0 * ((np.abs(Aw_off) @ np.abs(x)) @ np.abs(C)) + 2.0 * np.abs(uq)[:, None] * np.abs(x @ C)
    if n > 1:
        assert close(g, want, scale, 1e-6)
    assert close(o["tvec"].val[:n], uq - wl, o["tvec"].S[:n], 1e-15)
    full = Aw_off + 2.0 * np.diag(np.diag(lam))
    assert close(o["scal"].val, [uq.sum(), wl.sum(), full.sum()], o["scal"].S, 1e-14)
    assert np.all(F(o["uq"].val[n:]) == 0) and np.all(F(o["tvec"].val[n:]) == 0)
    t64 = ec.tile_lower_mask(npad, 64)
    assert np.array_equal(o["Aout"].own[:, :npad], t64) and np.all(F(o["Aout"].val[n:, :npad])[t64[n:]] == 0)


# ------------------------------------------------------------------ the metric and the six dK
@pytest.mark.parametrize("case", ec.CASES["metric_contract"])
def test_metric_contract_against_the_oracle_dC(case):
    n_rows, n_cols, keep = case
    i = ec.inputs("metric_contract", case)
    C, mask, dC = orc.spatial_metric(ec.THETA, LOWER, UPPER, (n_rows, n_cols), grad=True)
    assert bool(mask.all())
    pix = i["pix"]
    assert np.allclose(i["C"][:, :i["d"]], C.numpy()[np.ix_(pix, pix)], rtol=1e-14, atol=0)
    M = i["M"][:, :i["d"]]
    o = ec.reference("metric_contract", i)["grad5"]
    want = [float((dC[k].numpy()[np.ix_(pix, pix)] * M).sum()) for k in orc.DC_KEYS]
    assert close(o.val, want, o.S, 1e-14)


@pytest.mark.parametrize("n1,n2", ec.RECT)
def test_dk_ops_against_the_oracle_six_dK(n1, n2):
    """H = x1 dC x2^T and dq = (x dC x) / (2 q) from the oracle's dC, through the references of dq and dk_metric; sigma_0
    through dk_sigma0: the oracle's six dK."""
    theta = ec.THETA
    C, mask, dC = orc.spatial_metric(theta, LOWER, UPPER, (5, 5), grad=True)
    x1, x2 = syn.stimuli(n1, 25, 11), syn.stimuli(n2, 25, 11 + 101)
    K, dK = orc.arccos_gram(theta, x1, x2, C, dC)
    cos, q1, q2 = ec.gram(n1, n2, 11)
    base = dict(Cos=np.array(cos), q1=np.array(q1), q2=np.array(q2), n1=n1, n2=n2, s0=theta["sigma_0"])
    got = F(ec.reference("dk_sigma0", base)["dK"].val[:, :n2])
    assert close(got, dK["sigma_0"].numpy(), np.abs(dK["sigma_0"].numpy()) + 1.0, 1e-12)
    for key in orc.DC_KEYS:
        D = dC[key].numpy()
        dq = {}
        for name, x, q in (("dq1", x1, q1), ("dq2", x2, q2)):
            n = x.shape[0]
            inp = dict(Xt=np.ascontiguousarray(x.T), XDt=np.ascontiguousarray((x @ D).T), q=np.array(q), n=n, dp=25, want=3)
            r = ec.reference("dq", inp)
            assert close(r["h"].val, ((x @ D) * x).sum(1), r["h"].S, 1e-14)
            dq[name] = F(r["dq"].val)
        H = x1 @ D @ x2.T
        o = ec.reference("dk_metric", dict(base, H=H, **dq))["H"]
        want = dK[key].numpy()
        assert close(o.val[:, :n2], want, o.S[:, :n2] + 1e-300, 1e-11), key


# ------------------------------------------------------------------ moments and the E-step's vectors
@pytest.mark.parametrize("n", ec.CASES["moments"])
def test_moments_against_the_oracle(n):
    i = ec.inputs("moments", n)
    o = ec.reference("moments", i)
    d = np.arange(n)
    c = torch.from_numpy(i["Cos"][d, d])
    q = torch.from_numpy(i["q"])
    delta = torch.arccos(c)
    J = (torch.sqrt(1 - c * c) + orc.PI32 * c - delta * c) / orc.PI32        # oracle.arccos_gram, :988
    K = torch.diag(q * q * J)                                                # :990
    V = torch.diag(torch.from_numpy(i["V"][d, d]))
    m, r = torch.from_numpy(i["m"]), torch.from_numpy(i["r"])
    lam_m, lam_var = orc.latent_moments(torch.eye(n, dtype=torch.float64), K, torch.from_numpy(i["Kvec"]), m, V)
    logA = math.log(i["A"])
    f = orc.rate_mean(logA, i["lambda0"], lam_m, lam_var)
    assert np.array_equal(F(o["lam_m"].val), lam_m.numpy())
    assert close(o["lam_var"].val, lam_var.numpy(), o["lam_var"].S, 1e-14)
    assert close(o["f"].val, f.numpy(), o["f"].S, 1e-14)
    assert close(o["scal"].val, [float(r @ lam_m), float(r.sum()), float(f.sum())], o["scal"].S, 1e-13)
    # wl = -1/2 A^2 f g with g = 1 - J - (pi - delta)(1 - c) / pi has no counterpart in the oracle: by its formula, float64
    g = 1 - J - (orc.PI32 - delta) * (1 - c) / orc.PI32
    assert close(o["wl"].val, (-0.5 * i["A"] ** 2 * f * g).numpy(), o["wl"].S, 1e-14)
    assert float(np.max(np.abs(F(o["wl"].val)))) > 0 or n == 1


@pytest.mark.parametrize("case", ec.CASES["estep_prep"])
def test_estep_prep_against_the_oracle_on_the_identity(case):
    n, npad = case
    i = ec.inputs("estep_prep", case)
    o = ec.reference("estep_prep", i)
    f, r, m = (torch.from_numpy(i[k]) for k in ("f", "r", "m"))
    eye = torch.eye(n, dtype=torch.float64)
    logA = math.log(i["A"])
    m_new, V = orc.newton_estep(r, eye, m, logA, f, eye)
    m_chol, V_chol = orc.estep_cholesky(eye, r, m, f, logA)
    s2 = 1.0 / torch.diagonal(V_chol) - 1.0                         # V = diag(1 / (1 + s^2))
    rhs = m_new / torch.diagonal(V)                                 # m_new = V rhs
    sv, want = F(o["sv"].val), F(o["rhs"].val)
    assert close(sv[:n] ** 2, s2.numpy(), np.abs(s2.numpy()) + 1.0, 1e-13)
    assert close(want[:n], rhs.numpy(), o["rhs"].S[:n], 1e-13)
    assert np.all(sv[n:] == 0) and np.all(want[n:] == 0) and len(sv) == npad


def test_qvec_against_numpy():
    for case in ec.CASES["qvec"]:
        n, dp = case
        i = ec.inputs("qvec", case)
        o = ec.reference("qvec", i)
        # Kvec = diag(x C x^T) + s0^2 with XCt = (x C)^T (oracle.arccos_gram_diag, :1029); q = sqrt (:978)
        kv = (i["Xt"][:, :n] * i["XCt"][:, :n]).sum(0) + i["s0sq"]
        assert close(o["Kvec"].val[:n], kv, o["Kvec"].S[:n], 1e-14) and close(o["q"].val[:n], np.sqrt(kv), o["q"].S[:n], 1e-14)
        assert np.all(F(o["q"].val[n:]) == 1) and np.all(F(o["Kvec"].val[n:]) == 1)


def test_op_numbers_of_the_binding_follow_the_header():
    """_lib.EW_OPS is the header's enum in its order; every op has cases here."""
    import os
    import re
    from conftest import ROOT
    from gaussian_processes_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpfit_mi355x.h")).read()
    body = hdr[hdr.index("GPFIT_EW_TRMV_LOWER = 0"):hdr.index("GPFIT_EW_NOPS")]
    names = [m.lower() for m in re.findall(r"GPFIT_EW_(\w+)", body)]
    assert names == list(_lib.EW_OPS)
    assert int(re.search(r"GPFIT_EW_GROUP = (\d+)", hdr).group(1)) == _lib.EW_GROUP
    assert set(ec.CASES) | {"adjoint_reduce"} == set(_lib.EW_OPS)
