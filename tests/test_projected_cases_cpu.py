"""Pins projected_cases.py, the reference behind test_gpu_projected.py, so that it cannot be wrong in the same way as
the kernels:

  - the fp64 evaluation of every case (and of every unit of the group cases) lies within the bounds the kernels are held
    to, no NaN of the unread parts reaches a reference, and the exponent stays below 5 in magnitude;
  - every reference against a dense restatement with numpy's matrix products and einsum (utils.py:1090, 1101, 1138 for
    the moments; the adjoint formulas the kernels cite for G_a, G_Kb, G_K~b; utils.py:1421-1431 for the E-step);
  - the bounds discriminate: with column nb - 1 withheld from a row sum, or row n - 1 from a sum over the training
    points, the result falls outside its bound;
  - the FLOOR table holds the measured floors."""
import numpy as np
import pytest

import projected_cases as pc
import skinny_cases as sc
from elementwise_cases import LD, SENTINEL, U53

F = lambda a: np.asarray(a, dtype=np.float64)
ALL = [(op, case, 0) for op in pc.CASES for case in pc.CASES[op]] + [(op, case, u) for op in pc.GROUP_CASES
                                                                      for u, case in enumerate(pc.GROUP_CASES[op]) if u]


def bound_of(op, o):
    return (o.k + 2) * LD(U53) * o.S if o.kind == "sum" else LD(pc.bar(op)) * o.S


@pytest.mark.parametrize("op,case,unit", ALL, ids=[f"{op}-{case}-u{u}" for op, case, u in ALL])
def test_plain_lies_within_the_bounds_and_nothing_unread_leaks(op, case, unit):
    inp = pc.inputs(op, case, unit)
    ref, pl = pc.reference(op, inp), pc.plain(op, inp)
    for name, o in ref.items():
        assert np.all(np.isfinite(F(o.val))), (op, case, name)
        assert o.own.any()
    worst, msg = sc.check_all(op, sc.as_buffers(inp, pl), ref, inp["bufs"], pc.bar(op))
    assert msg is None, msg
    print(f"{op} {case} unit {unit}: worst error / bound {worst:.3f}")
    _, msg = sc.check_all(op, {b: inp["bufs"][b] for b in sc.as_buffers(inp, pl)}, ref, inp["bufs"], pc.bar(op))
    assert msg is not None                                   # an untouched output does not pass
    if op == "moments":
        lm, lv = pc.moment_terms(inp, LD)
        arg = inp["A"] * lm[0] + 0.5 * inp["A"] ** 2 * lv[0] + inp["lambda0"]
        assert float(np.max(np.abs(arg))) < 5.0


@pytest.mark.parametrize("op", sorted(pc.FLOOR))
def test_floor_table_holds_the_measured_floor(op):
    measured, recorded = sc.floor_of(op, pc.CASES[op], pc.inputs, pc.evaluate), pc.FLOOR[op]
    print(f"floor {op}: measured {measured:.3e} recorded {recorded:.3e}")
    assert max(recorded, U53) / 2.0 <= max(measured, U53) <= 2.0 * max(recorded, U53)
    assert 8.0 * max(recorded, U53) < 1e-14


def test_every_formula_op_has_a_floor_and_the_shapes_are_the_ragged_ones():
    for op, cases in pc.CASES.items():
        kinds = {o.kind for case in cases for o in pc.plain(op, pc.inputs(op, case)).values()}
        assert ("formula" in kinds) == (op in pc.FLOOR), op
    assert {nb for _, nb in pc.SHAPES} >= {1, 63, 65} and any(n % 4 for n, _ in pc.SHAPES)
    assert set(pc.GROUP_CASES) == set(pc.GROUP_OPS) and len(set(pc.UNIT_LINK)) == 3 and len(set(pc.GROUP_CASES["trace"])) == 3
    i = pc.inputs("estep_scale", (130, 65, 1))
    assert (i["np"], i["nrows"], i["npc"]) == (256, 160, 128) and i["bufs"]["part"].shape == (160 // 32 + 1, 128)
    assert pc.inputs("moments", (130, 65))["bufs"]["part"].shape == (3 * 33 + 5,)


def test_operands_hold_nan_wherever_the_contract_reads_nothing():
    i = pc.inputs("moments", (130, 65))
    for name in ("am", "Kb", "aV"):
        m = i["bufs"][name]
        assert m.shape == (256, 68) and np.isnan(m[130:]).all() and np.isnan(m[:, 65:]).all() and np.isfinite(m[:130, :65]).all()
    assert np.isnan(i["bufs"]["Kvec"][130:]).all() and np.isnan(i["bufs"]["r"][130:]).all() and np.isnan(i["bufs"]["mb"][65:]).all()
    i = pc.inputs("ga", (130, 65))
    assert np.isnan(i["bufs"]["gm"][130:]).all() and np.isnan(i["bufs"]["gv"][130:]).all() and np.isnan(i["bufs"]["Kb"][130:]).all()
    i = pc.inputs("gkb", (130, 65))
    assert np.isnan(i["bufs"]["GaKi"][130:256, :65]).all() and np.all(i["bufs"]["GaKi"][:, 65:] == SENTINEL)
    i = pc.inputs("trace", 130)
    assert np.isnan(i["bufs"]["A"]).sum() == 130 * pc.TRACE_LD - 130
    i = pc.inputs("estep_scale", (130, 65, 0))
    assert np.all(i["bufs"]["sv"][130:] == 0) and np.all(i["bufs"]["u"][130:] == 0) and np.isnan(i["bufs"]["aL"][:, 65:]).all()
    assert "aLp" not in i["bufs"] and "aLp" in pc.inputs("estep_scale", (130, 65, 1))["bufs"]


@pytest.mark.parametrize("case", pc.SHAPES)
def test_references_against_dense_numpy(case):
    n, nb = case
    near = lambda got, want, scale, k: np.all(np.abs(F(got) - want) <= (k + 8) * U53 * F(scale) + 1e-300)
    i = pc.inputs("moments", case)
    b, ref = i["bufs"], pc.reference("moments", i)
    am, Kb, aV, mb = b["am"][:n, :nb], b["Kb"][:n, :nb], b["aV"][:n, :nb], b["mb"][:nb]
    A, l0, r = i["A"], i["lambda0"], b["r"][:n]
    lm = am @ mb                                                           # utils.py:1090
    lv = b["Kvec"][:n] - np.einsum("ij,ij->i", am, Kb) + np.einsum("ij,ij->i", aV, am)   # :1101
    f = np.exp(A * lm + 0.5 * A * A * lv + l0)                             # :1138
    assert near(ref["lam_m"].val[:n], lm, ref["lam_m"].S[:n], nb) and near(ref["lam_var"].val[:n], lv, ref["lam_var"].S[:n], 2 * nb)
    assert near(ref["f"].val[:n], f, ref["f"].S[:n], 2 * nb) and near(ref["gm"].val[:n], A * (r - f), ref["gm"].S[:n], 2 * nb)
    assert near(ref["gv"].val[:n], -0.5 * A * A * f, ref["gv"].S[:n], 2 * nb)
    assert near(ref["out3"].val[:2], [r @ lm, r.sum()], ref["out3"].S[:2], n * nb)
    assert near(ref["out3.f"].val[2:3], [f.sum()], ref["out3.f"].S[2:3], n * nb)
    nblk = (n + 3) // 4
    assert near(ref["part"].val[2 * nblk:3 * nblk].sum(), f.sum(), ref["out3.f"].S[2], n * nb)
    assert ref["part"].own.sum() == 3 * nblk and ref["out3"].own.tolist() == [True, True, False, False, False]
    i = pc.inputs("ga", case)
    b, o = i["bufs"], pc.reference("ga", i)
    want = np.outer(b["gm"][:n], b["mb"][:nb]) - b["gv"][:n, None] * b["Kb"][:n, :nb] + 2 * b["gv"][:n, None] * b["aV"][:n, :nb]
    assert near(o["Ga"].val[:n, :nb], want, o["Ga"].S[:n, :nb], 4)
    assert np.array_equal(o["Ga"].own | o["Ga.zero"].own, np.pad(np.ones((i["np"], nb), bool), ((0, 1), (0, 3))))
    assert np.all(F(o["Ga.zero"].val)[n:i["np"], :nb] == 0)
    i = pc.inputs("gkb", case)
    b, o = i["bufs"], pc.reference("gkb", i)
    assert near(o["GaKi"].val[:n, :nb], b["gv"][:n, None] * b["am"][:n, :nb] - b["GaKi"][:n, :nb], o["GaKi"].S[:n, :nb], 4)
    assert np.array_equal(o["GaKi"].own | o["GaKi.zero"].own, np.pad(np.ones((i["np"], nb), bool), ((0, 1), (0, 3))))
    i = pc.inputs("gktb", case)
    b, o = i["bufs"], pc.reference("gktb", i)["G"]
    bb = np.outer(b["bvec"][:nb], b["bvec"][:nb])
    assert near(o.val[:nb, :nb], 0.5 * (b["Ki"][:, :nb] - bb - b["P1"][:, :nb]) + b["P2"][:, :nb], o.S[:nb, :nb], 4)
    assert np.array_equal(o.own, np.pad(np.ones((nb, nb), bool), ((0, 1), (0, 3))))
    i = pc.inputs("estep_rows", case)
    b, o = i["bufs"], pc.reference("estep_rows", i)
    f, r, A = b["f"][:n], b["r"][:n], i["A"]
    lam = b["a"][:, :nb] @ b["mb"][:nb]
    assert near(o["sv"].val[:n], A * np.sqrt(f), o["sv"].S[:n], 4)                        # utils.py:1421-1422
    assert near(o["u"].val[:n], A * A * f * lam + A * (r - f), o["u"].S[:n], nb)          # utils.py:1431 before a^T
    assert np.all(F(o["sv.zero"].val)[n:i["nrows"]] == 0) and (o["u"].own | o["u.zero"].own).sum() == i["nrows"]
    for with_alp in (0, 1):
        i = pc.inputs("estep_scale", case + (with_alp,))
        b, o = i["bufs"], pc.reference("estep_scale", i)
        aL = np.zeros((i["nrows"], i["npc"]))
        aL[:n, :nb] = b["aL"][:, :nb]
        Y = F(np.where(o["Y"].own, o["Y"].val, o["Y.zero"].val))[:i["nrows"], :i["npc"]]
        assert near(Y, b["sv"][:, None] * aL, np.abs(Y), 1) and (o["Y"].own | o["Y.zero"].own).sum() == i["nrows"] * i["npc"]
        assert near(o["part"].val[:-1].sum(0), aL.T @ b["u"], o["part"].S[:-1].sum(0), n)
        assert o["part"].own[:-1].all() and not o["part"].own[-1].any()
        assert ("aLp" in o) == bool(with_alp) and (not with_alp or np.array_equal(F(o["aLp"].val)[:i["nrows"], :i["npc"]], aL))
    i = pc.inputs("estep_moments", case)
    b, o = i["bufs"], pc.reference("estep_moments", i)
    Z = b["Z"][:, :nb]
    assert near(o["lam_m"].val[:n], Z @ b["z1"][:nb], o["lam_m"].S[:n], nb)
    assert near(o["lam_var"].val[:n], b["kv0"][:n] + (Z * Z).sum(1), o["lam_var"].S[:n], nb)


def test_trace_is_the_sum_of_the_diagonal():
    for n in pc.CASES["trace"]:
        i = pc.inputs("trace", n)
        o = pc.reference("trace", i)["out"]
        assert abs(float(o.val[0]) - np.nansum(i["bufs"]["A"])) <= (n + 3) * U53 * float(o.S[0]) and o.own.tolist() == [True, False, False]


def test_a_withheld_term_falls_outside_the_bound():
    """Column nb - 1 of every row sum; row n - 1 of out3, of the trace and of a slice sum of ESTEP_SCALE."""
    def outside(op, case, drop, names):
        inp = pc.inputs(op, case)
        ref, pl = pc.reference(op, inp), pc.evaluate(op, inp, np.float64, drop=drop)
        for name, where in names.items():
            o = ref[name]
            err = np.abs(pl[name].val.astype(LD) - o.val)
            lost = where(inp, o)
            assert lost.any() and o.own[lost].all() and np.all(err[lost] > bound_of(op, o)[lost]), (op, case, name)
    rows = lambda inp, o: np.arange(len(o.val)) < inp["n"]
    for case in pc.SHAPES[1:]:
        outside("moments", case, "col", {"lam_m": rows, "lam_var": rows})
        outside("estep_moments", case, "col", {"lam_m": rows, "lam_var": rows})
        outside("estep_rows", case, "col", {"u": rows})
        outside("moments", case, "row", {"out3": lambda inp, o: o.own, "out3.f": lambda inp, o: o.own})
        outside("estep_scale", case + (0,), "row",
                {"part": lambda inp, o: (np.arange(o.val.shape[0]) == (inp["n"] - 1) // 32)[:, None] & (np.arange(o.val.shape[1]) < inp["nb"])[None, :]})
    for n in pc.CASES["trace"][1:]:
        outside("trace", n, "row", {"out": lambda inp, o: o.own})


def test_no_launch_of_the_cases_reaches_outside_its_buffers():
    """The extents every launcher indexes by, against the shapes of the buffers of a case."""
    for op, case, unit in ALL:
        i = pc.inputs(op, case, unit)
        b = {k: np.asarray(v) for k, v in i["bufs"].items()}
        if op == "trace":
            assert b["A"].shape == (i["n"], i["ld"]) and i["ld"] >= i["n"] and b["out"].size >= 1
            continue
        n, nb, npad, nrows, npc, ld = (i[k] for k in ("n", "nb", "np", "nrows", "npc", "ld"))
        assert npad >= n and nrows >= n and nrows % 32 == 0 and npc >= nb
        for name, v in b.items():
            if v.ndim == 2 and name not in ("Y", "aLp", "part"):
                assert v.shape[1] == i["lda"] >= nb, (op, name)
        rows = {"moments": dict(am=n, Kb=n, aV=n), "ga": dict(Kb=n, aV=n, Ga=npad), "gkb": dict(am=n, GaKi=npad),
                "gktb": dict(Ki=nb, P1=nb, P2=nb, G=nb), "estep_rows": dict(a=n), "estep_scale": dict(aL=n, Y=nrows, part=nrows // 32),
                "estep_moments": dict(Z=n)}[op]
        for name, need in rows.items():
            assert b[name].shape[0] >= need, (op, name)
        lens = {"moments": dict(mb=nb, Kvec=n, r=n, lam_m=n, lam_var=n, f=n, gm=n, gv=n, part=3 * ((n + 3) // 4), out3=3),
                "ga": dict(gm=n, gv=n, mb=nb), "gkb": dict(gv=n), "gktb": dict(bvec=nb),
                "estep_rows": dict(mb=nb, f=n, r=n, sv=nrows, u=nrows), "estep_scale": dict(sv=nrows, u=nrows),
                "estep_moments": dict(z1=nb, kv0=n, lam_m=n, lam_var=n)}[op]
        for name, need in lens.items():
            assert b[name].size >= need, (op, name)
        if op == "estep_scale":
            assert ld >= npc and b["Y"].shape[1] == ld and b["part"].shape[1] == npc and ("aLp" not in b or b["aLp"].shape == b["Y"].shape)
