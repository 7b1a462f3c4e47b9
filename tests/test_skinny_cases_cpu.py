"""Pins skinny_cases.py, the reference behind test_gpu_skinny.py, so that it cannot be wrong in the same way as the
kernels:

  - the fp64 evaluation of every case lies within the bounds the kernels are held to, and no NaN of the unread parts
    reaches a reference;
  - the slab products, added over their slabs, are the dense triangular products of numpy; the liveness of a slab, taken
    from its definition, is the closed form both launches enumerate by (kernels.h: skinny_slab_live);
  - the five stages of gpfit_potrf_append_block, chained in longdouble from these references, reproduce the longdouble
    Cholesky factor of the grown matrix and its inverse: the references restate the call;
  - the bounds discriminate: with one term withheld -- the diagonal term of a triangular product, the last row of the
    ragged slab, one whole live slab of a sum -- every element that lost it falls outside its bound;
  - the FLOOR table holds the measured floor."""
import numpy as np
import pytest

import potrf_cases as pcs
import skinny_cases as sc
from elementwise_cases import LD, SENTINEL, U53

F = lambda a: np.asarray(a, dtype=np.float64)
ALL = [(op, case) for op in sc.CASES for case in sc.CASES[op]]


def outside(pl, ref, lost):
    """Is every element of ``lost`` outside the sum bound of ``ref``?"""
    err = np.abs(pl.val.astype(LD) - ref.val)
    bound = (ref.k + 2) * LD(U53) * ref.S
    assert lost.any() and ref.own[lost].all()
    return bool(np.all(err[lost] > bound[lost]))


@pytest.mark.parametrize("op,case", ALL, ids=[f"{op}-{case}" for op, case in ALL])
def test_plain_lies_within_the_bounds_and_nothing_unread_leaks(op, case):
    inp = sc.inputs(op, case)
    ref, pl = sc.reference(op, inp), sc.plain(op, inp)
    for name, o in ref.items():
        assert np.all(np.isfinite(F(o.val))), (op, case, name)
        assert o.own.any() and np.all(F(o.val)[~o.own] == SENTINEL)
    worst, msg = sc.check_all(op, sc.as_buffers(inp, pl), ref, inp["bufs"], sc.bar("finish"))
    assert msg is None, msg
    print(f"{op} {case}: worst error / bound {worst:.3f}")
    # an untouched output does not pass: the sentinel is no result
    _, msg = sc.check_all(op, {b: inp["bufs"][b] for b in sc.as_buffers(inp, pl)}, ref, inp["bufs"], sc.bar("finish"))
    assert msg is not None


def test_floor_table_holds_the_measured_floor():
    measured, recorded = sc.floor_of("finish", sc.CASES["finish"], sc.inputs, sc.evaluate), sc.FLOOR["finish"]
    print(f"floor finish: measured {measured:.3e} recorded {recorded:.3e}")
    assert max(recorded, U53) / 2.0 <= max(measured, U53) <= 2.0 * max(recorded, U53)
    kinds = {op: {o.kind for case in sc.CASES[op] for o in sc.plain(op, sc.inputs(op, case)).values()} for op in sc.CASES}
    assert [op for op in sc.CASES if "formula" in kinds[op]] == sorted(sc.FLOOR)


def test_liveness_from_the_definition_is_the_rule_of_the_launches():
    """kernels.h: tri 1: z SLAB < mt0 + MT; tri 2: (z + 1) SLAB > mt0; over every size of the cases and a few more."""
    for M in (1, 63, 64, 65, 255, 256, 257, 512, 513, 600, 1000):
        for tri in (0, 1, 2):
            for z in range(sc.n_slabs(M)):
                for mt0 in range(0, M, sc.MT):
                    rule = z * sc.SLAB < mt0 + sc.MT if tri == 1 else (z + 1) * sc.SLAB > mt0 if tri == 2 else True
                    assert sc.slab_live(tri, z, mt0, M, M) == rule, (M, tri, z, mt0)
    # 600: three slabs, ten panels, and panels with one, two and three live slabs in both triangles
    for tri in (1, 2):
        live = sc.live_mask(tri, 600, 600)
        assert live.shape == (3, 600) and set(live.sum(0)) == {1, 2, 3} and 600 % sc.MT != 0 and 600 % sc.SLAB != 0


def test_slab_products_add_up_to_the_dense_triangular_product():
    """Over the live slabs (slab_sum) the partials are tril(A) B, triu(A) B and A B of numpy in float64."""
    for case in sc.CASES["slabs"]:
        inp = sc.inputs("slabs", case)
        tri, M, K, kc = case[:4]
        A = np.nan_to_num(inp["opA"])
        assert np.array_equal(A, np.tril(A) if tri == 1 else np.triu(A) if tri == 2 else A)
        prods = sc.slab_products(inp["opA"], inp["keep"], inp["B"], inp["alpha"], LD)
        live = sc.live_mask(tri, M, K)
        part = np.stack([np.where(live[z][:, None], v, np.nan) for z, (v, _, _) in enumerate(prods)])   # dead: never read
        total, k, S = sc.slab_sum(part, live, LD)
        assert np.all(np.isfinite(F(total)))
        assert np.all(np.abs(F(total) - inp["alpha"] * (A @ inp["B"])) <= (K + 3) * U53 * F(sum(p[2] for p in prods)))
        # every term of a row lies in a live slab: the counts add up to the triangle's
        count = sum(np.where(live[z], kz[:, 0], 0) for z, (_, kz, _) in enumerate(prods))
        assert np.array_equal(count, inp["keep"].sum(1))
        # and the launch owns exactly the live (slab, row) pairs, kc columns each
        assert sc.reference("slabs", inp)["O"].own.sum() == live.sum() * kc


def test_layouts_place_the_operands_where_the_strides_say():
    for case in sc.CASES["slabs"]:
        inp = sc.inputs("slabs", case)
        a = inp["args"]
        tri, M, K, kc = case[:4]
        for m, r, c in ((0, 0, 0), (M - 1, K - 1, kc - 1), (M // 2, K // 3, kc // 2)):
            got = inp["bufs"]["A"][a["A"][1] + m * a["sam"] + r * a["sar"]]
            assert got == inp["opA"][m, r] or (np.isnan(got) and not inp["keep"][m, r])
            assert inp["bufs"]["B"][a["B"][1] + r * a["sbr"] + c * a["sbc"]] == inp["B"][r, c]
            assert inp["oidx"][m, c] == a["O"][1] + m * a["som"] + c * a["soc"]
        assert (a["sam"] == 1) == (case[4] == "m") and (a["sar"] == 1) == (case[4] == "r")
        assert (a["sbc"] == 1) == (case[5] == "c") and (a["sbr"] == 1) == (case[5] == "r")
        assert np.isnan(inp["bufs"]["A"]).sum() >= (~inp["keep"]).sum() + 3


def test_a_withheld_diagonal_term_falls_outside_the_bound():
    for tri in (1, 2):
        case = next(c for c in sc.CASES["slabs"] if c[:4] == (tri, 600, 600, 17))
        inp = sc.inputs("slabs", case)
        ref = sc.reference("slabs", inp)["O"]
        less = dict(inp, keep=inp["keep"] & ~np.eye(600, dtype=bool))          # r == m masked out as well
        pl = sc.plain("slabs", less)["O"]
        lost = np.zeros(inp["nbuf"], bool)
        for m in range(600):
            lost[inp["oidx"][m] + (m // sc.SLAB) * inp["soz"]] = True          # the slab that holds r = m
        assert outside(pl, ref, lost), tri
        # and one masked in: the first entry beyond the diagonal taken as 0.05 where the contract says zero
        more = dict(inp, keep=inp["keep"] | (np.eye(600, k=1 if tri == 1 else -1, dtype=bool)),
                    opA=np.where(inp["keep"], inp["opA"], 0.05))
        pl = sc.plain("slabs", more)["O"]
        rows = np.arange(599) if tri == 1 else np.arange(1, 600)
        lost = np.zeros(inp["nbuf"], bool)
        for m in rows:
            z = (m + (1 if tri == 1 else -1)) // sc.SLAB
            if sc.slab_live(tri, z, m // sc.MT * sc.MT, 600, 600):
                lost[inp["oidx"][m] + z * inp["soz"]] = True
        err = np.abs(pl.val.astype(LD) - ref.val)
        assert np.all(err[lost] > ((ref.k + 2) * LD(U53) * ref.S)[lost])


def test_a_withheld_last_row_of_the_ragged_slab_falls_outside_the_bound():
    for case in [c for c in sc.CASES["slabs"] if c[2] % sc.SLAB > 1 and c[3] <= 33]:
        inp = sc.inputs("slabs", case)
        tri, M, K, kc = case[:4]
        ref = sc.reference("slabs", inp)["O"]
        B = inp["B"].copy()
        B[K - 1] = 0.0
        pl = sc.plain("slabs", dict(inp, B=B))["O"]
        z = (K - 1) // sc.SLAB
        lost = np.zeros(inp["nbuf"], bool)
        for m in range(M):
            if inp["keep"][m, K - 1]:
                lost[inp["oidx"][m] + z * inp["soz"]] = True
        assert outside(pl, ref, lost), case


def test_a_withheld_live_slab_falls_outside_the_bound_of_the_sum():
    for case in sc.CASES["sum"]:
        inp = sc.inputs("sum", case)
        ref = sc.reference("sum", inp)
        for z in range(inp["nslab"]):
            part = inp["part"].copy()
            part[z] = 0.0
            pl = sc.plain("sum", dict(inp, part=part))
            rows = inp["live"][z]
            for name in ("dst", "L"):
                if name not in ref:
                    continue
                lost = np.zeros(ref[name].own.shape, bool).reshape(-1)
                ld = sc.LDT if name == "dst" else inp["args"]["ldl"]
                for m in np.flatnonzero(rows):
                    pos = m * ld + np.arange(inp["kc"]) if name == "dst" else (inp["n"] + np.arange(inp["kc"])) * ld + m
                    lost[pos] = True
                assert outside(pl[name], ref[name], lost.reshape(ref[name].own.shape)), (case, z, name)


def test_the_sum_never_reads_a_dead_slab_and_owns_what_the_contract_says():
    for case in sc.CASES["sum"]:
        inp = sc.inputs("sum", case)
        mode, tri, M, kc = case
        ref = sc.reference("sum", inp)
        dead = ~inp["live"]
        assert np.isnan(inp["part"][dead]).all() and (tri == 0 or dead.any())
        if mode == sc.ROWS:
            n, ldl, ldi = inp["n"], inp["args"]["ldl"], inp["args"]["ldi"]
            assert ldl != ldi and min(ldl, ldi) > n + kc
            L = (ref["L"].own | ref["L.zero"].own).reshape(n + kc, ldl)
            want = np.zeros_like(L)
            want[n:n + kc, :M] = True
            want[:M, n:n + kc] = True
            assert np.array_equal(L, want)
            Li = ref["Li.zero"].own.reshape(n + kc, ldi)
            want = np.zeros_like(Li)
            want[:M, n:n + kc] = True
            assert np.array_equal(Li, want)
            # L21 = Y^T
            Y = F(ref["dst"].val)[:M * sc.LDT].reshape(M, sc.LDT)[:, :kc]
            assert np.array_equal(F(ref["L"].val).reshape(n + kc, ldl)[n:, :M], Y.T)
        if mode == sc.SCHUR:
            unit = ref["dst.unit"] if kc < sc.LDT else ref["dst"]._replace(own=np.zeros_like(ref["dst"].own))
            both = ref["dst"].own | unit.own
            assert both[:sc.LDT * sc.LDT].all() and not both[sc.LDT * sc.LDT:].any()
            D = F(np.where(ref["dst"].own, ref["dst"].val, unit.val))[:sc.LDT * sc.LDT].reshape(sc.LDT, sc.LDT)
            assert np.array_equal(D[kc:, kc:], np.eye(sc.LDT - kc)) and not D[kc:, :kc].any() and not D[:kc, kc:].any()
            assert np.isnan(inp["bufs"]["Kc"][:inp["n"]]).all() and np.isnan(inp["bufs"]["Kc"][inp["n"]:, :kc][np.triu_indices(kc, 1)]).all()


def test_the_five_stages_chained_reproduce_the_cholesky_factor_of_the_grown_matrix():
    """(n0, k) = (257, 17) in longdouble: Y = L^-1 K12, S = K22 - Y^T Y, its factor, W = L^-T Y, [L^-1]21 = -L22^-1 W^T
    and the finish pass, each by the function behind the references above, against the longdouble factorisation of the
    whole matrix."""
    n, k = 257, 17
    N = n + k
    G = sc._mixed(sc._rng("composite"), N, N)
    S = (G @ G.T + N * np.eye(N)).astype(LD)
    whole = pcs._reference_longdouble(S, True)
    lead = pcs._reference_longdouble(S[:n, :n], True)
    Li0 = np.where(sc.tri_mask(1, n, n), lead.Linv, np.nan)                       # nothing above the diagonal
    total = lambda opA, keep, B, tri, alpha=1.0: sc.slab_sum(
        np.stack([np.where(sc.live_mask(tri, *opA.shape)[z][:, None], v, np.nan)
                  for z, (v, _, _) in enumerate(sc.slab_products(opA, keep, B, alpha, LD))]), sc.live_mask(tri, *opA.shape), LD)[0]
    Y = total(Li0, sc.tri_mask(1, n, n), S[:n, n:], 1)                             # stage 1
    YtY = total(Y.T, sc.tri_mask(0, k, n), Y, 0)                                   # stage 2
    K22 = np.tril(S[n:, n:])
    Sc = (K22 + np.tril(K22, -1).T) - YtY
    leaf = pcs._reference_longdouble(Sc, True)                                     # stage 3: the leaf
    W = total(Li0.T, sc.tri_mask(2, n, n), Y, 2)                                   # stage 4
    Li21 = total(W, sc.tri_mask(0, n, k), leaf.Linv.T, 0, -1.0).T                  # stage 5: out(m = j, c = a), stored transposed
    L = np.zeros((N, N), LD)
    Li = np.zeros((N, N), LD)
    L[:n, :n], Li[:n, :n] = lead.L, lead.Linv
    L[n:, :n], L[n:, n:] = Y.T, np.tril(leaf.L)
    Li[n:, :n], Li[n:, n:] = Li21, np.tril(leaf.Linv)
    eps = float(np.finfo(LD).eps)
    assert np.all(np.isfinite(F(L))) and np.all(np.isfinite(F(Li)))
    assert float(np.max(np.abs(L - whole.L))) <= 64 * N * eps * float(np.max(np.abs(whole.L)))
    assert float(np.max(np.abs(Li - whole.Linv))) <= 4096 * N * eps * float(np.max(np.abs(whole.Linv)))
    assert float(np.max(np.abs(Li @ whole.L - np.eye(N)))) <= 4096 * N * eps
    logdet = lead.logdet + float(2 * np.sum(np.log(np.diag(leaf.L))))
    assert abs(logdet - whole.logdet) <= 1e-13 * abs(whole.logdet)


def test_finish_takes_the_lower_triangles_and_twice_the_log_of_the_diagonal():
    for k in sc.CASES["finish"]:
        inp = sc.inputs("finish", k)
        ref = sc.reference("finish", inp)
        n = inp["n"]
        for name, src in (("L", "Lt"), ("Li", "Lit")):
            ld = inp["args"]["ld" + name[1:].lower() if name == "Li" else "ldl"]
            own = ref[name].own.reshape(n + k, ld)
            want = np.zeros_like(own)
            want[n:, n:n + k] = True
            assert np.array_equal(own, want)
            blk = F(ref[name].val).reshape(n + k, ld)[n:, n:n + k]
            assert np.array_equal(blk, np.tril(np.nan_to_num(inp[src][:k, :k]))) and np.isnan(inp[src]).sum() == 128 * 128 - k * (k + 1) // 2
        d = np.diag(inp["Lt"])[:k]
        assert abs(float(ref["logdet"].val[0]) - 2 * np.log(d).sum()) <= 1e-13 * max(1.0, float(ref["logdet"].S[0]))


def test_no_launch_of_the_cases_reaches_outside_its_buffers():
    """The largest index every launcher forms from the arguments of a case, against the size of the buffer behind it."""
    for case in sc.CASES["slabs"]:
        inp = sc.inputs("slabs", case)
        a, size = inp["args"], {k: np.asarray(v).size for k, v in inp["bufs"].items()}
        tri, M, K, kc = case[:4]
        assert a["A"][1] + (M - 1) * a["sam"] + (K - 1) * a["sar"] < size["A"]
        assert a["B"][1] + (K - 1) * a["sbr"] + (kc - 1) * a["sbc"] < size["B"]
        assert a["O"][1] + (sc.n_slabs(K) - 1) * a["soz"] + (M - 1) * a["som"] + (kc - 1) * a["soc"] < size["O"]
        assert (a["M"], a["K"], a["kc"], a["tri"]) == (M, K, kc, tri) and 1 <= kc <= sc.LDT
    for case in sc.CASES["sum"]:
        inp = sc.inputs("sum", case)
        a, size = inp["args"], {k: np.asarray(v).size for k, v in inp["bufs"].items()}
        mode, tri, M, kc = case
        assert (a["nslab"] - 1) * a["pz"] + (M - 1) * sc.LDT + kc - 1 < size["P"]
        assert (sc.LDT * sc.LDT if mode == sc.SCHUR else (M - 1) * sc.LDT + kc) <= size["dst"]
        if mode == sc.ROWS:
            for name, ld in (("L", a["ldl"]), ("Li", a["ldi"])):
                assert max((a["n"] + kc - 1) * ld + M - 1, (M - 1) * ld + a["n"] + kc - 1) < size[name]
        if mode == sc.SCHUR:
            assert M == kc and (a["n"] + kc - 1) * a["ldk"] + kc - 1 < size["Kc"]
    for k in sc.CASES["finish"]:
        inp = sc.inputs("finish", k)
        a, size = inp["args"], {name: np.asarray(v).size for name, v in inp["bufs"].items()}
        assert size["Lt"] == size["Lit"] == sc.LDT * sc.LDT and size["logdet"] >= 1
        assert (a["n"] + k - 1) * a["ldl"] + a["n"] + k - 1 < size["L"] and (a["n"] + k - 1) * a["ldi"] + a["n"] + k - 1 < size["Li"]
