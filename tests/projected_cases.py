"""Inputs, the plain references and the bounds shared by the tests of the element-wise passes of the projected
closures and of the projected E-step (csrc/projected.hip; test_projected_cases_cpu.py checks this module,
test_gpu_projected.py checks the launchers with it through the hook gpfit_dev_projected).  Pure numpy, in the shape of
elementwise_cases.py, whose helpers it imports; an output buffer with parts of different kinds has one ``Out`` per part,
named ``buffer.part`` (skinny_cases.check).

A case is (n, nb): n training points, a basis of nb; np = round_up(n, 128) rows of the closure operands, nrows =
round_up(n, 32) rows of the E-step's, npc = round_up(nb, 128).  Every matrix has the leading dimension nb + 3 with NaN
behind nb (Y, aLp and part of ESTEP_SCALE take the padded npc as their width: npc + 3); rows >= n of the closure operands
hold NaN, as do gm and gv there; of the matrix whose trace is taken the diagonal alone is given.  What the contract
requires holds the required value: sv and u are zero on the rows n .. nrows that ESTEP_SCALE multiplies by.  What is not
owned starts as the sentinel.

Bounds: the row sums lam_m, lam_var, the trace, part of ESTEP_SCALE and out3 are "sum", (k + 2) 2^-53 S with k the terms
of the whole reduction (for out3[0] the n nb products of r_i a_ij m_j) plus the partials it passes through (the lanes of
a wave, the blocks of part); Y is one product, aLp and every zero row exact; what goes through exp or sqrt, and the
products built on it (f, g_m, g_v, sum f, sv, u, G_a, G_Kb, G_K~b), is a "formula" held to 8 x FLOOR[op], floored at
2^-53, with the scale the magnitude of the terms of the element's formula.  A, lam_m and lam_var keep
|A lam_m + A^2/2 lam_var + lambda0| < 5, so the exponential amplifies nothing and the reference alone decides."""
import numpy as np

from elementwise_cases import LD, SENTINEL, U53, _embed, _exact, _formula, _mixed, _padded, _rng, _summed, round_up
from skinny_cases import _flat

# The largest scaled error of plain against reference over an op's cases, as measured on the CPU
# (test_projected_cases_cpu.py asserts it within a factor of two).
FLOOR = {
    "moments": 2.0e-16,
    "ga": 2.8e-16,
    "gkb": 1.9e-16,
    "gktb": 2.7e-16,
    "estep_rows": 2.0e-16,
}

SHAPES = ((1, 1), (5, 63), (130, 65), (130, 200), (257, 384))
CASES = {
    "moments": SHAPES, "ga": SHAPES, "gkb": SHAPES, "gktb": SHAPES, "trace": (1, 5, 130, 257, 600),
    "estep_rows": SHAPES, "estep_scale": tuple(s + (p,) for s in SHAPES for p in (0, 1)),   # p: with aLp
    "estep_moments": SHAPES,
}
GROUP_OPS = ("moments", "ga", "gkb", "gktb", "trace")
# three units in one launch: other data per unit, other A and lambda0, for the trace other n
GROUP_CASES = {"moments": ((130, 65),) * 3, "ga": ((130, 65),) * 3, "gkb": ((130, 65),) * 3, "gktb": ((130, 65),) * 3,
               "trace": (1, 130, 257)}
UNIT_LINK = ((0.7, -0.3), (0.45, 0.2), (1.1, -0.8))      # A, lambda0 of the units
TRACE_LD = 603                                           # common to the units of a trace launch
WAVE = 64


def _vec(v, size, fill=np.nan):
    out = np.full(size, fill)
    out[:len(v)] = v
    return out


def _rows(a, rows, fill=np.nan):
    """a with rows added up to ``rows``."""
    return np.vstack([a, np.full((rows - a.shape[0], a.shape[1]), fill)])


def inputs(op, case, unit=0):
    rng = _rng("projected", op, case, unit)
    A, lambda0 = UNIT_LINK[unit]
    if op == "trace":
        n = case
        M = np.full((n, TRACE_LD), np.nan)
        M[np.arange(n), np.arange(n)] = _mixed(rng, n)
        return dict(case=case, n=n, ld=TRACE_LD, bufs={"A": M, "out": np.full(3, SENTINEL)}, slots=["A", "out"])
    n, nb = case[:2]
    npad, nrows, npc, ld = round_up(n, 128), round_up(n, 32), round_up(nb, 128), nb + 3
    mat = lambda rows, scale=1.0: _padded(_rows(scale * _mixed(rng, n, nb), rows), ld)
    base = dict(case=case, n=n, nb=nb, np=npad, nrows=nrows, npc=npc, ld=ld, lda=ld, A=A, lambda0=lambda0)
    out = lambda *shape: np.full(shape, SENTINEL)
    if op == "moments":
        nblk = (n + 3) // 4
        # (aV at another scale than Kb: two clamped entries of a column never cancel in lam_var)
        bufs = {"am": mat(npad, 1 / np.sqrt(nb)), "Kb": mat(npad), "aV": mat(npad, 1.5), "mb": _vec(0.5 * _mixed(rng, nb), nb + 3),
                "Kvec": _vec(rng.uniform(1.0, 2.0, n), npad), "r": _vec(rng.poisson(1.5, n).astype(np.float64), npad),
                "lam_m": out(npad), "lam_var": out(npad), "f": out(npad), "gm": out(npad), "gv": out(npad),
                "part": out(3 * nblk + 5), "out3": out(5)}
        return dict(base, nblk=nblk, bufs=bufs, slots=["am", "Kb", "aV", "mb", "Kvec", "r", "lam_m", "lam_var", "f", "gm", "gv",
                                                       "part", "out3"])
    if op == "ga":
        bufs = {"Kb": mat(npad), "aV": mat(npad), "gm": _vec(_mixed(rng, n), npad), "gv": _vec(-rng.uniform(0.05, 1.0, n), npad),
                "mb": _vec(_mixed(rng, nb), nb + 3), "Ga": out(npad + 1, ld)}
        return dict(base, bufs=bufs, slots=["Kb", "aV", "gm", "gv", "mb", "Ga"])
    if op == "gkb":
        G = _padded(_rows(_mixed(rng, n, nb), npad + 1, SENTINEL), ld, SENTINEL)     # in place: the product in rows < n
        G[n:npad] = np.where(np.arange(ld) < nb, np.nan, SENTINEL)                    # overwritten with zeros, never read
        bufs = {"am": mat(npad), "gv": _vec(-rng.uniform(0.05, 1.0, n), npad), "GaKi": G}
        return dict(base, bufs=bufs, slots=["am", "gv", "GaKi"])
    if op == "gktb":
        sq = lambda: _padded(_mixed(rng, nb, nb), ld)
        bufs = {"Ki": sq(), "P1": sq(), "P2": sq(), "bvec": _vec(_mixed(rng, nb), nb + 3), "G": out(nb + 1, ld)}
        return dict(base, bufs=bufs, slots=["Ki", "P1", "P2", "bvec", "G"])
    if op == "estep_rows":
        bufs = {"a": _padded(_mixed(rng, n, nb) / np.sqrt(nb), ld), "mb": _vec(_mixed(rng, nb), nb + 3),
                "f": _vec(rng.uniform(0.05, 3.0, n), nrows), "r": _vec(rng.poisson(1.5, n).astype(np.float64), nrows),
                "sv": out(nrows + 3), "u": out(nrows + 3)}
        return dict(base, bufs=bufs, slots=["a", "mb", "f", "r", "sv", "u"])
    if op == "estep_scale":
        ldy = npc + 3
        bufs = {"aL": _padded(_mixed(rng, n, nb), ld), "sv": _vec(rng.uniform(0.1, 1.5, n), nrows, 0.0),
                "u": _vec(_mixed(rng, n), nrows, 0.0), "Y": out(nrows + 1, ldy), "part": out(nrows // 32 + 1, npc)}
        if case[2]:
            bufs["aLp"] = out(nrows + 1, ldy)
        return dict(base, ld=ldy, bufs=bufs, slots=["aL", "sv", "u", "Y", "aLp", "part"])
    if op == "estep_moments":
        bufs = {"Z": _padded(_mixed(rng, n, nb) / np.sqrt(nb), ld), "z1": _vec(_mixed(rng, nb), nb + 3),
                "kv0": _vec(rng.uniform(0.5, 1.5, n), n + 3), "lam_m": out(n + 3), "lam_var": out(n + 3)}
        return dict(base, bufs=bufs, slots=["Z", "z1", "kv0", "lam_m", "lam_var"])
    raise KeyError(op)


# ------------------------------------------------------------------ the formulas
def _rowsum(terms, T):
    """(value, k, S) of the sums along the rows of ``terms``: k counts the terms and the partials they pass through (a
    wave's 64 lanes, for at most two accumulators)."""
    terms = np.asarray(terms, dtype=T)
    k = terms.shape[1] + min(terms.shape[1], 2 * WAVE)
    return terms.sum(axis=1), np.full(terms.shape[0], k), np.abs(terms.astype(LD)).sum(axis=1)


def _top(out, shape):
    """An Out over a block at the top left of a buffer of ``shape`` the op does not own elsewhere."""
    return _embed(out, shape)


def _at(size, j, out):
    """An Out of one element at position j of a vector of ``size``."""
    return _flat(size, np.array([j]), out)


def moment_terms(i, T, drop_col=None):
    """lam_m and lam_var of MOMENTS, each as (value, k, S), from the operands in T (drop_col: a column withheld)."""
    n, nb = i["n"], i["nb"]
    b = i["bufs"]
    g = lambda k_: np.asarray(b[k_], dtype=T)
    am, Kb, aV = (g(k_)[:n, :nb] for k_ in ("am", "Kb", "aV"))
    mb = g("mb")[:nb]
    cols = np.arange(nb) != drop_col
    lm = _rowsum((am * mb[None, :])[:, cols], T)
    lv = _rowsum(np.concatenate([g("Kvec")[:n, None], -(am * Kb)[:, cols], (aV * am)[:, cols]], axis=1), T)
    return lm, lv


def evaluate(op, i, T, drop=None):
    """name -> Out of every output buffer (or part of one) of the launcher, computed in the number type T.  ``drop``
    withholds one term (the CPU test of the bounds): "col": column nb - 1 of the row sums, "row": row n - 1 of the sums
    over the training points."""
    b = i["bufs"]
    g = lambda k_: np.asarray(b[k_], dtype=T)
    if op == "trace":
        n = i["n"] - (drop == "row")
        d = g("A")[np.arange(n), np.arange(n)]
        return {"out": _top(_summed((d.sum().reshape(1), np.array([n + min(n, 256)]), np.abs(d.astype(LD)).sum().reshape(1))), (3,))}
    n, nb, npad, nrows, npc = i["n"], i["nb"], i["np"], i["nrows"], i["npc"]
    A, l0 = T(i["A"]), T(i["lambda0"])
    last = nb - 1 if drop == "col" else None
    cols = np.arange(nb) != last
    if op == "moments":
        lm, lv = moment_terms(i, T, last)
        r = g("r")[:n]
        arg = A * lm[0] + T(0.5) * A * A * lv[0] + l0
        f = np.exp(arg)
        s_f = np.abs(f) * (T(1) + np.abs(A) * lm[2] + T(0.5) * A * A * lv[2] + abs(l0))
        nblk = i["nblk"]
        rows = np.arange(n) < n - (drop == "row")
        blocks = lambda v: np.array([np.where(rows, v, 0)[4 * q:4 * q + 4].sum() for q in range(nblk)], dtype=v.dtype)
        terms3 = [r * lm[0], r, f]
        scale3 = [np.abs(r) * lm[2], np.abs(r).astype(LD), s_f]
        part = np.concatenate([blocks(np.asarray(t, dtype=T)) for t in terms3])
        part_S = np.concatenate([blocks(np.asarray(s, dtype=LD)) for s in scale3])
        tot = lambda v: np.where(rows, v, 0).sum()
        kk = rows.sum() + nblk
        return {"lam_m": _top(_summed(lm), (npad,)), "lam_var": _top(_summed(lv), (npad,)),
                "f": _top(_formula(f, s_f), (npad,)), "gm": _top(_formula(A * (r - f), np.abs(A) * (np.abs(r) + s_f)), (npad,)),
                "gv": _top(_formula(T(-0.5) * A * A * f, T(0.5) * A * A * s_f), (npad,)),
                "part": _top(_formula(part, part_S), (3 * nblk + 5,)),
                "out3": _top(_summed((np.array([tot(terms3[0]), tot(terms3[1])]), np.array([rows.sum() * lm[1][0] + nblk, kk]),
                                      np.array([tot(scale3[0]), tot(scale3[1])]))), (5,)),
                "out3.f": _at(5, 2, _formula(np.array([tot(f)]), np.array([tot(s_f)])))}
    if op == "ga":
        gm, gv, mb = g("gm")[:n, None], g("gv")[:n, None], g("mb")[None, :nb]
        Kb, aV = g("Kb")[:n, :nb], g("aV")[:n, :nb]
        val = gm * mb - gv * Kb + T(2) * gv * aV
        scale = np.abs(gm * mb) + np.abs(gv * Kb) + T(2) * np.abs(gv * aV)
        zero = np.zeros((npad, nb), bool)
        zero[n:] = True
        return {"Ga": _top(_formula(val, scale), (npad + 1, i["ld"])),
                "Ga.zero": _top(_exact(np.zeros((npad, nb), T), zero), (npad + 1, i["ld"]))}
    if op == "gkb":
        gv, am, G = g("gv")[:n, None], g("am")[:n, :nb], g("GaKi")[:n, :nb]
        zero = np.zeros((npad, nb), bool)
        zero[n:] = True
        return {"GaKi": _top(_formula(gv * am - G, np.abs(gv * am) + np.abs(G)), (npad + 1, i["ld"])),
                "GaKi.zero": _top(_exact(np.zeros((npad, nb), T), zero), (npad + 1, i["ld"]))}
    if op == "gktb":
        Ki, P1, P2 = (g(k_)[:, :nb] for k_ in ("Ki", "P1", "P2"))
        bb = g("bvec")[:nb, None] * g("bvec")[None, :nb]
        h = T(0.5)
        return {"G": _top(_formula(h * Ki - h * bb - h * P1 + P2, h * np.abs(Ki) + h * np.abs(bb) + h * np.abs(P1) + np.abs(P2)),
                          (nb + 1, i["ld"]))}
    if op == "estep_rows":
        lam = _rowsum((g("a")[:, :nb] * g("mb")[None, :nb])[:, cols], T)
        f, r = g("f")[:n], g("r")[:n]
        sv = A * np.sqrt(f)
        u = A * A * f * lam[0] + A * (r - f)
        pad = np.arange(nrows) >= n
        z = lambda: _top(_exact(np.zeros(nrows, T), pad), (nrows + 3,))
        return {"sv": _top(_formula(sv, np.abs(sv)), (nrows + 3,)), "sv.zero": z(),
                "u": _top(_formula(u, A * A * np.abs(f) * lam[2] + np.abs(A) * (np.abs(r) + np.abs(f))), (nrows + 3,)), "u.zero": z()}
    if op == "estep_scale":
        aL = np.zeros((nrows, npc), T)
        aL[:n, :nb] = g("aL")[:, :nb]
        if drop == "row":
            aL[n - 1] = 0
        sv, u = g("sv")[:, None], g("u")[:, None]
        data = np.zeros((nrows, npc), bool)
        data[:n, :nb] = True
        ldy = i["ld"]
        Y = sv * aL
        terms = (aL * u).reshape(nrows // 32, 32, npc)
        part = (terms.sum(1), (terms != 0).sum(1), np.abs(terms.astype(LD)).sum(1))
        res = {"Y": _top(_summed((Y, np.ones(Y.shape, np.int64), np.abs(Y.astype(LD))), data), (nrows + 1, ldy)),
               "Y.zero": _top(_exact(np.zeros((nrows, npc), T), ~data), (nrows + 1, ldy)),
               "part": _top(_summed(part), (nrows // 32 + 1, npc))}
        if "aLp" in b:
            res["aLp"] = _top(_exact(aL), (nrows + 1, ldy))
        return res
    if op == "estep_moments":
        Z, z1 = g("Z")[:, :nb], g("z1")[None, :nb]
        lm = _rowsum((Z * z1)[:, cols], T)
        lv = _rowsum(np.concatenate([g("kv0")[:n, None], (Z * Z)[:, cols]], axis=1), T)
        return {"lam_m": _top(_summed(lm), (n + 3,)), "lam_var": _top(_summed(lv), (n + 3,))}
    raise KeyError(op)


def reference(op, inp):
    return evaluate(op, inp, LD)


def plain(op, inp):
    return evaluate(op, inp, np.float64)


def bar(op):
    """The multiple of the 2^-53-floored FLOOR[op] a formula output is held to (the rule of elementwise_cases.bar); an
    op without a formula output never uses it."""
    return 8.0 * max(FLOOR.get(op, 0.0), U53)
