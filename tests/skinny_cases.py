"""Inputs, the plain references and the bounds shared by the tests of the skinny slab products (csrc/skinny.hip;
test_skinny_cases_cpu.py checks this module, test_gpu_skinny.py checks the launchers with it through the hook
gpfit_dev_skinny).  Pure numpy, in the shape of elementwise_cases.py, whose helpers it imports.

``inputs(op, case)`` gives the seeded operands of one launch as flat buffers with the launcher's arguments beside them
(``bufs``: name -> buffer as uploaded, an output prefilled with the sentinel; ``args``: field of the hook's struct ->
value, a pointer as (buffer, element offset)); ``evaluate(op, inp, T)`` the launcher's outputs in the number type T:
``reference`` in numpy.longdouble, ``plain`` in float64.  An output buffer with parts of different kinds has one
``Out`` per part, named ``buffer.part``; together they own what the launcher writes there.

What the contract says is never read holds NaN: behind a leading dimension and between the elements of a stride-2
operand, in front of a pointer at an odd offset, beyond the diagonal of a triangular op(A) (above the diagonal of the
stored factor, in either storage order), above the diagonal of K22 and in all of K's rows above it, beyond k in the
leaf's tiles, and in every partial of a slab that is not live for its panel.  What is not owned starts as the sentinel.

Bounds: a product's partial and a sum of partials are "sum" -- (k + 2) 2^-53 S with k the terms of the reduction (an
fp64 matrix instruction is a chain of fused multiply-adds: one rounding a term); the zeros of SUM_ROWS, the unit
diagonal of SUM_SCHUR and the triangles of FINISH are "exact"; the log-det of FINISH is a "formula" held to
8 x FLOOR, floored at 2^-53 (``bar``), FLOOR measured on the CPU."""
import numpy as np

from elementwise_cases import (LD, SENTINEL, U53, Out, _exact, _factor, _formula, _mixed, _rng, _summed, check as _ec_check,
                               same_bits)

SLAB, MT, LDT = 256, 64, 128         # kernels.h: SKINNY_SLAB, SKINNY_MT, SKINNY_LD
PLAIN, ROWS, SCHUR = 0, 1, 2         # kernels.h: SkinnySumMode

# The largest scaled error of plain against reference over an op's cases, as measured on the CPU
# (test_skinny_cases_cpu.py asserts it within a factor of two).
FLOOR = {
    "finish": 8.0e-17,
}


def bar(op):
    """The multiple of the 2^-53-floored FLOOR[op] a formula output is held to (the rule of elementwise_cases.bar)."""
    return 8.0 * max(FLOOR[op], U53)


# ------------------------------------------------------------------ the cases
# slabs: (tri, M, K, kc, a, b, o, off, alpha) -- a: which index of op(A) is contiguous ("m": sam == 1, "r": sar == 1,
# "2": neither, element stride 2); b: "c": sbc == 1, "r": sbr == 1, "2"; o: "c": (som, soc) = (ld, 1), "m": (1, ld);
# off: elements in front of all three base pointers
_PAIRS = ((1, 1), (65, 15), (65, 16), (65, 17), (257, 17), (257, 127), (257, 128), (600, 1), (600, 17), (600, 128))
CASES = {
    "slabs": tuple((1, m, m, kc, "r", "c", "c", 0, 1.0) for m, kc in _PAIRS)         # L^-1 K12
    + tuple((2, m, m, kc, "m", "c", "c", 0, 1.0) for m, kc in _PAIRS)                # L^-T Y
    + ((0, 5, 600, 5, "m", "c", "c", 0, 1.0), (0, 128, 257, 128, "m", "c", "c", 0, 1.0),      # Y^T Y
       (0, 130, 40, 17, "r", "r", "c", 0, 1.0),
       (0, 600, 128, 128, "r", "r", "m", 0, -1.0), (0, 600, 128, 128, "r", "r", "c", 0, 1.0))  # -W L22^-T
    + tuple((0, 130, 300, 33, a, b, "c", 0, 1.0) for a in "mr" for b in "cr")
    + ((0, 130, 300, 33, "2", "2", "c", 0, 1.0), (0, 130, 300, 33, "r", "c", "c", 1, 1.0)),
    # sum: (mode, tri, M, kc)
    "sum": ((PLAIN, 2, 600, 17), (ROWS, 1, 600, 17), (ROWS, 1, 257, 128), (SCHUR, 0, 1, 1), (SCHUR, 0, 17, 17),
            (SCHUR, 0, 128, 128)),
    "finish": (1, 17, 128),
}


def slab_live(tri, z, mt0, M, K):
    """Does slab z hold a term of the row panel at mt0?  From the definition: a reduction index r of the slab that the
    triangle keeps for one of the panel's rows."""
    m_lo, m_hi = mt0, min(mt0 + MT, M) - 1
    r_lo, r_hi = z * SLAB, min((z + 1) * SLAB, K) - 1
    if tri == 1:
        return r_lo <= m_hi
    if tri == 2:
        return r_hi >= m_lo
    return True


def n_slabs(K):
    return (K + SLAB - 1) // SLAB


def live_mask(tri, M, K):
    """[nslab][M]: is slab z live for row m's panel."""
    return np.array([[slab_live(tri, z, m // MT * MT, M, K) for m in range(M)] for z in range(n_slabs(K))])


def _strided(a, fast, off=0, fill=np.nan):
    """a[R, C] in a flat buffer with ``off`` elements in front.  fast = 1: rows of C + 3, the column index contiguous;
    fast = 0: columns of R + 3, the row index contiguous; fast = 2: rows of 2 C + 3, element stride 2.  Returns the
    buffer, the position of every element and the two strides."""
    R, C = a.shape
    s0, s1 = {1: (C + 3, 1), 0: (1, R + 3), 2: (2 * C + 3, 2)}[fast]
    size = {1: R * s0, 0: C * s1, 2: R * s0}[fast]
    idx = off + np.arange(R)[:, None] * s0 + np.arange(C)[None, :] * s1
    buf = np.full(off + size, fill)
    buf[idx] = a
    return buf, idx, (s0, s1)


def tri_mask(tri, M, K):
    """What the triangle keeps of op(A)(m, r): 1: r <= m, 2: r >= m."""
    m, r = np.arange(M)[:, None], np.arange(K)[None, :]
    return (r <= m) if tri == 1 else (r >= m) if tri == 2 else np.ones((M, K), bool)


def inputs(op, case, unit=0):
    rng = _rng("skinny", op, case, unit)
    if op == "slabs":
        tri, M, K, kc, a, b, o, off, alpha = case
        keep = tri_mask(tri, M, K)
        opA = np.where(keep, _mixed(rng, M, K) / np.sqrt(K), np.nan)
        B = _mixed(rng, K, kc)
        Abuf, _, (sam, sar) = _strided(opA, {"m": 0, "r": 1, "2": 2}[a], off)
        Bbuf, _, (sbr, sbc) = _strided(B, {"r": 0, "c": 1, "2": 2}[b], off)
        nz = n_slabs(K)
        blk, oidx, (som, soc) = _strided(np.zeros((M, kc)), {"m": 0, "c": 1}[o], 0)
        soz = 0 if nz == 1 else len(blk) + 5
        Obuf = np.full(off + (nz - 1) * soz + len(blk) + 5, SENTINEL)
        return dict(case=case, opA=opA, keep=keep, B=B, alpha=alpha, oidx=off + oidx, soz=soz, nbuf=len(Obuf),
                    bufs={"A": Abuf, "B": Bbuf, "O": Obuf},
                    args=dict(A=("A", off), sam=sam, sar=sar, B=("B", off), sbr=sbr, sbc=sbc, O=("O", off), soz=soz, som=som,
                              soc=soc, alpha=alpha, M=M, K=K, kc=kc, tri=tri))
    if op == "sum":
        mode, tri, M, kc = case
        nz = 3 if mode == SCHUR else n_slabs(M)
        K = nz * SLAB if mode == SCHUR else M
        live = live_mask(tri, M, K)                                 # [nz][M]
        part = np.where(live[:, :, None], _mixed(rng, nz, M, kc), np.nan)
        pz = M * LDT + 5
        P = np.full((nz, pz), np.nan)
        P[:, :M * LDT].reshape(nz, M, LDT)[:, :, :kc] = part
        rows = LDT if mode == SCHUR else M
        i = dict(case=case, part=part, live=live, mode=mode, M=M, kc=kc, nslab=nz,
                 bufs={"P": P, "dst": np.full(rows * LDT + 7, SENTINEL)},
                 args=dict(P=("P", 0), pz=pz, M=M, kc=kc, nslab=nz, tri=tri, mode=mode, dst=("dst", 0)))
        if mode == ROWS:
            n, ldl, ldi = M, M + kc + 2, M + kc + 5
            i["bufs"].update(L=np.full((n + kc, ldl), SENTINEL), Li=np.full((n + kc, ldi), SENTINEL))
            i["args"].update(L=("L", 0), ldl=ldl, Li=("Li", 0), ldi=ldi, n=n)
            i.update(n=n)
        if mode == SCHUR:
            n, ldk = 7, kc + 3
            K22 = _mixed(rng, kc, kc)
            Kc = np.full((n + kc, ldk), np.nan)
            Kc[n:, :kc] = np.where(np.tril(np.ones((kc, kc), bool)), K22, np.nan)   # the lower triangle alone
            i["bufs"].update(Kc=Kc)
            i["args"].update(Kc=("Kc", 0), ldk=ldk, n=n)
            i.update(n=n, K22=np.tril(K22))
        return i
    if op == "finish":
        k, n = case, 5
        ldl, ldi = n + k + 2, n + k + 5
        tiles = {}
        for name in ("Lt", "Lit"):
            t = np.full((LDT, LDT), np.nan)
            t[:k, :k] = np.where(np.tril(np.ones((k, k), bool)), _factor(rng, k), np.nan)
            tiles[name] = t
        return dict(case=case, k=k, n=n, **tiles,
                    bufs={"Lt": tiles["Lt"], "Lit": tiles["Lit"], "L": np.full((n + k, ldl), SENTINEL),
                          "Li": np.full((n + k, ldi), SENTINEL), "logdet": np.full(3, SENTINEL)},
                    args=dict(Lt=("Lt", 0), Lit=("Lit", 0), L=("L", 0), ldl=ldl, Li=("Li", 0), ldi=ldi, n=n, kc=k,
                              logdet=("logdet", 0)))
    raise KeyError(op)


# ------------------------------------------------------------------ the formulas
def slab_products(opA, keep, B, alpha, T):
    """Per slab z: (alpha sum_{r in z} op(A)(m, r) B(r, c), the number of terms, the sum of their magnitudes) over the
    whole M x kc block, with what the triangle drops taken as zero; live[z][m] beside them."""
    M, K = opA.shape
    A = np.where(keep, np.asarray(opA, dtype=T), T(0))
    B = np.asarray(B, dtype=T)
    out = []
    for z in range(n_slabs(K)):
        rs = slice(z * SLAB, min((z + 1) * SLAB, K))
        val = T(alpha) * (A[:, rs] @ B[rs])
        k = np.broadcast_to(keep[:, rs].sum(1)[:, None], val.shape)
        S = np.abs(A[:, rs].astype(LD)) @ np.abs(B[rs].astype(LD))
        out.append((val, k, S))
    return out


def slab_sum(part, live, T):
    """The partials of every (m, c) added in slab order over the live slabs of m's panel: (value, k, S)."""
    p = np.where(live[:, :, None], np.asarray(part, dtype=T), T(0))
    val = np.zeros(p.shape[1:], T)
    for z in range(p.shape[0]):
        val = val + p[z]
    return val, np.broadcast_to(live.sum(0)[:, None], val.shape), np.abs(p.astype(LD)).sum(0)


def _flat(shape, idx, out, fill=SENTINEL):
    """An Out over a block, placed at the positions idx of a buffer of ``shape`` the op does not own elsewhere."""
    val, own = np.full(shape, fill, dtype=out.val.dtype), np.zeros(shape, bool)
    val[idx], own[idx] = np.where(out.own, out.val, val[idx]), out.own
    k = S = None
    if out.k is not None:
        k = np.zeros(shape, np.int64)
        k[idx] = out.k
    if out.S is not None:
        S = np.zeros(shape, LD)
        S[idx] = out.S
    return Out(val, own, out.kind, k, S)


def evaluate(op, i, T):
    """name -> Out of every output buffer (or part of one) of the launcher, computed in the number type T."""
    if op == "slabs":
        tri, M, K, kc = i["case"][:4]
        live = live_mask(tri, M, K)
        prods = slab_products(i["opA"], i["keep"], i["B"], i["alpha"], T)
        val, own = np.full(i["nbuf"], SENTINEL, dtype=T), np.zeros(i["nbuf"], bool)
        k, S = np.zeros(i["nbuf"], np.int64), np.zeros(i["nbuf"], LD)
        for z, (v, kz, Sz) in enumerate(prods):
            idx = (i["oidx"] + z * i["soz"])[live[z]]
            val[idx], own[idx], k[idx], S[idx] = v[live[z]], True, kz[live[z]], Sz[live[z]]
        return {"O": Out(val, own, "sum", k, S)}
    if op == "sum":
        mode, M, kc = i["mode"], i["M"], i["kc"]
        v, k, S = slab_sum(i["part"], i["live"], T)
        blk = lambda rows: (np.arange(rows)[:, None] * LDT + np.arange(kc)[None, :])
        if mode == SCHUR:
            K22 = np.asarray(i["K22"], dtype=T)
            K22 = K22 + np.tril(K22, -1).T
            tile = np.arange(LDT * LDT).reshape(LDT, LDT)
            unit = np.ones((LDT, LDT), bool)
            unit[:kc, :kc] = False
            res = {"dst": _flat(LDT * LDT + 7, tile[:kc, :kc], _summed((K22 - v, k + 1, np.abs(K22.astype(LD)) + S)))}
            if kc < LDT:
                res["dst.unit"] = _flat(LDT * LDT + 7, tile, _exact(np.eye(LDT, dtype=T), unit))
            return res
        res = {"dst": _flat(M * LDT + 7, blk(M), _summed((v, k, S)))}
        if mode == ROWS:
            n = i["n"]
            for name, ld in (("L", i["args"]["ldl"]), ("Li", i["args"]["ldi"])):
                cols = np.arange(M)[:, None] * ld + n + np.arange(kc)[None, :]       # [m][n + c]
                res[name + ".zero"] = _flat((n + kc) * ld, cols, _exact(np.zeros((M, kc), T)))
            rows = (n + np.arange(kc)[None, :]) * i["args"]["ldl"] + np.arange(M)[:, None]   # [n + c][m]
            res["L"] = _flat((n + kc) * i["args"]["ldl"], rows, _summed((v, k, S)))
        return res
    if op == "finish":
        k, n = i["k"], i["n"]
        res = {}
        for name, src, ld in (("L", "Lt", i["args"]["ldl"]), ("Li", "Lit", i["args"]["ldi"])):
            t = np.tril(np.nan_to_num(i[src][:k, :k])).astype(T)
            idx = (n + np.arange(k)[:, None]) * ld + n + np.arange(k)[None, :]
            res[name] = _flat((n + k) * ld, idx, _exact(t))
        terms = T(2) * np.log(np.diag(i["Lt"])[:k].astype(T))
        res["logdet"] = _flat(3, np.arange(1), _formula(terms.sum().reshape(1), np.abs(terms.astype(LD)).sum().reshape(1)))
        return res
    raise KeyError(op)


def reference(op, inp):
    return evaluate(op, inp, LD)


def plain(op, inp):
    return evaluate(op, inp, np.float64)


# ------------------------------------------------------------------ comparison
def buffer_of(name):
    return name.split(".")[0]


def as_buffers(inp, outs):
    """The buffers a launch would leave if it computed ``outs``: the initial ones with every owned element replaced."""
    got = {}
    for buf in {buffer_of(p) for p in outs}:
        g = np.asarray(inp["bufs"][buf], dtype=np.float64).reshape(-1).copy()
        for p, o in outs.items():
            if buffer_of(p) == buf:
                own = o.own.reshape(-1)
                g[own] = np.asarray(o.val, dtype=np.float64).reshape(-1)[own]
        got[buf] = g
    return got


def floor_of(op, cases, inputs_fn, evaluate_fn):
    """The measured floor of a formula op: the largest scaled error of plain against reference over its cases."""
    worst = 0.0
    for case in cases:
        inp = inputs_fn(op, case)
        ref, pl = evaluate_fn(op, inp, LD), evaluate_fn(op, inp, np.float64)
        for name, o in ref.items():
            own = o.own & (o.S > 0) if o.kind == "formula" else None
            if own is not None and own.any():
                worst = max(worst, float((np.abs(pl[name].val.astype(LD) - o.val)[own] / o.S[own]).max()))
    return worst


def check(op, name, got, ref, init, bar_value=None):
    """Compare a downloaded buffer with the Outs of its parts (ref: name -> Out, all of this buffer).  Returns (worst
    error / bound, message or None).  Exact parts, sums and what no part owns go through elementwise_cases.check; a
    formula part is held to bar_value x its scale."""
    got = np.asarray(got).reshape(-1)
    init = np.asarray(init, dtype=got.dtype).reshape(-1)
    owned = np.zeros(got.shape, bool)
    for o in ref.values():
        assert not (owned & o.own.reshape(-1)).any(), f"{op} {name}: two parts own one element"
        owned |= o.own.reshape(-1)
    worst = 0.0
    for part, o in ref.items():
        o = Out(*(None if f is None else np.asarray(f).reshape(-1) for f in o[:2]), o.kind,
                *(None if f is None else np.asarray(f).reshape(-1) for f in o[3:]))
        theirs = owned & ~o.own                          # another part's elements: that part's business
        base = np.where(theirs, got, init)
        if o.kind != "formula":
            ratio, msg = _ec_check(op, part, got, o, base)
        else:
            ratio, msg = _ec_check(op, part, got, Out(o.val, np.zeros(got.shape, bool), "exact", None, None), np.where(o.own, got, base))
            if msg is None and not np.all(np.isfinite(got[o.own])):
                msg = f"{op} {part}: non-finite result"
            if msg is None:
                err, bound = np.abs(got.astype(LD) - o.val), LD(bar_value) * o.S
                bad = o.own & (err > bound)
                if bad.any():
                    j = int(np.argmax(np.where(bad, err - bound, -1)))
                    msg = f"{op} {part}[{j}]: |err| {float(err[j]):.3e} > bound {float(bound[j]):.3e} (got {got[j]!r}, ref {float(o.val[j])!r})"
                pos = o.own & (bound > 0)
                ratio = float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0
        if msg is not None:
            return np.inf, msg
        worst = max(worst, ratio)
    return worst, None


def check_all(op, got, ref, init, bar_value=None):
    """Every buffer of a launch: got, init: buffer -> array; ref: part -> Out.  (worst ratio, first message or None)."""
    worst = 0.0
    for buf in sorted({buffer_of(p) for p in ref}):
        ratio, msg = check(op, buf, got[buf], {p: o for p, o in ref.items() if buffer_of(p) == buf}, init[buf], bar_value)
        if msg is not None:
            return np.inf, msg
        worst = max(worst, ratio)
    return worst, None
