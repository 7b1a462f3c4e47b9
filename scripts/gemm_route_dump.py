"""Dump what the GEMM launcher decides over a fixed grid of launches.  Host only: no GPU call.

    python scripts/gemm_route_dump.py [OUT.txt]

One line per grid point: the query, every field of gpfit_dev_gemm_route_t and, for a launch on a balanced schedule
(XCD-aware table, stream-K), the SHA-256 of the plan gpfit_dev_gemm_plan hands out (for the k_slabs route: of the
slab plan).  Run it at two commits and compare the files (or the digest printed at the end) to show that a change of
the launcher's host code decides every launch as before.  GPFIT_* tuning knobs are removed from the environment
first: the grid is laid around the thresholds of the default build.

The grid is a union of sweeps, not one cartesian product (that would be 10^9 points): every dimension is swept in
full against the shapes, in the company of the dimensions it interacts with."""
import ctypes
import hashlib
import itertools
import os
import sys

for k in [k for k in os.environ if k.startswith("GPFIT_")]:
    del os.environ[k]
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from gaussian_processes_amd import _lib                      # noqa: E402
from gaussian_processes_amd.build import build_library       # noqa: E402

# whole and ragged sizes on 128-, 64- and 32-tiles, on both sides of every threshold of the default build: 384
# 128-tiles (2560^2 = 400 | 2048 x 2560 = 320; lower 3584 = 406 | 3456 = 378), 256 64-tiles (1024^2 | 960 x 1024), the
# 32-tile limit 1024 (1152 x 512), 512 workgroups for the deep pipeline (1024^2 = 256 | 1536^2 = 576 64-tiles), the
# stream-K tail (2944^2 = 512 + 17 | 3840^2 = 512 + 388 | 4096^2 = 2 x 512), the XCD-aware table at 1536 tiles
# (5120^2 = 1600 | 4992^2 = 1521; lower 7040 = 1540 | 6912 = 1485)
SQUARES = (32, 64, 96, 128, 160, 200, 256, 512, 1000, 1024, 1056, 1536, 2048, 2560, 2944, 3456, 3584, 3712, 3840, 4096,
           4992, 5120, 6912, 7040, 8192, 10240, 10300)
RECTS = ((2048, 2560), (2560, 2048), (960, 1024), (1152, 512), (512, 8192), (8192, 512), (4096, 2048), (1000, 616),
         (10240, 1024), (3072, 5120), (64, 4096), (4096, 8192))
SHAPES = tuple((n, n) for n in SQUARES) + RECTS
SOME = tuple((n, n) for n in (64, 200, 512, 1024, 2048, 2560, 2944, 3584, 3712, 4096, 5120, 7040, 8192)) + \
    ((2048, 2560), (1000, 616), (4096, 8192))
KS = (256, 1024, 4096, 8192)
TRIS = tuple(itertools.product((0, 1, 2), repeat=2))
FIELDS = [n for n, _ in _lib.DevGemmRoute._fields_]
NAMES = ("M", "N", "K", "lda", "out_lower", "a_tri", "b_tri", "a_kmajor", "b_kmajor", "walk", "tile", "split_k", "batch",
         "nptr", "epi", "aux", "sumsq", "k_slabs")

PTRS = (ctypes.c_void_p * 32)(*([0x1000] * 32))   # host arrays of a pointer batch; the hooks never follow the entries
PTR_FIELDS = ("Ap", "Bp", "Cp", "auxp", "sumsqp")


def args_of(q):
    kw = {"lda": q["K"], "ldb": q["K"], "ldc": q["N"], "alpha": 1.0, "batch": 1, "split_k": 1, **q}
    if kw.get("nptr", 0) > 0:
        for f in PTR_FIELDS:
            kw[f] = ctypes.cast(PTRS, ctypes.c_void_p)
    return _lib.DevGemmArgs(**kw)


def grid():
    """(is_f32, query, pair query or None)"""
    for f32, (M, N), K in itertools.product((0, 1), SHAPES, KS):
        base = {"M": M, "N": N, "K": K}
        lowers = (0, 1) if M == N else (0,)
        # 1. structure x every walk, with and without the half-occupancy bit (16)
        for lower, (at, bt), walk in itertools.product(lowers, TRIS, range(32)):
            yield f32, {**base, "out_lower": lower, "a_tri": at, "b_tri": bt, "walk": walk}, None
        # 2. forced tiles, split-K, strided batches (and a lower output that is not square: refused)
        for lower, (at, bt), walk, tile, split, batch in itertools.product(
                (0, 1), ((0, 0), (1, 1), (2, 0), (0, 1)), (0, 8, 11, 16), (0, 32, 64, 128), (1, 4), (1, 3)):
            yield f32, {**base, "out_lower": lower, "a_tri": at, "b_tri": bt, "walk": walk, "tile": tile, "split_k": split,
                        "batch": batch}, None
        # 3. pointer batches (33: one more than a launch holds; with split-K: refused)
        if K in (256, 1024):
            for lower, (at, bt), nptr, tile, split, walk in itertools.product(lowers, TRIS, (0, 2, 7, 33), (0, 32, 64, 128),
                                                                              (1, 4), (0, 24)):
                yield f32, {**base, "out_lower": lower, "a_tri": at, "b_tri": bt, "nptr": nptr, "tile": tile, "split_k": split,
                            "walk": walk}, None
    # 4. fused epilogues with and without their operands, on every schedule and where they are refused
    for f32, (M, N), K in itertools.product((0, 1), SOME, (1024, 4096)):
        for lower, epi, aux, sumsq, ak, bk, tile, walk, nptr, (at, bt) in itertools.product(
                (0, 1) if M == N else (0,), (1, 2, 4), (0, 1), (0, 1), (0, 1), (0, 1), (0, 128), (0, 8, 16), (0, 2),
                ((0, 0), (1, 1), (2, 2))):
            yield f32, {"M": M, "N": N, "K": K, "out_lower": lower, "epi": epi, "aux": aux, "sumsq": sumsq, "a_kmajor": ak,
                        "b_kmajor": bk, "tile": tile, "walk": walk, "nptr": nptr, "a_tri": at, "b_tri": bt}, None
        for epi, split, batch, slabs, tile in itertools.product((0, 1, 2, 4), (1, 4), (1, 3), (0, 2), (0, 32, 64, 128)):
            yield f32, {"M": M, "N": N, "K": K, "out_lower": int(M == N and epi == 1), "epi": epi, "aux": 1, "sumsq": 1,
                        "b_kmajor": int(epi != 1), "split_k": split, "batch": batch, "k_slabs": slabs, "tile": tile}, None
    # 5. the k_slabs route (an upper triangular square op(A): K = M) and everything it refuses
    for f32, (M, N), slabs in itertools.product((0, 1), SOME + ((1024, 4096), (1536, 1536), (960, 1024)), (2, 4)):
        for K, at, bt, lower, tile, split, nptr, batch, walk in itertools.product(
                (M, 1024), (0, 2), (0, 1), (0, 1), (0, 32, 64, 128), (1, 4), (0, 2, 33), (1, 3), (0, 16)):
            if K % 32 == 0:
                yield f32, {"M": M, "N": N, "K": K, "a_tri": at, "b_tri": bt, "out_lower": lower, "tile": tile,
                            "split_k": split, "nptr": nptr, "batch": batch, "walk": walk, "k_slabs": slabs}, None
    # 6. argument errors: K off the K step (1008: of fp32 only), leading dimensions off 16 bytes
    for f32, (M, N), K, dl, nptr, walk in itertools.product((0, 1), SHAPES, (1000, 1008, 1024), (0, 1, 2), (0, 2), (0, 8)):
        yield f32, {"M": M, "N": N, "K": K, "lda": K + dl, "nptr": nptr, "walk": walk}, None
    yield 0, {"M": 0, "N": 256, "K": 256}, None
    yield 0, {"M": 256, "N": -1, "K": 256, "epi": 2}, None
    # 7. pair launches over the pointer batches: the update A22 -= L21 L21^T of a node of the recursion (lower) with
    #    the first product of its inverse merge, and what keeps two launches from sharing one
    for f32, n1, n2, na, nb, tile in itertools.product((0, 1), (32, 64, 128, 256, 512, 1024, 2048, 1000), (64, 128, 256, 512, 1024, 96),
                                                       (2, 7, 33, 0), (2, 7), (0, 32, 64, 128)):
        a = {"M": n2, "N": n2, "K": n1, "out_lower": 1, "nptr": na, "beta": 1.0, "alpha": -1.0, "tile": tile}
        b = {"M": n2, "N": n1, "K": n1, "b_kmajor": 1, "b_tri": 1, "nptr": nb, "walk": 1, "tile": tile}
        yield f32, a, b
        for k, v in (("a_kmajor", 1), ("epi", 4), ("split_k", 4), ("k_slabs", 2), ("walk", 17), ("lda", n1 + 1), ("out_lower", 0)):
            yield f32, {**a, k: v}, b
            yield f32, a, {**b, k: v}


def route_class(q, r, pair):
    """Which route the point took, for the summary.  `declined`: a launch the documented thresholds send to stream-K
    over all tiles (one problem on whole 128-tiles, both operands triangular, >= 384 tiles, K >= 1024) that stays
    data-parallel because the planner found a tile with an empty k range."""
    if pair is not None:
        return "pair" if r.pair else "pair refused (-3)"
    if r.rc:
        return "refused (-3)"
    if r.tile == 0:
        return "empty"
    if r.xcd:
        return "XCD-aware table"
    if r.sk_first >= 0:
        return "stream-K, all tiles" if r.sk_first == 0 else "stream-K tail"
    if r.slabs:
        return "k_slabs"
    if r.half_occ:
        return "half-occupancy"
    if (r.tile == 128 and q["a_tri"] and q["b_tri"] and q.get("nptr", 0) == 0 and q.get("batch", 1) == 1 and
            q.get("split_k", 1) == 1 and q["M"] % 128 == 0 and q["N"] % 128 == 0 and q["K"] >= 1024 and r.blocks >= 384):
        return "stream-K declined by the planner"
    return f"data-parallel {r.tile}" + (" deep" if r.stages > 2 else "") + (" split-K" if q.get("split_k", 1) > 1 else "")


def plan_hash(lib, f32, a, kind):
    need = lib.gpfit_dev_gemm_plan(f32, ctypes.byref(a), kind, None, 0)
    if need <= 0:
        return f"plan{kind}={need}"
    buf = (ctypes.c_int32 * need)()
    assert lib.gpfit_dev_gemm_plan(f32, ctypes.byref(a), kind, buf, need) == need
    return f"plan{kind}={hashlib.sha256(bytes(buf)).hexdigest()[:16]}"


def main():
    build_library(verbose=False)
    lib = _lib.load()
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    digest, lines, counts = hashlib.sha256(), 0, {}
    r = _lib.DevGemmRoute()
    for f32, q, q2 in grid():
        q = {n: 0 for n in NAMES if n not in ("lda", "split_k", "batch")} | q
        a = args_of(q)
        b = args_of(q2) if q2 is not None else None
        rc = lib.gpfit_dev_gemm_route(f32, ctypes.byref(a), ctypes.byref(b) if b is not None else None, ctypes.byref(r))
        line = f"f32={f32} " + " ".join(f"{n}={getattr(a, n) or 0}" for n in NAMES)
        if b is not None:
            line += " | " + " ".join(f"{n}={getattr(b, n) or 0}" for n in NAMES)
        line += f" -> ret={rc} " + " ".join(f"{n}={getattr(r, n)}" for n in FIELDS)
        if b is None and r.rc == 0:
            if r.xcd:
                line += " " + plan_hash(lib, f32, a, 1)
            elif r.sk_first >= 0:
                line += " " + plan_hash(lib, f32, a, 2)
            elif r.slabs:
                line += " " + plan_hash(lib, f32, a, 3)
        line += "\n"
        digest.update(line.encode())
        lines += 1
        cls = route_class(q, r, q2)
        counts[cls] = counts.get(cls, 0) + 1
        if out:
            out.write(line)
    print(f"grid points {lines}")
    for k in sorted(counts):
        print(f"  {k:36s} {counts[k]}")
    print(f"sha256 {digest.hexdigest()}")


if __name__ == "__main__":
    main()
