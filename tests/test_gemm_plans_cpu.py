"""Every plan of the GEMM launcher's balanced schedules is an exact cover.  Host only: no GPU call.

The stream-K schedule (csrc/gemm_streamk.hip) cuts the (tile, k-step) space of a launch -- of all its tiles, or of
the tail behind a data-parallel head -- into one contiguous share per workgroup; the XCD-aware schedule
(csrc/gemm_sched.hip) is a table of tiles.  gpfit_dev_gemm_route says which launches take them and
gpfit_dev_gemm_plan hands out the plan the launcher would upload.  For every such launch of the sweep below:

 * head (the data-parallel kernel's enumeration of block ids 0 .. first-1, restated HERE from the documented walk
   semantics of gpfit_dgemm_ex, not taken from the library) + the plan's tile list = every output tile once, and
   the tile list is the rest of that same walk; the non-negative entries of an XCD table = every tile once;
 * the k range of every tile is the triangular rule of csrc/common.h, the prefix sums are consistent, and
   replaying the kernel's cut (per_block consecutive k-steps per workgroup) hands out every k-step exactly once;
 * a segment that is not a whole tile has its workspace slot 2 b + (nseg > 0) exactly once in the fix-up lists, under
   its own tile, in block order; no whole tile is in the fix-up lists; every slot fits the workspace.
"""
import ctypes
import itertools

import numpy as np
import pytest

from gaussian_processes_amd import _lib
from gaussian_processes_amd.build import build_library

T = 128
SQUARE = range(1, 81)                                             # tiles per side
RECT = ((24, 16), (16, 24), (23, 23), (17, 31), (40, 13), (8, 64), (64, 8), (72, 9), (3, 200), (50, 64))   # tm, tn
KS = (1024, 2048, 8192)
WALKS = (0, 1, 2, 3, 8)                                           # 8: the XCD-aware table (it fixes the walk itself)


@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _lib.load()


def walk_order(walk, lower, tm, tn):
    """The documented walk: row-major over the tiles (of the lower triangle: rows i, columns 0 .. i); bit 1:
    column-major (lower: columns j, rows j .. nt-1); bit 0: backwards."""
    if lower:
        order = ([(i, j) for j in range(tn) for i in range(j, tm)] if walk & 2 else
                 [(i, j) for i in range(tm) for j in range(i + 1)])
    else:
        order = ([(i, j) for j in range(tn) for i in range(tm)] if walk & 2 else
                 [(i, j) for i in range(tm) for j in range(tn)])
    return order[::-1] if walk & 1 else order


def k_range(K, at, bt, ti, tj):
    kb, ke = 0, K
    if at == 1: ke = min(ke, ti * T + T)
    if at == 2: kb = max(kb, ti * T)
    if bt == 1: kb = max(kb, tj * T)
    if bt == 2: ke = min(ke, tj * T + T)
    return kb, ke


def query(lib, f32, **kw):
    a = _lib.DevGemmArgs(**{"lda": kw["K"], "ldb": kw["K"], "ldc": kw["N"], "alpha": 1.0, "batch": 1, "split_k": 1, **kw})
    r = _lib.DevGemmRoute()
    assert lib.gpfit_dev_gemm_route(f32, ctypes.byref(a), None, ctypes.byref(r)) == 0
    return a, r


def get_plan(lib, f32, a, kind):
    need = lib.gpfit_dev_gemm_plan(f32, ctypes.byref(a), kind, None, 0)
    assert need > 0, need
    buf = (ctypes.c_int32 * need)()
    assert lib.gpfit_dev_gemm_plan(f32, ctypes.byref(a), kind, buf, need) == need
    return np.frombuffer(buf, dtype=np.int32).copy()


def check_streamk(p, f32, tm, tn, K, lower, at, bt, walk, first):
    tag = (tm, tn, K, lower, at, bt, walk, f32)
    kt = 32 if f32 else 16
    pfirst, nt, total, blocks, per_block, nfix, nslot, ws_slots = (int(v) for v in p[:8])
    assert pfirst == first, tag
    rec = p[8:8 + 5 * nt].reshape(nt, 5)
    fix_tile = p[8 + 5 * nt:][:nfix]
    fix_ptr = p[8 + 5 * nt + nfix:][:nfix + 1]
    fix_slot = p[8 + 5 * nt + 2 * nfix + 1:][:nslot]
    assert 8 + 5 * nt + 2 * nfix + 1 + nslot == len(p), tag
    # --- tiles: head + tail = the walk
    order = walk_order(walk, lower, tm, tn)
    tail = [(int(r0) // T, int(c0) // T) for r0, c0 in rec[:, :2]]
    assert np.all(rec[:, :2] % T == 0), tag
    head = order[:first]
    count = {}
    for t in head + tail:
        count[t] = count.get(t, 0) + 1
    missing = sorted(set(order) - set(count))
    twice = sorted(t for t, c in count.items() if c != 1)
    assert not missing and not twice and len(head) + len(tail) == len(order), \
        f"{tag}: first {first}: tiles never written {missing}; written twice {twice}"
    assert tail == order[first:], f"{tag}: the tail is not the rest of the head's walk"
    # --- k ranges and prefix sums
    pre = 0
    for (ti, tj), (_, _, kbeg, ksteps, prefix) in zip(tail, rec.tolist()):
        kb, ke = k_range(K, at, bt, ti, tj)
        assert ke > kb and kbeg == kb and ksteps * kt == ke - kb and prefix == pre, (tag, ti, tj)
        pre += ksteps
    assert total == pre and 0 < blocks <= 512 and per_block == -(-total // blocks), tag
    # --- replay the kernel's cut
    ends = rec[:, 4] + rec[:, 3]
    done = np.zeros(nt, dtype=np.int64)          # k-steps handed out per tile
    want = [[] for _ in range(nt)]               # slots per split tile, block order
    for b in range(blocks):
        it, it_end = b * per_block, min(total, (b + 1) * per_block)
        if it >= it_end:
            continue
        t = int(np.searchsorted(ends, it, side="right"))
        nseg = 0
        while it < it_end:
            tbeg, tend = int(rec[t, 4]), int(ends[t])
            assert tbeg <= it < tend, tag
            s1 = min(it_end, tend)
            assert done[t] == it - tbeg, f"{tag}: tile {t} k-steps out of order"
            done[t] += s1 - it
            if not (it == tbeg and s1 == tend):
                want[t].append(2 * b + (1 if nseg else 0))
            assert nseg == 0 or it == tbeg, tag     # only the first segment of a workgroup starts inside a tile
            nseg += 1
            it = s1
            t += 1
    assert np.array_equal(done, rec[:, 3]), f"{tag}: k-steps not handed out exactly once"
    # --- fix-up lists
    split = [t for t in range(nt) if want[t]]
    assert fix_tile.tolist() == split, tag
    assert fix_ptr[0] == 0 and fix_ptr[-1] == nslot, tag
    for n, t in enumerate(split):
        assert fix_slot[fix_ptr[n]:fix_ptr[n + 1]].tolist() == want[t], (tag, t)
    assert len(set(fix_slot.tolist())) == nslot, tag
    assert ws_slots == 1024 and (nslot == 0 or (0 <= fix_slot.min() and fix_slot.max() < ws_slots)), tag


def check_xcd(p, tm, tn, lower, tag):
    n = int(p[0])
    table = p[1:]
    assert len(table) == n and n % 8 == 0, tag
    ent = table[table >= 0]
    assert np.all(table[table < 0] == -1), tag
    got = sorted((int(e) >> 16, int(e) & 0xffff) for e in ent)
    want = sorted((i, j) for i in range(tm) for j in range((i + 1) if lower else tn))
    assert got == want, f"{tag}: the table does not hold every tile exactly once"


def cases():
    """The shapes x K in KS with the triangular flags where the shape allows them (a triangular op(A) is M x M, a
    triangular op(B) N x N), and every square shape once more at K = its own side for the triangular combinations: the
    products of triangular factors the fit sends down the stream-K route (3584 = 28, 3712 = 29 tiles per side, ...)."""
    shapes = [(n, n) for n in SQUARE] + list(RECT)
    for (tm, tn), lower, f32 in itertools.product(shapes, (0, 1), (0, 1)):
        if lower and tm != tn:
            continue
        for K in KS + ((tm * T,) if tm == tn and tm * T not in KS else ()):
            for at, bt in itertools.product((0, 1, 2), repeat=2):
                if (at and tm * T != K) or (bt and tn * T != K) or (K not in KS and not (at or bt)):
                    continue
                yield tm, tn, K, lower, at, bt, f32


def test_every_streamk_and_xcd_plan_is_an_exact_cover(lib):
    seen = {"streamk_all": set(), "streamk_tail": set(), "xcd": set(), "plain": set()}     # distinct (tm, tn, K) per route
    firsts = {}
    for tm, tn, K, lower, at, bt, f32 in cases():
        for walk in WALKS:
            a, r = query(lib, f32, M=tm * T, N=tn * T, K=K, out_lower=lower, a_tri=at, b_tri=bt, walk=walk)
            assert r.rc == 0
            tag = (tm, tn, K, lower, at, bt, walk, f32)
            if r.xcd:
                assert walk & 8 and r.sk_first == -1 and r.tile == T, tag
                check_xcd(get_plan(lib, f32, a, 1), tm, tn, lower, tag)
                assert lib.gpfit_dev_gemm_plan(f32, ctypes.byref(a), 2, None, 0) == -1
                seen["xcd"].add((tm, tn, K))
            elif r.sk_first >= 0:
                assert r.tile == T, tag
                check_streamk(get_plan(lib, f32, a, 2), f32, tm, tn, K, lower, at, bt, walk & 3, r.sk_first)
                seen["streamk_all" if r.sk_first == 0 else "streamk_tail"].add((tm, tn, K))
                if not (at or bt or f32) and K == 1024 and lower:
                    firsts[(tm, walk)] = r.sk_first
            else:
                assert lib.gpfit_dev_gemm_plan(f32, ctypes.byref(a), 2, None, 0) == -1, tag
                seen["plain"].add((tm, tn, K))
    # the sweep is not vacuous: every kind of plan was met at many distinct shapes -- stream-K over all tiles among them
    # at the sizes the fit sends there -- and the lower SYRK at the fit's sizes keeps the head it was tuned with
    assert min(len(v) for v in seen.values()) >= 40, {k: len(v) for k, v in seen.items()}
    assert {(28, 28, 3584), (29, 29, 3712), (64, 64, 8192)} <= seen["streamk_all"]
    for walk in (0, 1, 2, 3):
        assert [firsts.get((n, walk)) for n in (32, 36, 48, 56, 64)] == [512, 512, 1024, 1536, 2048], (walk, firsts)


def test_route_query_names_the_launcher_choices(lib):
    """Spot checks of gpfit_dev_gemm_route against the thresholds the sources document (defaults, no tuning knob set)."""
    q = lambda f32=0, **kw: query(lib, f32, **{"M": 256, "N": 256, "K": 256, **kw})[1]
    r = q(M=3584, N=3584, K=3584, out_lower=1, a_tri=1, b_tri=1)
    assert (r.tile, r.sk_first, r.xcd, r.stages) == (128, 0, 0, 2)
    r = q(M=2944, N=2944, K=1024)                         # 529 tiles: 512 + a tail of 17
    assert (r.tile, r.sk_first) == (128, 512)
    assert q(M=2944, N=2944, K=1008).sk_first == -1       # K below 1024
    assert q(M=2944, N=2944, K=1024, tile=64).sk_first == -1
    r = q(M=5120, N=5120, K=1024, walk=8)                 # 1600 tiles >= 1536
    assert (r.xcd, r.sk_first, r.tile) == (1, -1, 128) and r.blocks % 8 == 0 and r.blocks >= 1600
    assert q(M=5120, N=5120, K=1024, walk=0).xcd == 0
    assert q(M=4992, N=4992, K=1024, walk=8).xcd == 0     # 1521 tiles
    r = q(M=1024, N=1024, K=1024)                         # 64 128-tiles -> 256 64-tiles, deep pipeline of 4 stages
    assert (r.tile, r.stages, r.edge, r.blocks) == (64, 4, 0, 256)
    r = q(M=512, N=512, K=512)
    assert (r.tile, r.stages, r.blocks) == (32, 8, 256)
    r = q(M=1000, N=616, K=528)
    assert r.edge == 1 and r.stages == 2
    assert q(M=2048, N=2560, K=512).tile == 64            # 320 tiles < 384
    r = q(M=2560, N=2560, K=512, walk=16)                 # 400
    assert (r.tile, r.half_occ, r.sk_first) == (128, 1, -1)
    r = q(M=512, N=512, K=8192, split_k=8)
    assert r.sk_first == -1 and r.blocks % 8 == 0
    # fused epilogues: tile norms on the three schedules; a launch that cannot carry one is an error
    r = q(M=3712, N=3712, K=3712, out_lower=1, a_tri=1, b_tri=1, b_kmajor=1, epi=2, sumsq=1)
    assert (r.rc, r.sk_first, r.epi, r.sumsq_entries) == (0, 0, 2, 33 * 435)
    r = q(M=1024, N=1024, K=1024, out_lower=1, b_kmajor=1, epi=2, sumsq=1, tile=128)
    assert (r.rc, r.epi, r.sumsq_entries) == (0, 2, 36)
    assert q(M=1024, N=1024, K=1024, out_lower=1, b_kmajor=1, epi=2, sumsq=1).rc == -3      # 64-tiles
    assert q(M=2944, N=2944, K=1024, epi=1, tile=128).rc == -3                               # mirror needs a lower output
    # fp32 takes the same routes
    assert q(1, M=2944, N=2944, K=1024).sk_first == 512


def test_streamk_tail_follows_the_column_major_walk_of_a_lower_output(lib):
    """The defect this module was written for: N = 4096 lower, K = 1024, walk 2 (column-major).  Head = the first 512
    tiles of the walk by columns; a tail enumerated by rows left ten tiles unwritten and wrote ten twice."""
    a, r = query(lib, 0, M=4096, N=4096, K=1024, out_lower=1, walk=2)
    assert r.sk_first == 512
    p = get_plan(lib, 0, a, 2)
    tail = sorted((int(x) // T, int(y) // T) for x, y in p[8:8 + 5 * 16].reshape(16, 5)[:, :2])
    assert tail == sorted(walk_order(2, 1, 32, 32)[512:])
    assert tail == sorted([(31, 26)] + [(i, j) for j in range(27, 32) for i in range(j, 32)])
