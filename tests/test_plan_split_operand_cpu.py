"""The schedule table of a launch whose op(B) is dense left of a column and lower triangular from it on
(GemmArgsT::b_split: [T21 | T22] = C [S | LV22] as one launch, fit.hip:t_in_blocks).  Host only: no GPU call.

The planner is asked through gpfit_dev_gemm_plan (kind 4: the XCD-aware table with each tile's k range) for the
launch of n2 x (n1 + n2) x n2 with a lower triangular op(A), for (n1, n2) = (256, 256), (384, 256) and (4096, 4096).
The small shapes take the table only with GPFIT_XCD_MIN_TILES lowered, and the knob is read once per process: the
queries run in a child process.  Asserted: every tile with a non-empty k range is in the table exactly once, no empty
tile is, the k ranges equal the restatement below, and 4096 + 4096 gives the 1552 tiles that put the launch above the
launcher's own threshold of 1536 (asked again in this process, with no knob set)."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from gaussian_processes_amd import _lib
from gaussian_processes_amd.build import build_library

T = 128
SHAPES = ((256, 256), (384, 256), (4096, 4096))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
from gaussian_processes_amd import _lib
lib = _lib.load()
out = {}
for n1, n2 in json.loads(sys.argv[2]):
    a = _lib.DevGemmArgs(M=n2, N=n1 + n2, K=n2, lda=n2, ldb=n1 + n2, ldc=n1 + n2, alpha=1.0, batch=1, split_k=1, a_tri=1, b_tri=1,
                         b_kmajor=1, b_split=n1, walk=8, tile=128)
    need = lib.gpfit_dev_gemm_plan(0, ctypes.byref(a), 4, None, 0)
    assert need > 0, need
    buf = (ctypes.c_int32 * need)()
    assert lib.gpfit_dev_gemm_plan(0, ctypes.byref(a), 4, buf, need) == need
    out[f"{n1},{n2}"] = list(buf)
print("PLANS " + json.dumps(out))
"""


def k_range(n1, n2, ti, tj):
    """Lower triangular op(A): k below the tile's last row.  op(B): every k left of column n1; from it on, k from the
    tile's first column counted from n1."""
    kb, ke = 0, min(n2, ti * T + T)
    if tj * T >= n1:
        kb = tj * T - n1
    return kb, ke


@pytest.fixture(scope="module")
def plans():
    build_library(verbose=False)
    env = dict(os.environ, GPFIT_XCD_MIN_TILES="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(SHAPES)], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("PLANS ")][0][6:])


@pytest.mark.parametrize("n1,n2", SHAPES)
def test_table_is_the_tiles_with_a_k_range(plans, n1, n2):
    p = plans[f"{n1},{n2}"]
    length = p[0]
    assert len(p) == 1 + 3 * length and length % 8 == 0
    rows = [p[1 + 3 * e:4 + 3 * e] for e in range(length)]
    want = {}
    for ti in range(n2 // T):
        for tj in range((n1 + n2) // T):
            kb, ke = k_range(n1, n2, ti, tj)
            if ke > kb:
                want[(ti, tj)] = (kb, ke)
    seen = {}
    for t, kb, ke in rows:
        if t < 0:
            assert (kb, ke) == (0, 0)
            continue
        key = (t >> 16, t & 0xffff)
        assert key not in seen, f"tile {key} twice"
        seen[key] = (kb, ke)
    assert not set(want) - set(seen), f"tiles never written: {sorted(set(want) - set(seen))[:8]}"
    assert not set(seen) - set(want), f"tiles without a k range in the table: {sorted(set(seen) - set(want))[:8]}"
    assert seen == want
    # the 21 block in full and the 22 block's lower tiles
    t1, t2 = n1 // T, n2 // T
    assert len(seen) == t2 * t1 + t2 * (t2 + 1) // 2
    if (n1, n2) == (4096, 4096):
        assert len(seen) == 1552


def test_the_headline_launch_takes_the_table_on_its_own():
    """No knob: 1552 tiles are above the launcher's 1536, the route is the table and its grid holds them; one tile column
    less of the dense part (1520 tiles) is refused -- a split operand has no other schedule."""
    build_library(verbose=False)
    lib = _lib.load()

    def route(n1, n2):
        a = _lib.DevGemmArgs(M=n2, N=n1 + n2, K=n2, lda=n2, ldb=n1 + n2, ldc=n1 + n2, alpha=1.0, batch=1, split_k=1, a_tri=1,
                             b_tri=1, b_kmajor=1, b_split=n1, walk=9)
        r = _lib.DevGemmRoute()
        assert lib.gpfit_dev_gemm_route(0, ctypes.byref(a), None, ctypes.byref(r)) == 0
        return r
    r = route(4096, 4096)
    assert r.rc == 0 and r.xcd == 1 and r.tile == 128 and 1552 <= r.blocks < 1552 + 64
    assert route(3968, 4096).rc == -3
