"""The three launchers of csrc/skinny.hip -- launch_skinny_slabs, launch_skinny_sum, launch_append_block_finish -- each
on its own through the hook gpfit_dev_skinny, against the plain longdouble reference of skinny_cases.py, element by
element.

Every case is one launch of microseconds on buffers of this test's own.  What the contract says is never read is NaN in
the inputs (skinny_cases.inputs: behind every leading dimension, between the elements of a strided operand, beyond the
diagonal of a triangular op(A), above the diagonal of K22, the partials of dead slabs); every output buffer is prefilled
with a sentinel and must hold it wherever the launcher owns nothing.  Bounds (skinny_cases): partials and sums to the
a-priori (k + 2) 2^-53 S, the zeros, the unit diagonal and the triangles bit for bit, the log-det to 8 x the floor
measured on the CPU.  Each test prints the worst error as a fraction of its bound."""
import ctypes

import numpy as np
import pytest
import torch

import skinny_cases as sc

pytestmark = pytest.mark.gpu


class Device:
    """gpfit_dev_skinny on device buffers of this test's own; numpy in, numpy out."""

    def __init__(self):
        from gaussian_processes_amd import _lib, utils
        self._lib = _lib
        self.lib = _lib.load()
        self.last_error = _lib.last_error
        self.ctx = utils.get_engine(256, 1)._ctx
        self.stream = utils._stream

    def hook(self, op, args):
        return self.lib.gpfit_dev_skinny(self.ctx, self.stream(), self._lib.SKINNY_OP[op], ctypes.byref(args))

    def upload(self, inp):
        return {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda() for k, v in inp["bufs"].items()}

    def args(self, inp, bufs):
        a = self._lib.DevSkinnyArgs()
        for field, v in inp["args"].items():
            setattr(a, field, bufs[v[0]].data_ptr() + 8 * v[1] if isinstance(v, tuple) else v)
        return a

    def run(self, op, inp, ref):
        """One case through the hook on fresh buffers; the output buffers as numpy."""
        bufs = self.upload(inp)
        rc = self.hook(op, self.args(inp, bufs))
        assert rc == 0, self.last_error()
        torch.cuda.synchronize()
        return {b: bufs[b].cpu().numpy() for b in {sc.buffer_of(p) for p in ref}}


@pytest.fixture(scope="module")
def dev():
    return Device()


def run_case(dev, op, case):
    """The case against the reference: value within bound on what the launcher owns, the sentinel elsewhere, no NaN; and
    the same bits from a second run on fresh buffers."""
    inp = sc.inputs(op, case)
    ref = sc.reference(op, inp)
    got = dev.run(op, inp, ref)
    worst, msg = sc.check_all(op, got, ref, inp["bufs"], sc.bar("finish"))
    assert msg is None, f"{case}: {msg}"
    for b, g in got.items():
        assert not np.isnan(g).any(), (op, case, b)
    print(f"{op} {case}: worst error / bound {worst:.3f}")
    again = dev.run(op, inp, ref)
    assert all(sc.same_bits(got[b], again[b]) for b in got), (op, case)


SLABS = sc.CASES["slabs"]


@pytest.mark.parametrize("case", [c for c in SLABS if c[0] == 1], ids=str)
def test_slabs_lower_triangular_row_major(dev, case):
    """launch_skinny_slabs, tri = 1, sar == 1 (L^-1 K12): one to three slabs, panels with one, two and three live slabs,
    a ragged last slab and panel, kc on both sides of every multiple of 16; NaN above the diagonal of the factor."""
    run_case(dev, "slabs", case)


@pytest.mark.parametrize("case", [c for c in SLABS if c[0] == 2], ids=str)
def test_slabs_upper_triangular_from_the_transposed_factor(dev, case):
    """launch_skinny_slabs, tri = 2, sam == 1 (L^-T Y): op(A)(m, r) = L^-1[r][m]; NaN above the diagonal of the factor."""
    run_case(dev, "slabs", case)


@pytest.mark.parametrize("case", [c for c in SLABS if c[0] == 0], ids=str)
def test_slabs_dense_in_every_layout(dev, case):
    """launch_skinny_slabs, tri = 0: the shapes of the call's second and fourth stage (the fourth with the transposed,
    negated output over ten panels), and (130, 300, 33) with either operand in either storage order, with no unit
    stride at all, and with all three base pointers at an odd element offset."""
    run_case(dev, "slabs", case)


@pytest.mark.parametrize("case", sc.CASES["sum"], ids=str)
def test_sum_in_its_three_modes(dev, case):
    """launch_skinny_sum: PLAIN, ROWS (L21 = Y^T and the zero columns of both factors, ldl != ldi), SCHUR (the whole
    128-tile from the lower triangle of K22); the partials of dead slabs are NaN."""
    run_case(dev, "sum", case)


@pytest.mark.parametrize("k", sc.CASES["finish"])
def test_finish_writes_the_two_triangles_and_the_logdet(dev, k):
    """launch_append_block_finish: NaN above the diagonal and beyond k in the leaf's tiles."""
    run_case(dev, "finish", k)


def test_hook_refuses_what_could_become_a_wild_access(dev):
    """-3 before any launch, every output still the sentinel."""
    for op, case, changes in (
            ("slabs", (0, 130, 40, 17, "r", "r", "c", 0, 1.0),
             [("A", None), ("B", None), ("O", None), ("M", 0), ("K", 0), ("kc", 0), ("kc", 129), ("tri", -1), ("tri", 3)]),
            ("sum", (sc.ROWS, 1, 257, 128),
             [("P", None), ("dst", None), ("L", None), ("Li", None), ("M", 0), ("kc", 0), ("kc", 129), ("nslab", 0), ("tri", 3),
              ("mode", 3), ("mode", -1), ("n", 0)]),
            ("sum", (sc.SCHUR, 0, 17, 17), [("Kc", None), ("n", 0)]),
            ("finish", 17, [("Lt", None), ("Lit", None), ("L", None), ("Li", None), ("logdet", None), ("kc", 0), ("kc", 129),
                            ("n", 0)])):
        inp = sc.inputs(op, case)
        bufs = dev.upload(inp)
        for field, value in changes:
            a = dev.args(inp, bufs)
            setattr(a, field, value)
            assert dev.hook(op, a) == -3 and "gpfit_dev_skinny" in dev.last_error(), (op, field, value)
        assert dev.lib.gpfit_dev_skinny(dev.ctx, dev.stream(), 3, ctypes.byref(dev.args(inp, bufs))) == -3
        assert dev.lib.gpfit_dev_skinny(dev.ctx, dev.stream(), -1, ctypes.byref(dev.args(inp, bufs))) == -3
        assert dev.lib.gpfit_dev_skinny(None, dev.stream(), 0, ctypes.byref(dev.args(inp, bufs))) == -3
        assert dev.lib.gpfit_dev_skinny(dev.ctx, dev.stream(), 0, None) == -3
        torch.cuda.synchronize()
        for name in {sc.buffer_of(p) for p in sc.reference(op, inp)}:
            assert sc.same_bits(bufs[name].cpu().numpy(), np.asarray(inp["bufs"][name], dtype=np.float64)), (op, name)
