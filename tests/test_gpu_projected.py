"""The launchers of csrc/projected.hip that run behind no chain gate, each on its own through the hook
gpfit_dev_projected, against the plain longdouble reference of projected_cases.py, element by element:
launch_proj_moments_group (with its sum3), launch_proj_ga_group, launch_proj_gkb_group, launch_proj_gktb_group,
launch_proj_trace_group, launch_estep_proj_rows, launch_estep_proj_scale, launch_estep_proj_moments.  (The chain-gated
variants share these bodies and stay with the chain tests.)

Every case is a launch or two of microseconds on buffers of this test's own, at the true ragged sizes: nb = 1, 63, 65,
n % 4 != 0, n no multiple of 32 or 128.  What the contract says is never read is NaN in the inputs (behind every leading
dimension, rows >= n of the closure operands, everything but the diagonal under the trace); every output buffer is
prefilled with a sentinel and must hold it wherever the launcher owns nothing.  Bounds (projected_cases): sums to the
a-priori (k + 2) 2^-53 S, zero rows and copies bit for bit, what goes through exp or sqrt to 8 x the floor measured on
the CPU.  Each test prints the worst error as a fraction of its bound."""
import ctypes

import numpy as np
import pytest
import torch

import projected_cases as pc
import skinny_cases as sc

pytestmark = pytest.mark.gpu


class Device:
    """gpfit_dev_projected on device buffers of this test's own; numpy in, numpy out."""

    def __init__(self):
        from gaussian_processes_amd import _lib, utils
        self._lib = _lib
        self.lib = _lib.load()
        self.last_error = _lib.last_error
        self.ctx = utils.get_engine(256, 1)._ctx
        self.stream = utils._stream

    def hook(self, op, args):
        return self.lib.gpfit_dev_projected(self.ctx, self.stream(), self._lib.PROJ_OP[op], ctypes.byref(args))

    def upload(self, inp):
        return {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda() for k, v in inp["bufs"].items()}

    def args(self, op, units, bufs):
        """The hook's struct for the units of one launch (one unit for the single launchers); the ctypes arrays it points
        to are kept alive on the struct."""
        a = self._lib.DevProjArgs()
        i = units[0]
        for field in ("n", "np", "nb", "nrows", "npc", "ld", "lda", "A"):
            if field in i:
                setattr(a, field, i[field])
        a._keep = []
        if op in pc.GROUP_OPS:
            nu = a.n_units = len(units)
            for k, name in enumerate(i["slots"]):
                arr = (ctypes.c_void_p * nu)(*[b[name].data_ptr() for b in bufs])
                a._keep.append(arr)
                a.up[k] = ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p))
            for field, key, ctype in (("uA", "A", ctypes.c_double), ("ulambda0", "lambda0", ctypes.c_double), ("un", "n", ctypes.c_int32)):
                arr = (ctype * nu)(*[u.get(key, 0) for u in units])
                a._keep.append(arr)
                setattr(a, field, ctypes.cast(arr, ctypes.POINTER(ctype)))
        else:
            for k, name in enumerate(i["slots"]):
                a.p[k] = bufs[0][name].data_ptr() if name in bufs[0] else None
        return a

    def run(self, op, units, refs):
        """One launch for the units on fresh buffers; per unit the output buffers as numpy."""
        bufs = [self.upload(i) for i in units]
        rc = self.hook(op, self.args(op, units, bufs))
        assert rc == 0, self.last_error()
        torch.cuda.synchronize()
        return [{b: bb[b].cpu().numpy() for b in {sc.buffer_of(p) for p in ref}} for bb, ref in zip(bufs, refs)]


@pytest.fixture(scope="module")
def dev():
    return Device()


def verify(op, case, got, ref, inp):
    worst, msg = sc.check_all(op, got, ref, inp["bufs"], pc.bar(op))
    assert msg is None, f"{case}: {msg}"
    for b, g in got.items():
        assert not np.isnan(g).any(), (op, case, b)
    return worst


def run_case(dev, op, case):
    """The case (a group of one where the launcher is unit-batched) against the reference: value within bound on what the
    launcher owns, the sentinel elsewhere, no NaN; and the same bits from a second run on fresh buffers."""
    inp = pc.inputs(op, case)
    ref = pc.reference(op, inp)
    got, = dev.run(op, [inp], [ref])
    print(f"{op} {case}: worst error / bound {verify(op, case, got, ref, inp):.3f}")
    again, = dev.run(op, [inp], [ref])
    assert all(sc.same_bits(got[b], again[b]) for b in got), (op, case)


@pytest.mark.parametrize("case", pc.SHAPES, ids=str)
@pytest.mark.parametrize("op", ["moments", "ga", "gkb", "gktb"])
def test_closure_passes_as_a_group_of_one(dev, op, case):
    """launch_proj_moments_group (part as 3 x ceil(n / 4), out3 over all n), launch_proj_ga_group, launch_proj_gkb_group
    (in place) and launch_proj_gktb_group."""
    run_case(dev, op, case)


@pytest.mark.parametrize("n", pc.CASES["trace"])
def test_trace_reads_the_diagonal_alone(dev, n):
    """launch_proj_trace_group: everything off the diagonal is NaN."""
    run_case(dev, "trace", n)


@pytest.mark.parametrize("case", pc.SHAPES, ids=str)
@pytest.mark.parametrize("op", ["estep_rows", "estep_moments"])
def test_estep_row_passes(dev, op, case):
    """launch_estep_proj_rows (zero on the rows n .. nrows) and launch_estep_proj_moments at the true ragged nb."""
    run_case(dev, op, case)


@pytest.mark.parametrize("case", pc.CASES["estep_scale"], ids=str)
def test_estep_scale_with_and_without_the_padded_copy(dev, case):
    """launch_estep_proj_scale: Y and aLp zero padded to [nrows][npc], part as [nrows / 32][npc]."""
    run_case(dev, "estep_scale", case)


@pytest.mark.parametrize("op", pc.GROUP_OPS)
def test_three_units_give_the_bits_of_their_groups_of_one(dev, op):
    """Three units with different data, different A and lambda0 (for the trace different n) in one launch: every unit's
    outputs bit-equal to its own group of one, and within the bounds."""
    units = [pc.inputs(op, case, unit=u) for u, case in enumerate(pc.GROUP_CASES[op])]
    refs = [pc.reference(op, i) for i in units]
    together = dev.run(op, units, refs)
    for u, (i, ref, got) in enumerate(zip(units, refs, together)):
        alone, = dev.run(op, [i], [ref])
        for b in got:
            assert sc.same_bits(got[b], alone[b]), (op, u, b)
        print(f"{op} group unit {u}: worst error / bound {verify(op, pc.GROUP_CASES[op][u], got, ref, i):.3f}")


def test_hook_refuses_what_could_become_a_wild_access(dev):
    """-3 before any launch, every output still the sentinel (an in-place operand its input)."""
    table = (
        ("moments", (130, 65), [("n_units", 0), ("n_units", 17), ("n", 0), ("nb", 0), ("ld", 64), ("uA", None), ("ulambda0", None),
                                ("up", 12), ("up", 0), ("ptr", 6)]),
        ("ga", (130, 65), [("n_units", 17), ("n", 0), ("np", 129), ("nb", 0), ("ld", 64), ("up", 5), ("ptr", 5)]),
        ("gkb", (130, 65), [("n_units", 0), ("np", 0), ("ld", 0), ("up", 2), ("ptr", 2)]),
        ("gktb", (130, 65), [("n_units", 17), ("nb", 0), ("ld", 64), ("up", 4), ("ptr", 4)]),
        ("trace", 130, [("n_units", 0), ("n_units", 17), ("un", None), ("unv", 0), ("ld", 0), ("up", 1), ("ptr", 1)]),
        ("estep_rows", (130, 65), [("n", 0), ("nb", 0), ("nrows", 128), ("nrows", 161), ("nrows", 0), ("lda", 64), ("p", 4), ("p", 0)]),
        ("estep_scale", (130, 65, 1), [("n", 0), ("nb", 0), ("nrows", 150), ("nrows", 96), ("npc", 0), ("ld", 127), ("lda", 64),
                                       ("p", 3), ("p", 5), ("p", 0)]),
        ("estep_moments", (130, 65), [("n", 0), ("nb", 0), ("ld", 64), ("p", 3), ("p", 4), ("p", 0)]),
    )
    for op, case, changes in table:
        inp = pc.inputs(op, case)
        bufs = dev.upload(inp)
        for field, value in changes:
            a = dev.args(op, [inp], [bufs])
            if field == "up":            # a missing table
                a.up[value] = None
            elif field == "ptr":         # a NULL in a table
                arr = (ctypes.c_void_p * 1)(None)
                a._keep.append(arr)
                a.up[value] = ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p))
            elif field == "p":
                a.p[value] = None
            elif field == "unv":         # an extent below 1 in the per-unit table
                arr = (ctypes.c_int32 * 1)(value)
                a._keep.append(arr)
                a.un = ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32))
            else:
                setattr(a, field, value)
            assert dev.hook(op, a) == -3 and "gpfit_dev_projected" in dev.last_error(), (op, field, value)
        good = dev.args(op, [inp], [bufs])
        assert dev.lib.gpfit_dev_projected(dev.ctx, dev.stream(), 8, ctypes.byref(good)) == -3
        assert dev.lib.gpfit_dev_projected(dev.ctx, dev.stream(), -1, ctypes.byref(good)) == -3
        assert dev.lib.gpfit_dev_projected(None, dev.stream(), dev._lib.PROJ_OP[op], ctypes.byref(good)) == -3
        assert dev.lib.gpfit_dev_projected(dev.ctx, dev.stream(), dev._lib.PROJ_OP[op], None) == -3
        torch.cuda.synchronize()
        for name in {sc.buffer_of(p) for p in pc.reference(op, inp)}:
            assert sc.same_bits(bufs[name].cpu().numpy(), np.asarray(inp["bufs"][name], dtype=np.float64)), (op, name)
    # aLp alone may be absent
    inp = pc.inputs("estep_scale", (130, 65, 0))
    assert dev.args("estep_scale", [inp], [dev.upload(inp)]).p[4] is None
