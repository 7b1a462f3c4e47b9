"""The element-wise and reduction launchers of csrc/elementwise.hip, each on its own through the hook
gpfit_dev_elementwise, against the plain longdouble reference of elementwise_cases.py, element by element.

Every case is a few launches of microseconds on buffers of this test's own.  What a launcher's contract says is never
read is NaN in the inputs (elementwise_cases.inputs); every output buffer is prefilled with a sentinel (an in-place
operand with its input), scratch with NaN, and what the launcher does not own must hold afterwards what it held
before.  Bounds (elementwise_cases: ``Out``, ``check``): sums are held to the a-priori (k + 2) 2^-53 S, formula outputs to
8 x (16 x for device-only summation orders) the floor the fp64 restatement makes against the reference on the same
inputs (``FLOOR``, asserted on the CPU), exact outputs, bit identity, zeros and symmetry as such.  Each test prints the
worst error as a fraction of its bound."""
import ctypes

import numpy as np
import pytest
import torch

import elementwise_cases as ec

pytestmark = pytest.mark.gpu

# p: the pointer slots in the hook's order -- an input or output by name ("?name": may be absent), or (scratch name,
# number of doubles); ld: a key of the inputs, or "@out" for the leading dimension of that output's buffer; n, s: keys
SPEC = {
    "trmv_lower": dict(p=["L", "x", "y"], ld=["ld"], n=["np"]),
    "trmv_lower_t": dict(p=["L", "x", "z", ("partial", lambda i: (i["np"] // ec.TRMV_ROWS + 1) * i["np"])], ld=["ld"], n=["np"]),
    "symv_lower": dict(p=["A", "x", "y"], ld=["ld"], n=["n"]),
    "gemv_sub": dict(p=["M", "x", "y", "out"], ld=["ld"], n=["rows", "cols"]),
    "gemv_t_sub": dict(p=["M", "x", "y", "out", ("partial", lambda i: (i["rows"] // ec.TRMV_ROWS + 1) * i["cols"])], ld=["ld"],
                       n=["rows", "cols"]),
    "dot": dict(p=["x", "y", "out"], n=["n"]),
    "logdet": dict(p=["L0", "out0"], ld=["ld"], n=["n"]),
    "logdet_pair": dict(p=["L0", "out0", "L1", "out1"], ld=["ld"], n=["n"]),
    "frob_lower": dict(p=["T", "out", ("partial", lambda i: (i["np"] // 128) ** 2)], ld=["ld"], n=["np"]),
    "frob_tiles": dict(p=["T", "partial"], ld=["ld"], n=["rows", "cols", "lower"]),
    "reduce_slices": dict(p=["?src", "dst"], ld=["stride", "count"], n=["nslice", "to32"]),
    "reduce_slabs": dict(p=["src", "dst"], ld=["stride"], n=["nslab", "slab_rows", "rows", "cols"]),
    "reduce_slices_sym": dict(p=["src", "dst"], ld=["stride"], n=["nslice", "n"]),
    "pack_lower": dict(p=["A", "dst"], ld=["ld", "@dst"], n=["n", "np"]),
    "pack_tri": dict(p=["A", "dst"], ld=["ld", "@dst"], n=["n", "np"]),
    "unpack_sym": dict(p=["A", "dst"], ld=["ld", "@dst"], n=["n"]),
    "unpack_tri": dict(p=["A", "dst"], ld=["ld", "@dst"], n=["n"]),
    "symmetrize": dict(p=["A"], ld=["ld"], n=["n"]),
    "symmetrize_avg": dict(p=["A"], ld=["ld"], n=["n"]),
    "pad_copy": dict(p=["src", "dst"], ld=["ld", "@dst"], n=["rows", "cols", "prow", "pcol"]),
    "gather": dict(p=["X", "Xt", "pix", "?Xm"], ld=["ldx", "@Xt", "@Xm"], n=["n", "d", "dp", "np"]),
    "estep_build": dict(p=["K", "sv", "Mb", "SK", "Kl"], ld=["ldk", "@Mb"], n=["n", "np"]),
    "add_diag": dict(p=["A"], ld=["ld"], n=["n"], s=["v"]),
    "axpby_block": dict(p=["dst", "src"], ld=["@dst", "@src"], n=["rows", "cols"], s=["a", "b"]),
    "demote_block": dict(p=["src", "dst"], ld=["@src", "@dst"], n=["rows", "cols"]),
    "qvec": dict(p=["Xt", "XCt", "Kvec", "q"], ld=["ld"], n=["n", "np", "dp"], s=["s0sq"]),
    "moments": dict(p=["Kvec", "q", "Cos", "V", "m", "r", "lam_m", "lam_var", "f", "wl", "scal",
                       ("part", lambda i: 3 * (i["n"] // 256 + 1)), "ticket"], ld=["ldc", "ldv"], n=["n"], s=["A", "lambda0"]),
    "adjoint_rect": dict(p=["W", "Cos", "q1", "q2", "Aout", ("upart", lambda i: i["np1"] * i["np2"] // 64),
                            ("vpart", lambda i: i["np1"] * i["np2"] // 64), ("tile_sum", lambda i: i["np1"] * i["np2"] // 4096),
                            "t1", "t2", "uq1", "uq2", "scal3", "?extra1"], ld=["ldw", "ldc", "@Aout"], n=["n1", "n2", "np1", "np2"]),
    "metric_contract": dict(p=["pix", "C", "M", "grad5", ("part", lambda i: 5 * ec.METRIC_BLOCKS), "ticket"], ld=["ldc", "ldm"],
                            n=["d", "n_rows", "n_cols"]),
    "dk_sigma0": dict(p=["Cos", "q1", "q2", "dK"], ld=["ldc", "@dK"], n=["n1", "n2"], s=["s0"]),
    "dq": dict(p=["Xt", "XDt", "q", "?dq", "?h"], ld=["ld"], n=["n", "dp"]),
    "dk_metric": dict(p=["H", "Cos", "q1", "q2", "dq1", "dq2"], ld=["ldh", "ldc"], n=["n1", "n2"]),
    "estep_prep": dict(p=["f", "r", "m", "sv", "rhs"], n=["n", "np"], s=["A"]),
    "rowscale_add": dict(p=["Y", "Xm", "t"], ld=["@Y", "@Xm"], n=["np", "dp"], s=["scale"]),
}
# outputs that are double whatever the element type
DOUBLE_OUT = {("dot", "out"), ("logdet", "out0"), ("logdet_pair", "out0"), ("logdet_pair", "out1"), ("frob_lower", "out"),
              ("frob_tiles", "partial"), ("moments", "scal"), ("adjoint", "uq"), ("adjoint", "scal"), ("metric_contract", "grad5")}


class Device:
    """gpfit_dev_elementwise on device buffers of this test's own; numpy in, numpy out."""

    def __init__(self):
        from gaussian_processes_amd import _lib, utils
        self._lib = _lib
        self.lib = _lib.load()
        self.last_error = _lib.last_error
        self.ctx = utils.get_engine(256, 1)._ctx
        self.stream = utils._stream

    def hook(self, op, f32, args, group=False):
        return self.lib.gpfit_dev_elementwise(self.ctx, self.stream(), self._lib.EW_OP[op] + (self._lib.EW_GROUP if group else 0),
                                              int(f32), ctypes.byref(args))

    def buffers(self, op, inp, ref, f32):
        """name -> device tensor for every slot of the op: inputs uploaded, outputs prefilled (their input when in
        place, the sentinel otherwise), scratch NaN, the ticket word zero.  Also name -> the initial numpy buffer."""
        R = np.float32 if f32 else np.float64
        bufs, init = {}, {}
        for slot in SPEC[op]["p"]:
            if isinstance(slot, tuple):
                bufs[slot[0]] = torch.full((int(slot[1](inp)),), float("nan"), dtype=torch.float64, device="cuda")
                continue
            name = slot.lstrip("?")
            if name == "ticket":
                bufs[name] = torch.zeros(1, dtype=torch.int32, device="cuda")
            elif name in ref:
                dt = np.float64 if (op, name) in DOUBLE_OUT else R
                if op == "reduce_slices" and inp["to32"] or op == "demote_block":
                    dt = np.float32
                a = np.array(inp[name], dtype=dt) if inp.get(name) is not None else np.full(ref[name].val.shape, ec.SENTINEL, dt)
                init[name] = a
                bufs[name] = torch.from_numpy(a).cuda()
            elif name == "src" and op == "reduce_slices" and inp["to32"]:
                bufs[name] = torch.from_numpy(inp["src64"]).cuda()
            elif inp.get(name) is not None:
                bufs[name] = torch.from_numpy(np.ascontiguousarray(inp[name])).cuda()
        return bufs, init

    def args(self, op, inp, bufs):
        a = self._lib.DevEwArgs()
        sp = SPEC[op]
        for k, slot in enumerate(sp["p"]):
            name = slot[0] if isinstance(slot, tuple) else slot.lstrip("?")
            a.p[k] = bufs[name].data_ptr() if name in bufs else None
        for k, key in enumerate(sp.get("ld", ())):
            if key.startswith("@"):
                a.ld[k] = bufs[key[1:]].shape[-1] if key[1:] in bufs else 0
            else:
                a.ld[k] = int(inp[key])
        for k, key in enumerate(sp.get("n", ())):
            a.n[k] = int(inp[key])
        for k, key in enumerate(sp.get("s", ())):
            a.s[k] = float(inp[key])
        if "theta" in inp:
            a.theta[:] = list(inp["theta"])
        return a

    def run(self, op, inp, f32=False, calls=1):
        """One case through the hook (``calls`` times on the same buffers).  Returns (outputs per call, init, ticket)."""
        ref = ec.reference(op, inp)
        bufs, init = self.buffers(op, inp, ref, f32)
        a = self.args(op, inp, bufs)
        outs = []
        for _ in range(calls):
            rc = self.hook(op, f32, a)
            assert rc == 0, self.last_error()
            torch.cuda.synchronize()
            outs.append({name: bufs[name].cpu().numpy() for name in ref})
        ticket = int(bufs["ticket"].cpu()[0]) if "ticket" in bufs else None
        return outs, init, ref, ticket


@pytest.fixture(scope="module")
def dev():
    return Device()


def verify(op, case, got, ref, init, f32=False):
    worst = 0.0
    for name, o in ref.items():
        ratio, msg = ec.check(op, name, got[name], o, init[name], f32)
        assert msg is None, f"{case}: {msg}"
        worst = max(worst, ratio)
    return worst


def run_cases(dev, op, twice=True):
    """Every fp64 case of the op against the reference; run twice on fresh buffers: the same bits."""
    for case in ec.CASES[op]:
        inp = ec.inputs(op, case)
        (got,), init, ref, _ = dev.run(op, inp)
        worst = verify(op, case, got, ref, init)
        print(f"{op} {case}: worst error / bound {worst:.3f}")
        if twice:
            (again,), _, _, _ = dev.run(op, inp)
            assert all(ec.same_bits(got[k], again[k]) for k in got), (op, case)


# ------------------------------------------------------------------ products and plain reductions
@pytest.mark.parametrize("op", ["trmv_lower", "trmv_lower_t", "symv_lower", "gemv_sub", "gemv_t_sub", "dot", "logdet",
                                "logdet_pair", "frob_lower", "frob_tiles", "reduce_slices", "reduce_slabs", "reduce_slices_sym"])
def test_sums_against_the_reference_and_bit_identical_twice(dev, op):
    run_cases(dev, op)


def test_reduce_slices_sym_is_exactly_symmetric(dev):
    for case in ec.CASES["reduce_slices_sym"]:
        inp = ec.inputs("reduce_slices_sym", case)
        (got,), _, _, _ = dev.run("reduce_slices_sym", inp)
        G = got["dst"].reshape(inp["n"], inp["n"])
        assert ec.same_bits(G, G.T.copy())


def test_frob_block_partials_are_in_row_major_tile_order(dev):
    """256 x 384: partial[ti * 3 + tj], element by element (a transposed or triangular order would move them)."""
    inp = ec.inputs("frob_tiles", (256, 384, 0))
    (got,), _, ref, _ = dev.run("frob_tiles", inp)
    T = inp["T"][:, :384]
    for ti in range(2):
        for tj in range(3):
            want = float(np.sum(T[ti * 128:(ti + 1) * 128, tj * 128:(tj + 1) * 128].astype(ec.LD) ** 2))
            assert abs(got["partial"][ti * 3 + tj] - want) <= 1e-12 * want, (ti, tj)
    assert len(set(np.round(got["partial"], 6))) == 6


def test_gemv_t_sub_refuses_a_column_count_off_the_multiple(dev):
    """cols = 65: -3 from the launcher before any launch, nothing written."""
    inp = ec.inputs("gemv_t_sub", (5, 64))
    ref = ec.reference("gemv_t_sub", inp)
    bufs, init = dev.buffers("gemv_t_sub", inp, ref, False)
    a = dev.args("gemv_t_sub", inp, bufs)
    a.n[1] = 65
    assert dev.hook("gemv_t_sub", False, a) == -3 and "multiple of 64" in dev.last_error()
    torch.cuda.synchronize()
    assert ec.same_bits(bufs["out"].cpu().numpy(), init["out"]) and bool(torch.isnan(bufs["partial"]).all())


def test_hook_refuses_what_could_become_a_wild_access(dev):
    inp = ec.inputs("trmv_lower_t", 128)
    ref = ec.reference("trmv_lower_t", inp)
    bufs, init = dev.buffers("trmv_lower_t", inp, ref, False)
    def bad(change, op="trmv_lower_t", f32=False, group=False):
        a = dev.args("trmv_lower_t", inp, bufs)
        change(a)
        return dev.hook(op, f32, a, group)
    assert bad(lambda a: a.p.__setitem__(2, None)) == -3 and "gpfit_dev_elementwise" in dev.last_error()
    assert bad(lambda a: a.n.__setitem__(0, 0)) == -3
    assert bad(lambda a: a.n.__setitem__(0, 100)) == -3           # np no multiple of 64
    assert bad(lambda a: None, op="symv_lower", f32=True) == -3    # no float instance
    assert bad(lambda a: setattr(a, "n_units", 17), group=True) == -3
    assert bad(lambda a: setattr(a, "n_units", 1), group=True) == -3   # no per-unit pointer tables
    assert dev.lib.gpfit_dev_elementwise(dev.ctx, dev.stream(), 99, 0, ctypes.byref(dev.args("trmv_lower_t", inp, bufs))) == -3
    torch.cuda.synchronize()
    assert ec.same_bits(bufs["z"].cpu().numpy(), init["z"])


# ------------------------------------------------------------------ layout ops
@pytest.mark.parametrize("op", ["pack_lower", "pack_tri", "unpack_sym", "unpack_tri", "symmetrize", "symmetrize_avg", "pad_copy",
                                "gather", "estep_build", "add_diag", "axpby_block", "demote_block"])
def test_layout_ops_exactly_and_nothing_else_touched(dev, op):
    run_cases(dev, op, twice=False)


# ------------------------------------------------------------------ the model's formulae
@pytest.mark.parametrize("op", ["qvec", "adjoint_rect", "dk_sigma0", "dq", "dk_metric", "estep_prep", "rowscale_add"])
def test_formula_ops_against_the_reference(dev, op):
    run_cases(dev, op, twice=False)


@pytest.mark.parametrize("op", ["moments", "metric_contract"])
def test_ticket_reductions_reset_their_ticket_and_repeat_their_bits(dev, op):
    for case in ec.CASES[op]:
        inp = ec.inputs(op, case)
        (first, second), init, ref, ticket = dev.run(op, inp, calls=2)
        worst = verify(op, case, first, ref, init)
        print(f"{op} {case}: worst error / bound {worst:.3f}")
        assert ticket == 0, (op, case, ticket)
        assert all(ec.same_bits(first[k], second[k]) for k in first), (op, case)


def run_adjoint(dev, inp, f32):
    """launch_adjoint and launch_adjoint_reduce behind it, on partial buffers that hold NaN where neither writes."""
    ref = ec.reference("adjoint", inp)
    R = np.float32 if f32 else np.float64
    n, npad = inp["n"], inp["np"]
    t = npad // 64
    up = lambda k: torch.from_numpy(np.ascontiguousarray(inp[k])).cuda()
    nan = lambda m: torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
    init = {"Aout": np.full(ref["Aout"].val.shape, ec.SENTINEL, R), "tvec": np.full(npad, ec.SENTINEL, R),
            "uq": np.full(npad, ec.SENTINEL), "scal": np.full(3, ec.SENTINEL)}
    out = {k: torch.from_numpy(v).cuda() for k, v in init.items()}
    W, Cos, b, q, wl = up("W"), up("Cos"), up("b"), up("q"), up("wl")
    upart, vpart, sumA = nan(t * npad), nan(t * npad), nan(t * (t + 1) // 2)
    a = dev._lib.DevEwArgs()
    for k, tsr in enumerate((W, Cos, b, q, out["Aout"], upart, vpart, sumA)):
        a.p[k] = tsr.data_ptr()
    a.ld[0], a.n[0], a.n[1] = inp["ld"], n, npad
    assert dev.hook("adjoint", f32, a) == 0, dev.last_error()
    r = dev._lib.DevEwArgs()
    for k, tsr in enumerate((upart, vpart, sumA, q, wl, out["tvec"], out["uq"], out["scal"])):
        r.p[k] = tsr.data_ptr()
    r.n[0], r.n[1], r.n[2], r.n[3] = n, npad, t, t * (t + 1) // 2
    assert dev.hook("adjoint_reduce", f32, r) == 0, dev.last_error()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, init, ref


@pytest.mark.parametrize("case", ec.CASES["adjoint"])
def test_adjoint_pass_and_its_reduce(dev, case):
    """The canonical lower triangle alone is the input (NaN above the diagonal of W and Cos); Aout on the lower 64-tiles
    with zeros above the diagonal inside the diagonal tiles, the tiles above untouched; tvec, uq and the three sums with
    zero padding."""
    inp = ec.inputs("adjoint", case)
    got, init, ref = run_adjoint(dev, inp, False)
    worst = verify("adjoint", case, got, ref, init)
    print(f"adjoint {case}: worst error / bound {worst:.3f}")
    again, _, _ = run_adjoint(dev, inp, False)
    assert all(ec.same_bits(got[k], again[k]) for k in got)


# ------------------------------------------------------------------ fp32 instances
@pytest.mark.parametrize("op", sorted(ec.F32_CASES))
def test_float_instances_on_the_smallest_multi_block_case(dev, op):
    case = ec.F32_CASES[op]
    inp = ec.inputs(op, case, np.float32)
    if op == "adjoint":
        got, init, ref = run_adjoint(dev, inp, True)
    else:
        (got,), init, ref, _ = dev.run(op, inp, f32=not (op == "reduce_slices" and inp["to32"]))
    worst = verify(op, case, got, ref, init, f32=True)
    print(f"{op} fp32 {case}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("n", ec.CASES["symmetrize"])
def test_symmetrize_float_at_every_size(dev, n):
    inp = ec.inputs("symmetrize", n, np.float32)
    (got,), init, ref, _ = dev.run("symmetrize", inp, f32=True)
    verify("symmetrize", n, got, ref, init, f32=True)
    A = got["A"][:, :n]
    assert ec.same_bits(A, A.T.copy()) and ec.same_bits(np.tril(A), np.tril(init["A"][:, :n]))


# ------------------------------------------------------------------ group forms
def repad(buf, ld, fill):
    out = np.full((buf.shape[0], ld), fill, dtype=buf.dtype)
    out[:, :min(ld, buf.shape[1])] = buf[:, :ld]
    return out


def group_inputs(op):
    """The three units of the op's group case, brought to the extents and leading dimensions the group form shares."""
    units = [ec.inputs(op, case, unit=u) for u, case in enumerate(ec.GROUP_CASES[op])]
    if op in ("pack_lower", "pack_tri"):
        for i in units:
            i["np"] = max(j["np"] for j in units)
    if op in ("symmetrize_avg", "logdet_pair"):
        ld = max(i["ld"] for i in units)
        for i in units:
            for key, fill in (("A", ec.SENTINEL), ("L0", np.nan), ("L1", np.nan)):
                if key in i:
                    i[key] = repad(i[key], ld, fill)
            i["ld"] = ld
    return units


# per-unit tables of the group forms: slot index -> key, for un / uld / us
PER_UNIT = {"pack_lower": dict(un={0: "n"}, uld={0: "ld"}), "pack_tri": dict(un={0: "n"}, uld={0: "ld"}),
            "pad_copy": dict(un={0: "rows", 1: "cols"}, uld={0: "ld"}), "gather": dict(un={0: "n", 1: "d"}, uld={0: "ldx"}),
            "qvec": dict(un={0: "n"}, us={0: "s0sq"}), "symmetrize_avg": dict(un={0: "n"}), "logdet_pair": dict(un={0: "n"})}


@pytest.mark.parametrize("op", sorted(ec.GROUP_CASES))
def test_group_forms_give_the_bits_of_the_single_form(dev, op):
    """Three units with different data (different extents where the form takes them) in one launch: every unit's output
    bit-equal to the single form on that unit's data -- the same body, whatever the grid -- and within the bounds."""
    units = group_inputs(op)
    if op == "qvec":
        for u, i in enumerate(units):
            i["s0sq"] = i["s0sq"] + u
    single = []
    for i in units:
        (got,), init, ref, _ = dev.run(op, i)
        single.append(got)
    refs = [ec.reference(op, i) for i in units]
    made = [dev.buffers(op, i, r, False) for i, r in zip(units, refs)]
    a = dev.args(op, units[0], made[0][0])
    nu = len(units)
    a.n_units = nu
    keep = []
    for k, slot in enumerate(SPEC[op]["p"]):
        name = slot[0] if isinstance(slot, tuple) else slot.lstrip("?")
        if all(name in bufs for bufs, _ in made):
            arr = (ctypes.c_void_p * nu)(*[bufs[name].data_ptr() for bufs, _ in made])
            keep.append(arr)
            a.up[k] = ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p))
    for field, ctype in (("un", ctypes.c_int32), ("uld", ctypes.c_int64), ("us", ctypes.c_double)):
        for k, key in PER_UNIT.get(op, {}).get(field, {}).items():
            arr = (ctype * nu)(*[i[key] for i in units])
            keep.append(arr)
            getattr(a, field)[k] = ctypes.cast(arr, ctypes.POINTER(ctype))
    assert dev.hook(op, False, a, group=True) == 0, dev.last_error()
    torch.cuda.synchronize()
    for u, ((bufs, init), ref) in enumerate(zip(made, refs)):
        got = {name: bufs[name].cpu().numpy() for name in ref if name != "Xm"}
        for name in got:
            assert ec.same_bits(got[name], single[u][name]), (op, u, name)
        worst = verify(op, ec.GROUP_CASES[op][u], got, {k: ref[k] for k in got}, init)
        print(f"{op} group unit {u}: worst error / bound {worst:.3f}")
