"""What every context entry point leaves behind for the next call, and what it makes of what the last one left
(the probes of tests/context_cases.py, one call of one entry point each, on contexts of this module's own).

A fit keeps one context for its whole run, so every call finds the work buffers holding the remains of another call, of
another size and precision.  Three contracts carry that, and all three are checked here by bit equality -- no tolerance:

* poison: a call's outputs do not depend on what the work buffers held.  Every floating-point work buffer of the context
  (``gpfit_dev_ctx_buffer_name``: the table of csrc/api_dev.hip, capacity behind the padded problem included) is filled
  with byte 0xFF -- NaN as fp64 and as fp32 -- then with 0x47 -- finite and far from the data, for the clips and
  comparisons that swallow NaN -- and the call gives the bits it gave on the fresh context.  Of a group only unit 1's
  context is poisoned, and every unit keeps its bits.
* cache: whatever runs between two evaluations of one M-step, the second (``reuse_V``) has the bits of the first --
  because the entry point in between left V's factor alone (``KEEPS``) or said that it did not (``DROPS``).  Which of the
  two happened is read from the flops the second evaluation executed (``set_profile(1)``): those of a reuse directly
  behind the first, or those of a fresh evaluation, both measured in the same test; and it is the class the registry
  states from the source.
* pending: while an asynchronous evaluation is in flight on a context, every entry point refuses (-3, "pending") and
  writes nothing; the evaluation is then collected with the bits of the synchronous one, and the call succeeds with its
  own.

The poison never reaches a buffer whose contents are an index or a ticket (pix, info, the chain block: not in the
table).  No context of this module goes back to a pool: each test creates its own and destroys them."""
import ctypes

import pytest
import torch

import context_cases as cc
from gaussian_processes_amd import _lib
from gaussian_processes_amd.engine import GPFitEngine

pytestmark = pytest.mark.gpu
INSTANCES = ("f64", "mixed", "f32")


def ids(probes):
    return [p.name for p in probes]


class engines:
    """One context per unit of the probe, this test's own, destroyed on the way out."""

    def __init__(self, probe):
        cap = cc.CAP_LARGE if probe in cc.LARGE else cc.CAP
        self.engines = [GPFitEngine(cap, cc.D_FULL, cc.D_FULL) for _ in range(probe.units)]

    def __enter__(self):
        return self.engines

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        for e in self.engines:
            e.close()


def run(call, what):
    """The call made and checked, and what it wrote."""
    rc = call.run()
    assert rc == 0, (what, rc, _lib.last_error())
    got = cc.collect(call)
    assert len(cc.untouched(got)) < len(got), (what, "the call wrote nothing")
    return got


def flops(eng):
    p = eng.get_profile()
    return tuple(p[k] for k in ("gemm_flops", "gemm_launches", "leaf_launches", "gram_flops", "small_gemm_flops",
                                "small_gemm_launches"))


@pytest.mark.parametrize("probe", cc.PROBES + cc.LARGE, ids=ids(cc.PROBES + cc.LARGE))
def test_outputs_do_not_depend_on_stale_workspace(probe):
    with engines(probe) as engs:
        want = run(probe.build(engs), (probe.name, "fresh"))
        victim = engs[1 if probe.units > 1 else 0]
        for byte in cc.POISON:
            cc.fill_workspace(victim, byte)
            got = run(probe.build(engs), (probe.name, hex(byte)))
            bad = cc.differences(got, want)
            assert not bad, f"{probe.name}: behind a workspace of {byte:#x} bytes these outputs lost the bits of the fresh context: {bad}"


@pytest.mark.parametrize("instance", INSTANCES)
@pytest.mark.parametrize("probe", cc.SINGLE, ids=ids(cc.SINGLE))
def test_the_cached_factor_of_V_survives_or_is_dropped(probe, instance):
    with engines(probe) as (eng,):
        eng.set_profile(1)
        base = run(cc.base_eval(eng, instance), "base")
        fresh = flops(eng)
        reused = run(cc.base_eval(eng, instance, reuse_V=True), "reuse behind base")
        reuse = flops(eng)
        assert not cc.differences(reused, base) and reuse != fresh, (reuse, fresh)     # the two references tell apart
        run(probe.build([eng]), probe.name)
        again = run(cc.base_eval(eng, instance, reuse_V=True), "reuse behind " + probe.name)
        executed = flops(eng)
        bad = cc.differences(again, base)
        assert not bad, f"reuse_V behind {probe.name} ({instance}): {bad} lost the bits of the first evaluation"
        assert executed in (reuse, fresh), (executed, reuse, fresh)
        measured = cc.KEEPS if executed == reuse else cc.DROPS
        print(f"{probe.name} ({instance}): {measured}")
        assert measured == probe.cache, f"{probe.name} ({instance}) {measured} V's cached factor; the registry says {probe.cache}"


@pytest.mark.parametrize("between", ["potrf", "elbo"])
def test_a_group_reuses_its_cached_factors_unit_by_unit(between):
    """Three contexts hold cached factors; a call that keeps (potrf) or drops (elbo) the cache runs on one of them;
    gpfit_fit_eval_batch with reuse_V then gives every unit the bits of its first evaluation."""
    group = cc.BY_NAME["fit_eval_batch"]
    with engines(group) as engs:
        base = run(cc._fit_batch(engs, False, 1), "base")
        run(cc.BY_NAME[between].build([engs[1]]), between)
        again = run(cc._fit_batch(engs, False, 1 | 2), "reuse behind " + between)
        assert not cc.differences(again, base)


@pytest.mark.parametrize("probe", cc.PROBES, ids=ids(cc.PROBES))
def test_every_entry_point_refuses_while_an_evaluation_is_pending(probe):
    lib = _lib.load()
    with engines(probe) as engs:
        busy = engs[1 if probe.units > 1 else 0]
        want = run(probe.build(engs), (probe.name, "reference"))
        sync = run(cc.base_eval(busy, "f64"), "synchronous")
        flight = cc.base_eval(busy, "f64", async_call=True)
        assert flight.run() == 0
        call = probe.build(engs)
        before = cc.collect(call)
        rc = call.run()
        why = _lib.last_error()
        assert rc == -3 and "pending" in why, (probe.name, rc, why)
        assert why.startswith(probe.entry.replace("_f32", "") + ":"), (probe.name, why)     # this call's refusal, not an older one's
        assert not cc.differences(cc.collect(call), before), f"{probe.name} wrote while it refused"
        out = (ctypes.c_double * 16)()
        assert lib.gpfit_fit_eval_finish(busy._ctx, out) == 0, _lib.last_error()
        flight.outs["out"][:] = list(out)
        assert not cc.differences(cc.collect(flight), sync)
        assert not cc.differences(run(call, (probe.name, "behind the collect")), want)
