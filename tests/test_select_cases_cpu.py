"""The CPU arithmetic behind the tests of the batch-aware selection (select_cases.py) checked against itself: the
long-double recurrence equals exact Gaussian conditioning by a dense solve; every step of every case that is not a
deliberate tie separates its pick from the runner-up by a relative gap of at least 1e-6 (what lets the GPU tests demand
equal picks); the duplicate pool shows what the rule is for; at A = 0.05 the rule degenerates to the top-B."""
import numpy as np
import pytest

import predict_cases as cases
import select_cases as sel

LD = np.longdouble
GAP = 1e-6


def _check_conditioning(Sigma, ref, unit=0):
    picks = [i for i in ref["picked"] if i >= 0]
    exact = sel.exact_conditioning(Sigma, picks, ref["tau"][unit])
    return float(np.max(np.abs(ref["sigma2"][unit] - exact)) / np.max(np.abs(np.diag(Sigma))))


@pytest.mark.parametrize("name", sorted(sel.SINGLE))
def test_recurrence_is_exact_conditioning_and_every_step_has_a_gap(name):
    Sigma, _ = sel.single_inputs(name)
    ref = sel.single_reference(name)
    n_select = sel.SINGLE[name][2]
    assert len(set(ref["picked"])) == n_select and min(ref["picked"]) >= 0
    e = _check_conditioning(Sigma, ref)
    print(f"\n{name}: conditioning against the dense solve {e:.2e}, smallest gap {min(ref['gap']):.2e}")
    assert e <= 1e-16                 # long double on both sides: eps = 1.1e-19, up to 128 terms per sum
    assert min(ref["gap"]) >= GAP


@pytest.mark.parametrize("name", sorted(sel.UNITS))
def test_units_recurrence_and_gap(name):
    inp = sel.unit_inputs(name)
    ref = sel.unit_reference(name)
    assert len(set(ref["picked"])) == sel.UNITS[name][2]
    worst = max(_check_conditioning(inp[u][0], ref, u) for u in range(len(inp)))
    print(f"\n{name}: conditioning {worst:.2e}, smallest gap {min(ref['gap']):.2e}")
    assert worst <= 1e-16
    assert min(ref["gap"]) >= GAP


def test_fp64_transcription_follows_the_reference():
    for name in sorted(sel.SINGLE):
        Sigma, mu = sel.single_inputs(name)
        _, A, n_select = sel.SINGLE[name]
        ref = sel.single_reference(name)
        f64 = sel.greedy_f64([Sigma], [mu], [A], [sel.LAMBDA0], None, n_select)
        assert f64["picked"] == ref["picked"]
        e = float(np.max(np.abs(f64["sigma2"][0].astype(LD) - ref["sigma2"][0])) / np.max(np.diag(Sigma)))
        print(f"\n{name}: fp64 transcription, conditional variances {e:.2e}")
        assert e <= 1e-12                 # fp64: eps = 2.2e-16 over up to 128 rank-1 updates of 300 rows


def test_duplicates_take_one_slot_each():
    Sigma, mu = sel.duplicate_inputs()
    ref = sel.duplicate_reference()
    picked = ref["picked"]
    top = sel.top_b(ref["T"][0], 8)
    print(f"\nduplicate pool: top-8 {top}, greedy {picked}, gaps {['%.1e' % g for g in ref['gap']]}")
    for row, copy, _ in sel.DUPLICATES:
        assert row in top and copy in top                       # the top-B spends two slots on each pair
        assert (row in picked) + (copy in picked) == 1          # the greedy rule one
    # the exact copy ties with its original at step 0, bit for bit; the lowest index wins
    assert ref["T"][0][20] == ref["T"][0][21] and ref["gap"][0] == 0.0
    assert picked[0] == 20 and 21 not in picked
    # every other step has its gap, among the rows still worth a slot
    assert min(ref["gap"][1:]) >= GAP
    # the copy's variance collapses once the original is chosen
    one = sel.greedy_reference([Sigma], [mu], [1.0], [sel.LAMBDA0], None, 1)
    assert one["sigma2"][0][21] < 1e-2 * Sigma[21, 21]


def test_exhaustion_and_non_finite_rows():
    Sigma, mu = sel.single_inputs("identity130")
    ref = sel.greedy_reference([Sigma[:5, :5]], [mu[:5]], [1.0], [sel.LAMBDA0], None, 8)
    assert sorted(ref["picked"][:5]) == [0, 1, 2, 3, 4] and ref["picked"][5:] == [-1, -1, -1]
    assert all(np.isnan(u) for u in ref["utility"][5:])
    dead = np.array(Sigma[:40, :40])
    dead[7, :] = 0.0              # variance zero and no covariance: the row's utility is NaN at every step
    dead[:, 7] = 0.0
    ref = sel.greedy_reference([dead], [mu[:40]], [1.0], [sel.LAMBDA0], None, 8)
    assert all(not np.isfinite(T[7]) for T in ref["T"]) and 7 not in ref["picked"] and min(ref["picked"]) >= 0


def test_weak_link_degenerates_to_the_top_b():
    """A = 0.05 (synthetic.F_PARAMS): tau is in the hundreds, one presentation conditions nothing."""
    Sigma, mu = sel.single_inputs("identity130")
    ref = sel.greedy_reference([Sigma], [mu], [0.05], [sel.LAMBDA0], None, 8)
    assert min(ref["tau"][0]) > 100.0
    assert ref["picked"] == sel.top_b(ref["T"][0], 8)
