"""bench.py --dump-outputs writes what the last timed step returned, so that two builds can be compared output for
output; a plain run prints only the headline line (the roofline, in-flight and CPU legs are --full).  The helpers
and the argument checks run on the CPU; one GPU test runs the benchmark end to end at a small size and compares its
dump with a direct evaluation of the same seeded inputs."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_step_arrays_of_an_evaluation_and_of_a_table(tmp_path):
    bench = load_bench()
    keys = bench.syn.THETA_KEYS
    res = {"loss": 1.5, "loglik": -2.0, "grad": {k: float(i) for i, k in enumerate(keys)}, "d": 7, "in_bounds": True,
           "lam_m": None, "f": torch.arange(4, dtype=torch.float32)}
    arrays = bench.step_arrays(res)
    assert sorted(arrays) == ["d", "f", "grad", "in_bounds", "loglik", "loss"]
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert arrays["loss"].shape == () and float(arrays["loss"]) == 1.5
    assert np.array_equal(arrays["grad"], np.arange(len(keys), dtype=np.float64))
    assert np.array_equal(arrays["f"], np.arange(4.0))
    table = torch.arange(14, dtype=torch.float64).reshape(2, 7)
    assert list(bench.step_arrays({"loss": 0.0}, table)) == ["results"]

    bench.dump_outputs(str(tmp_path / "out"), arrays)
    for name, a in arrays.items():
        b = np.load(tmp_path / "out" / f"{name}.npy")
        assert b.dtype == np.float64 and np.array_equal(a, b)


def test_dump_outputs_refuses_more_than_64_mib(tmp_path):
    bench = load_bench()
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path), {"big": np.zeros((64 << 20) // 8 + 1)})
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked_before_any_work(argv):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--steps must be at least 1" in p.stderr, p.stderr[-2000:]


@pytest.mark.gpu
def test_plain_run_is_lean_and_its_dump_matches_a_direct_evaluation(tmp_path):
    N, d, steps = 1024, 256, 3
    out = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--n", str(N), "--d", str(d), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == steps and line["dtype"] == "f64" and line["ms_per_step"] > 0
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) < 1e-2 * line["value"]
    for key in ("roofline", "cpu_baseline", "independent_units_in_flight"):
        assert key not in line, key

    bench = load_bench()
    syn = bench.syn
    loss, grad = np.load(out / "loss.npy"), np.load(out / "grad.npy")
    assert loss.dtype == grad.dtype == np.float64 and grad.shape == (len(syn.THETA_KEYS),)
    assert float(loss) == line["loss"]

    dev = torch.device("cuda:0")
    grid = syn.grid_for(d)
    lower, upper = syn.limits()
    X = torch.from_numpy(syn.stimuli(N, d)).to(dev)
    r_np, m_np = syn.cell_inputs(N, 0)
    V = bench.build_V(X, grid, syn.theta0(0), dev)
    eng = bench.GPFitEngine(N, d)
    try:
        ref = eng.fit_eval(syn.theta_eval(0), lower, upper, grid, X, torch.from_numpy(r_np).to(dev),
                           torch.from_numpy(m_np).to(dev), V, syn.F_PARAMS["logA"], syn.F_PARAMS["lambda0"], want_vectors=False)
    finally:
        eng.close()
    g_ref = np.array([ref["grad"][k] for k in syn.THETA_KEYS])
    assert abs(float(loss) - ref["loss"]) <= 1e-12 * abs(ref["loss"])
    assert np.max(np.abs(grad - g_ref)) <= 1e-10 * np.max(np.abs(g_ref))
    for name in ("loglik", "KL", "logdet_K", "logdet_V"):
        assert abs(float(np.load(out / f"{name}.npy")) - ref[name]) <= 1e-12 * max(1.0, abs(ref[name])), name
