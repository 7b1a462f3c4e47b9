"""utils.score_pool_cells against a loop of utils.score_pool calls over the same cells (profiles/r26_score_pool_group.txt):
`python scripts/score_pool_group_times.py`.

16 cells on one pool, d = 256, 100 response counts, at the shapes of scripts/score_pool_times.py.  The loop is what a
population's closed loop did before the group call: score_pool cell after cell and the utilities added up with torch.
The group side is one score_pool_cells call: the cells of a bucket in device calls of up to 16 units
(gpfit_score_pool_batch) and the sum by gpfit_utility_sum.  Both sides warm and alternated in one process, ``--reps``
timed repetitions behind 2 warm-up rounds; median and range of the host clock around calls that end in a device
synchronisation.  The cells share the inducing images and the basis (one eigendecomposition per shape) as separate
tensors, and differ in their posteriors.  Every cell's results are compared bit for bit between the two sides."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussian_processes_amd import synthetic as syn  # noqa: E402
from gaussian_processes_amd import utils as U  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--cells", type=int, default=16)
ap.add_argument("--max-pool", type=int, default=20000, help="skip the shapes with a larger pool")
ap.add_argument("--max-nt", type=int, default=4096, help="skip the shapes with more inducing images")
args = ap.parse_args()

dev = torch.device("cuda")
LOWER, UPPER = syn.limits()
PX = 16
theta = {k: torch.tensor(float(v), dtype=torch.float64) for k, v in syn.theta0().items()}
r_counts = torch.arange(0, 100, dtype=torch.float64).to(dev)
SHAPES = [(4096, 512, 512, "identity"), (20000, 2100, 2100, "identity"), (20000, 2100, 2100, "eigenbasis"),
          (20000, 4096, 515, "truncated")]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def same_bits(a, b):
    return bool((a.view(torch.int64) == b.view(torch.int64)).all())


for P, nt, k, basis in [s for s in SHAPES if s[0] <= args.max_pool and s[1] <= args.max_nt]:
    X = torch.from_numpy(syn.stimuli(P + nt, PX * PX, seed=3)).to(dev)
    xstar, xtilde = X[:P].contiguous(), X[P:].contiguous()
    C, mask = U.localker(theta, UPPER, LOWER, PX)
    xt_m = xtilde[:, mask].contiguous()
    Kt = U.acosker(theta, xt_m, xt_m, C=C)
    if basis == "identity":
        B = U._mark_identity(torch.eye(nt, dtype=torch.float64, device=dev))
        K_b, Kinv_b = Kt, U.spd_inverse(Kt)
    else:
        ev, evec = torch.linalg.eigh(Kt)
        B = evec[:, nt - k:].contiguous()
        K_b, Kinv_b = torch.diag(ev[nt - k:]), torch.diag(1 / ev[nt - k:])
    cells = []
    for cell in range(args.cells):
        g = torch.Generator(device="cpu").manual_seed(5 + cell)
        R = torch.randn(k, k, dtype=torch.float64, generator=g).to(dev)
        V_b = U.spd_inverse(Kinv_b + U.matmul(R, R, transB=True) / (10 * k))
        V_b = 0.5 * (V_b + V_b.T)
        m_b = torch.randn(k, dtype=torch.float64, generator=g).to(dev)
        own_B = B if basis == "identity" else B.clone()
        cells.append({"xtilde": xtilde.clone(), "C": C.clone(), "theta": theta, "mask": mask,
                      "folded": U.fold_posterior(K_b, Kinv_b, m_b, V_b, own_B),
                      "f_params": {"logA": torch.tensor(syn.F_PARAMS["logA"] + 0.01 * cell),
                                   "lambda0": torch.tensor(syn.F_PARAMS["lambda0"])}})
        del R, V_b

    def loop():
        outs = [U.score_pool(xstar, c["xtilde"], c["C"], c["theta"], c["folded"], c["f_params"], r_masked=r_counts, mask=c["mask"])
                for c in cells]
        total = outs[0]["utility"]
        for o in outs[1:]:
            total = total + o["utility"]
        return outs, total

    def group():
        return U.score_pool_cells(xstar, cells, r_masked=r_counts)

    arms = {"loop of score_pool + torch sum": loop, "score_pool_cells (group calls)": group}
    times = {name: [] for name in arms}
    warm = 2
    for i in range(args.reps + warm):
        for name, fn in arms.items():
            t, _ = timed(fn)
            if i >= warm:
                times[name].append(t)
    outs, total = loop()
    res = group()
    sizes = list(U.last_pool_group_sizes)
    torch.cuda.synchronize()
    equal = all(same_bits(res[key][i], o[key]) for i, o in enumerate(outs) for key in ("mu", "sigma2", "rate", "utility"))
    equal_sum = same_bits(res["population_utility"], total)
    chunks = -(-P // 4096)
    per_call = (6 if basis != "identity" else 5) + chunks * (8 if basis != "identity" else 7)
    print(f"--- {args.cells} cells, P = {P}, nt = {nt}, k = {k}, {basis} basis, d = {int(mask.sum())}, nr = {r_counts.numel()}; "
          f"units per group call {sizes}; launches: {per_call} per device call, so {args.cells * per_call} + {args.cells - 1} "
          f"additions by the loop, {len(sizes) * per_call} + 1 sum by the group side")
    med = {name: float(np.median(ts)) for name, ts in times.items()}
    first = next(iter(arms))
    for name, ts in times.items():
        print(f"    {name:34s} median {med[name]:9.3f} ms   min {min(ts):9.3f}   max {max(ts):9.3f}   "
              f"per cell {med[name] / args.cells:7.3f} ms   ratio to the loop {med[name] / med[first]:.3f}")
    print(f"    every cell's mu, sigma2, rate, utility bit-identical: {equal}; population utility bit-identical: {equal_sum}",
          flush=True)
    del X, xstar, xtilde, Kt, K_b, Kinv_b, B, cells, outs, res, total
    torch.cuda.empty_cache()
