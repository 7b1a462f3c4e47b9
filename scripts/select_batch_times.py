"""utils.select_round against the selection the examples do by default, utils.score_pool_cells followed by torch.topk
(profiles/r27_select_batch.txt): `python scripts/select_batch_times.py`.

Pools of 4096 images against 512 inducing images and of 20000 against 2100, d = 64, identity basis, 100 response counts,
A = 1 and lambda0 = -0.3 (at the synthetic A = 0.05 the rule degenerates to the top-B), for one cell and for 16 cells, at
n_select 8, 32 and 128 with the default shortlist of 1024.  Both sides warm and alternated in one process, five timed
repetitions: median (min .. max) of the host clock around calls that end in a device synchronisation.  Beside them one
pool_covariance call on the shortlist and the select_batch call alone (2 n_select + 1 launches), and how many of the
picks the top-B shares."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussian_processes_amd import synthetic as syn  # noqa: E402
from gaussian_processes_amd import utils as gp  # noqa: E402


def say(*a):
    print(" ".join(str(x) for x in a), flush=True)


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def make_cell(cell, nt, theta, C, d):
    xt = torch.from_numpy(syn.stimuli(nt, d, seed=900 + cell)).cuda()
    Kt = gp.acosker(theta, xt, xt, C=C)
    Kt = 0.5 * (Kt + Kt.T) + 1e-6 * torch.eye(nt, dtype=torch.float64, device="cuda")
    Kinv = torch.linalg.inv(Kt)
    Kinv = 0.5 * (Kinv + Kinv.T)
    g = torch.Generator(device="cpu").manual_seed(cell)
    G = torch.diag(0.05 + 0.1 * torch.rand(nt, dtype=torch.float64, generator=g)).cuda()
    V = torch.linalg.inv(Kinv + G)
    V = 0.5 * (V + V.T)
    m = (0.3 * torch.randn(nt, dtype=torch.float64, generator=g)).cuda()
    B = gp._mark_identity(torch.eye(nt, dtype=torch.float64, device="cuda"))
    folded = gp.fold_posterior(Kt, Kinv, m, V, B)
    del B
    return {"xtilde": xt, "C": C, "theta": theta, "folded": folded,
            "f_params": {"logA": torch.tensor(0.0, dtype=torch.float64), "lambda0": torch.tensor(-0.3, dtype=torch.float64)}}


def main():
    lower, upper = syn.limits()
    theta = {k: torch.tensor(float(v), dtype=torch.float64) for k, v in syn.theta0().items()}
    C, mask = gp.localker(theta, upper, lower, 8)
    d = 64
    assert int(mask.sum()) == d
    counts = torch.arange(0, 100, dtype=torch.float64).cuda()
    say("ms, median (min .. max) of 5 warm runs, baseline and select_round alternated; A = 1, lambda0 = -0.3, shortlist 1024")
    for P, nt in ((4096, 512), (20000, 2100)):
        pool = torch.from_numpy(syn.stimuli(P, d, seed=5)).cuda()
        all_cells = [make_cell(c, nt, theta, C, d) for c in range(16)]
        for n_cells in (1, 16):
            cells = all_cells[:n_cells]

            def base(b):
                s = gp.score_pool_cells(pool, cells, r_masked=counts)
                return torch.topk(s["population_utility"], b).indices

            for b in (8, 32, 128):
                base(b)
                out = gp.select_round(pool, cells, b, counts)          # warm-up of both
                rb, rn = [], []
                for _ in range(5):
                    rb.append(timed(lambda: base(b), 1)[0])
                    rn.append(timed(lambda: gp.select_round(pool, cells, b, counts), 1)[0])
                keep = out["shortlist"]
                rows = pool[keep].contiguous()
                c0 = cells[0]
                cov = timed(lambda: gp.pool_covariance(rows, c0["xtilde"], c0["C"], c0["theta"], c0["folded"]), 5)
                Sig = [gp.pool_covariance(rows, c["xtilde"], c["C"], c["theta"], c["folded"]) for c in cells]
                mus = [out["scores"]["mu"][u][keep] for u in range(n_cells)]
                fps = [c["f_params"] for c in cells]
                loop = timed(lambda: gp.select_batch(Sig, mus, fps, counts, b), 5)
                top = set(torch.topk(out["scores"]["population_utility"], b).indices.tolist())
                same = len(top & set(out["picked"].tolist()))
                say(f"P {P} nt {nt} cells {n_cells} n_select {b}: topk baseline {np.median(rb):.2f} ({min(rb):.2f} .. {max(rb):.2f})"
                    f" | select_round {np.median(rn):.2f} ({min(rn):.2f} .. {max(rn):.2f})"
                    f" | one pool_covariance (M {rows.shape[0]}) {cov[0]:.2f} ({cov[1]:.2f} .. {cov[2]:.2f})"
                    f" | select_batch alone, {2 * b + 1} launches {loop[0]:.2f} ({loop[1]:.2f} .. {loop[2]:.2f})"
                    f" | picks shared with the top-{b}: {same}")
                del Sig
        del all_cells, pool
        torch.cuda.empty_cache()


main()
