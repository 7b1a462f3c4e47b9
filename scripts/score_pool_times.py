"""utils.score_pool against the present composition (profiles/r25_score_pool.txt): `python scripts/score_pool_times.py`.

The composition is the scoring step of examples/active_learning.py without --score-call, line for line: acosker(diag),
the rectangular acosker times B (torch), lambda_moments, nd_utility, on whole images indexed by the mask.  The call is
fold_posterior once per model (timed on its own) and score_pool(..., mask=mask) with chunk_rows = the model's padded
size, 0 (one chunk: the composition has grown the workspace to the pool by then), 4096 (what the default gives in a
workspace that only score_pool sized, utils.POOL_ROWS) and 8192.  All arms warm and alternated in one process, 7 timed
repetitions behind 2 warm-up rounds; median and range of the host clock around calls that end in a device
synchronisation.  The last columns: the largest deviation of the call's mu, sigma2 and utility from the composition's,
relative to max |.|, and whether both pick the same image.

Shapes (P, nt, k): (4096, 512, 512) and (20000, 2100, 2100) in the identity basis, (20000, 2100, 2100) in the eigenbasis
of K~, (20000, 4096, 515) truncated to the top 515 eigenvectors; d = 256, nr = 100.  Inputs: synthetic stimuli,
theta0, V = (K~_b^-1 + R R^T / (10 k))^-1 with R ~ N(0, 1), m ~ N(0, 1)."""
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--max-pool", type=int, default=20000, help="skip the shapes with a larger pool")
args = ap.parse_args()

dev = torch.device("cuda")
LOWER, UPPER = syn.limits()
PX = 16
theta = {k: torch.tensor(float(v), dtype=torch.float64) for k, v in syn.theta0().items()}
fp = {"logA": torch.tensor(syn.F_PARAMS["logA"]), "lambda0": torch.tensor(syn.F_PARAMS["lambda0"])}
r_counts = torch.arange(0, 100, dtype=torch.float64)
SHAPES = [(4096, 512, 512, "identity"), (20000, 2100, 2100, "identity"), (20000, 2100, 2100, "eigenbasis"),
          (20000, 4096, 515, "truncated")]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


for P, nt, k, basis in [s for s in SHAPES if s[0] <= args.max_pool]:
    X = torch.from_numpy(syn.stimuli(P + nt, PX * PX, seed=3)).to(dev)
    xstar, xtilde = X[:P].contiguous(), X[P:].contiguous()
    C, mask = U.localker(theta, UPPER, LOWER, PX)
    xt_m = xtilde[:, mask].contiguous()
    Kt = U.acosker(theta, xt_m, xt_m, C=C)
    g = torch.Generator(device="cpu").manual_seed(5)
    if basis == "identity":
        B = U._mark_identity(torch.eye(nt, dtype=torch.float64, device=dev))
        K_b, Kinv_b = Kt, U.spd_inverse(Kt)
    else:
        ev, evec = torch.linalg.eigh(Kt)
        B = evec[:, nt - k:].contiguous()
        K_b, Kinv_b = torch.diag(ev[nt - k:]), torch.diag(1 / ev[nt - k:])
    R = torch.randn(k, k, dtype=torch.float64, generator=g).to(dev)
    V_b = U.spd_inverse(Kinv_b + U.matmul(R, R, transB=True) / (10 * k))
    V_b = 0.5 * (V_b + V_b.T)
    m_b = torch.randn(k, dtype=torch.float64, generator=g).to(dev)
    A, lambda0 = torch.exp(fp["logA"]), fp["lambda0"]

    def composition():
        Kvec_star = U.acosker(theta, xstar[:, mask], x2=None, C=C, dC=None, diag=True)
        K_star_b = U.acosker(theta, xstar[:, mask], x2=xtilde[:, mask], C=C, dC=None, diag=False) @ B
        lam_m, lam_var = U.lambda_moments(xstar[:, mask], K_b, K_star_b @ Kinv_b, Kvec_star, K_star_b, C, m_b, V_b, theta)
        return lam_m, lam_var, U.nd_utility(A ** 2 * lam_var, A * lam_m + lambda0, r_counts)

    timed(lambda: U.fold_posterior(K_b, Kinv_b, m_b, V_b, B))
    t_fold, folded = timed(lambda: U.fold_posterior(K_b, Kinv_b, m_b, V_b, B))
    model_rows = (max(nt, k) + 127) // 128 * 128

    def call(chunk_rows):
        return U.score_pool(xstar, xtilde, C, theta, folded, fp, r_masked=r_counts, mask=mask, chunk_rows=chunk_rows)

    arms = {"composition": composition, f"score_pool chunk_rows={model_rows} (model-sized)": lambda: call(model_rows),
            "score_pool chunk_rows=0 (one chunk)": lambda: call(0),
            "score_pool chunk_rows=4096 (default)": lambda: call(4096), "score_pool chunk_rows=8192": lambda: call(8192)}
    times = {name: [] for name in arms}
    warm = 2
    for i in range(args.reps + warm):
        for name, fn in arms.items():
            t, _ = timed(fn)
            if i >= warm:
                times[name].append(t)
    lam_m, lam_var, u = composition()
    new = call(4096)
    torch.cuda.synchronize()
    print(f"--- P = {P}, nt = {nt}, k = {k}, {basis} basis, d = {int(mask.sum())}, nr = {r_counts.numel()} "
          f"(fold_posterior, once per model: {t_fold:.2f} ms)")
    med = {name: float(np.median(ts)) for name, ts in times.items()}
    for name, ts in times.items():
        print(f"    {name:46s} median {med[name]:8.3f} ms   min {min(ts):8.3f}   max {max(ts):8.3f}   "
              f"ratio to the composition {med[name] / med['composition']:.3f}")
    print(f"    agreement with the composition: mu {rel(new['mu'], lam_m):.2e} sigma2 {rel(new['sigma2'], lam_var):.2e} "
          f"utility {rel(new['utility'], u):.2e}; same image picked: {int(new['utility'].argmax()) == int(u.argmax())}", flush=True)
    del X, xstar, xtilde, Kt, K_b, Kinv_b, V_b, B, folded, new, lam_m, lam_var, u
    torch.cuda.empty_cache()
