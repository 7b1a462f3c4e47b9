"""The fused loss against the composite (profiles/r22_elbo.txt): `python scripts/elbo_times.py --part single|group`.

single: utils.elbo_terms with the switch off (compute_loglikelihood + compute_KL_div: two factorisations, the product
V K~^-1, one matmul, four reductions) against the switch on (gpfit_elbo), without and with log|K~| given, on the same
inputs at (N, nb) = (512, 512), (1024, 1024), (3160, 541), (2048, 2048), (4096, 4096): all three warm, alternated in one
process (composite, fused, fused with logdet, composite, ...), 7 timed repetitions behind 2 warm-up rounds; median and
range of the host clock around calls that end with both numbers read back (float()), as varGP reads them.  The last
columns: the largest relative deviation of the fused (loglik, KL) from the composite's.

group: one gpfit_elbo_batch call of 16 units against 16 gpfit_elbo calls on the same 16 workspaces, at (512, 512) and
(3160, 541), alternated the same way; K~ factored in the call.

Inputs: K~ = G G^T / nb + I / 10 with G ~ N(0, 1), K~^-1 from the library's factor (symmetrised), V = the full Newton
step's posterior at a rate f = exp(0.35 z - 0.3), r ~ Poisson(f), m, lam_m ~ N(0, 1)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gaussian_processes_amd import utils as gp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=("single", "group"), required=True)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--shapes", type=int, nargs="+", default=None)
ap.add_argument("--units", type=int, default=16)
args = ap.parse_args()
dev = torch.device("cuda:0")
shapes = args.shapes or ([512, 512, 1024, 1024, 3160, 541, 2048, 2048, 4096, 4096] if args.part == "single"
                         else [512, 512, 3160, 541])


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def inputs(N, nb, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64, device=dev, generator=gen)
    G = rnd(nb, nb)
    K = gp.matmul(G, G, transB=True) / nb
    K = (K + K.T) / 2 + 0.1 * torch.eye(nb, dtype=torch.float64, device=dev)
    L, Li, logdet, info = gp.cholesky(K, want_inverse=True)
    assert info == 0
    Kinv = gp.matmul(Li, Li, transA=True)
    Kinv = (Kinv + Kinv.T) / 2
    a = rnd(N, nb) / nb ** 0.5
    f = torch.exp(0.35 * rnd(N) - 0.3)
    r = torch.poisson(f, generator=gen)
    fp = {"logA": torch.tensor(0.1, dtype=torch.float64), "lambda0": torch.tensor(-0.3, dtype=torch.float64)}
    _, V = gp._estep_projected(r, a, gp.matmul(a, L), L, rnd(nb), fp, f)
    return dict(r=r, f=f, lam_m=rnd(N), fp=fp, m=rnd(nb), V=V, K=K, Kinv=Kinv, logdet=logdet)


fmt = lambda t: f"{statistics.median(t):8.3f} ms ({min(t):.3f} .. {max(t):.3f})"
rel = lambda x, y: max(abs(a - b) / abs(b) for a, b in zip(x, y))
print(f"{args.part}: {args.reps} alternated repetitions behind 2 warm-up rounds, median (min .. max)")
for N, nb in zip(shapes[0::2], shapes[1::2]):
    if args.part == "single":
        c = inputs(N, nb, N + nb)

        def terms(on, logdet=None):
            gp.FUSED_LOSS = on
            ll, kl = gp.elbo_terms(c["r"], c["f"], c["lam_m"], c["fp"], c["m"], c["V"], c["K"], c["Kinv"], logdet_K=logdet)
            return float(ll), float(kl)
        runs = {"composite": lambda: terms(False), "fused": lambda: terms(True), "fused, logdet given": lambda: terms(True, c["logdet"])}
        t, out = {k: [] for k in runs}, {}
        for i in range(args.reps + 2):
            for k, fn in runs.items():
                ms, out[k] = timed(fn)
                if i >= 2:
                    t[k].append(ms)
        med = {k: statistics.median(v) for k, v in t.items()}
        print(f"N {N:5d} nb {nb:5d}: " + " | ".join(f"{k} {fmt(v)}" for k, v in t.items()) +
              f" | composite / fused {med['composite'] / med['fused']:5.2f}, with logdet {med['composite'] / med['fused, logdet given']:5.2f}"
              f" | deviation from the composite {rel(out['fused'], out['composite']):.1e}, {rel(out['fused, logdet given'], out['composite']):.1e}",
              flush=True)
        del c
    else:
        engines = gp._group_engines(args.units, nb)
        cs = [inputs(N, nb, 100 * u + N + nb) for u in range(args.units)]
        qs = [gp._loss_prepare(c["r"], c["f"], c["lam_m"], c["fp"], c["m"], c["V"], c["K"], c["Kinv"], engine=e)
              for c, e in zip(cs, engines)]
        runs = {"16 single calls": lambda: [gp._loss_run_single(q) for q in qs], "one group call": lambda: gp._request_run_group(qs)}
        t, out = {k: [] for k in runs}, {}
        for i in range(args.reps + 2):
            for k, fn in runs.items():
                ms, out[k] = timed(fn)
                if i >= 2:
                    t[k].append(ms)
        assert out["16 single calls"] == out["one group call"], "a unit of the group differs from its single call"
        med = {k: statistics.median(v) for k, v in t.items()}
        print(f"N {N:5d} nb {nb:5d}, {args.units} units: " + " | ".join(f"{k} {fmt(v)}" for k, v in t.items()) +
              f" | single / group {med['16 single calls'] / med['one group call']:5.2f} | every unit of the group has the bits of its single call",
              flush=True)
        del cs, qs
