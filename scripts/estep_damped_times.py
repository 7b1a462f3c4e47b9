"""The damped E-step against the full one (profiles/r21_estep_damped.txt): `python scripts/estep_damped_times.py`.

utils._estep_projected_damped (gpfit_estep_projected_damped, alpha = 0.5) and utils._estep_projected
(gpfit_estep_projected, no moments) on the same inputs at (N, nb) = (3160, 1024), (3160, 2100), (4096, 4096): both warm,
alternated in one process (full, damped, full, damped, ...), 7 timed repetitions behind 2 warm-up rounds of both; median
and range of the host clock around calls that end in a device synchronisation (the wrappers' two torch.empty of the
outputs are inside).  Inputs: K~ = G G^T / nb + I / 10 with G ~ N(0, 1), a ~ N(0, 1) / sqrt(nb), f = exp(0.7 lam - 0.3),
r ~ Poisson(f), V = the full step's result at 1.7 times the rate; the factor of K~, its inverse and a L are formed before
the timed region, as varGP forms them once per EM iteration.  The last column: the damped call at alpha = 1 against the
full step (max relative difference of V_new, of m_new)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gaussian_processes_amd import utils as gp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--shapes", type=int, nargs="+", default=[3160, 1024, 3160, 2100, 4096, 4096])
ap.add_argument("--alpha", type=float, default=0.5)
args = ap.parse_args()
dev = torch.device("cuda:0")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def rel(x, y):
    return float((x - y).abs().max() / y.abs().max())


print(f"{args.reps} alternated repetitions behind 2 warm-up rounds, median (min .. max); alpha = {args.alpha}")
for N, nb in zip(args.shapes[0::2], args.shapes[1::2]):
    gen = torch.Generator(device=dev).manual_seed(N + nb)
    rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64, device=dev, generator=gen)
    G = rnd(nb, nb)
    K = gp.matmul(G, G, transB=True) / nb
    K = (K + K.T) / 2 + 0.1 * torch.eye(nb, dtype=torch.float64, device=dev)
    a = rnd(N, nb) / nb ** 0.5
    f = torch.exp(0.35 * rnd(N) - 0.3)
    r = torch.poisson(f, generator=gen)
    m = rnd(nb)
    fp = {"logA": torch.tensor(0.1, dtype=torch.float64)}
    L, Linv, _, info = gp.cholesky(K, want_inverse=True)
    assert info == 0
    aL = gp.matmul(a, L)
    _, V = gp._estep_projected(r, a, aL, L, m, fp, 1.7 * f)
    del G
    full = lambda: gp._estep_projected(r, a, aL, L, m, fp, f)
    damped = lambda: gp._estep_projected_damped(r, a, aL, L, Linv, V, m, fp, f, args.alpha)
    tf, td = [], []
    for i in range(args.reps + 2):
        t_full, out_full = timed(full)
        t_damped, out_damped = timed(damped)
        if i >= 2:   # two warm-up rounds of both
            tf.append(t_full)
            td.append(t_damped)
    assert gp.cholesky(out_damped[1])[3] == 0 and torch.equal(out_damped[1], out_damped[1].T)
    one = gp._estep_projected_damped(r, a, aL, L, Linv, V, m, fp, f, 1.0)
    fmt = lambda t: f"{statistics.median(t):9.3f} ms ({min(t):.3f} .. {max(t):.3f})"
    print(f"N {N:5d} nb {nb:5d}: full {fmt(tf)} | damped {fmt(td)} | damped / full "
          f"{statistics.median(td) / statistics.median(tf):5.2f} | alpha = 1 against full: V {rel(one[1], out_full[1]):.1e} "
          f"m {rel(one[0], out_full[0]):.1e}", flush=True)
    del K, a, L, Linv, aL, V, out_full, out_damped, one
