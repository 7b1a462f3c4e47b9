"""The damped E-steps of an EM iteration as one device call against the host loop (profiles/r23_estep_damped_chain.txt):
`python scripts/estep_damped_chain_times.py [--part single|group]`.

single: nEstep damped steps as varGP's host loop drives them -- per step utils._estep_projected_damped, utils.lambda_moments
(the host composition) and utils._fparam_lbfgs, three waits -- against one utils._estep_chain_damped call
(gpfit_estep_chain_damped) on the same inputs at (N, nb) = (3160, 1024), (3160, 2100), (4096, 4096): both warm, alternated
in one process (loop, chain, loop, chain, ...), 7 timed repetitions behind 2 warm-up rounds of both; median and range of
the host clock around calls that end in a device synchronisation.  The chain's request copies (m, V, f and the moments)
are inside its time, as they are in a fit.  The last column: the chain's (m, V) against the loop's.

group: 16 units as one gpfit_estep_chain_damped_batch call (utils._estep_chain_damped_group) against 16 single chain
calls on the same inputs at (3160, 1024), alternated the same way; every unit of the group is compared with its single
call bit for bit.

Inputs as scripts/estep_damped_times.py: K~ = G G^T / nb + I / 10 with G ~ N(0, 1), a ~ N(0, 1) / sqrt(nb),
f = exp(0.35 z - 0.3), r ~ Poisson(f), V = the full step's result at 1.7 times the rate, kv0 ~ U(0.05, 0.15); the factor of
K~, its inverse and a L are formed before the timed region, as varGP forms them once per EM iteration."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gaussian_processes_amd import utils as gp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=("single", "group", "both"), default="both")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--shapes", type=int, nargs="+", default=[3160, 1024, 3160, 2100, 4096, 4096])
ap.add_argument("--group-shape", type=int, nargs=2, default=[3160, 1024])
ap.add_argument("--units", type=int, default=16)
ap.add_argument("--alpha", type=float, default=0.5)
ap.add_argument("--nestep", type=int, default=10)
ap.add_argument("--nfstep", type=int, default=4)
args = ap.parse_args()
dev = torch.device("cuda:0")
LOG_A0 = 0.1


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def rel(x, y):
    return float((x - y).abs().max() / y.abs().max())


def inputs(N, nb, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64, device=dev, generator=gen)
    G = rnd(nb, nb)
    K = gp.matmul(G, G, transB=True) / nb
    K = (K + K.T) / 2 + 0.1 * torch.eye(nb, dtype=torch.float64, device=dev)
    a = rnd(N, nb) / nb ** 0.5
    f = torch.exp(0.35 * rnd(N) - 0.3)
    r = torch.poisson(f, generator=gen)
    m = rnd(nb)
    kv0 = 0.05 + 0.1 * torch.rand(N, dtype=torch.float64, device=dev, generator=gen)
    L, Linv, _, info = gp.cholesky(K, want_inverse=True)
    assert info == 0
    aL = gp.matmul(a, L)
    _, V = gp._estep_projected(r, a, aL, L, m, {"logA": torch.tensor(LOG_A0, dtype=torch.float64)}, 1.7 * f)
    Kb = gp.matmul(a, K)
    return {"r": r, "a": a, "aL": aL, "L": L, "Linv": Linv, "kv0": kv0, "V": V, "m": m, "f": f, "Kb": Kb,
            "Kvec": kv0 + torch.sum(Kb * a, 1)}


def host_loop(c):
    """What varGP does per damped E-step with the switch off."""
    fp = {"logA": torch.tensor(LOG_A0, dtype=torch.float64)}
    m, V, f = c["m"], c["V"], c["f"]
    for i in range(args.nestep):
        m, V = gp._estep_projected_damped(c["r"], c["a"], c["aL"], c["L"], c["Linv"], V, m, fp, f, args.alpha)
        lam_m, lam_var = gp.lambda_moments(None, None, c["a"], c["Kvec"], c["Kb"], None, m, V, None)
        f, _ = gp._fparam_lbfgs(lam_m, lam_var, c["r"], fp, args.nfstep, i)
    return m, V, float(fp["logA"])


def chain(c):
    m, V, _, _, _, rec = gp._estep_chain_damped(c["r"], c["a"], c["aL"], c["L"], c["Linv"], c["kv0"], c["V"], c["m"], c["f"],
                                                LOG_A0, args.alpha, args.nestep, args.nfstep)
    assert all(q[9] == 0 and q[10] == 1 and q[6] == 0 for q in rec), rec
    return m, V, rec[-1][0]


fmt = lambda t: f"{statistics.median(t):9.3f} ms ({min(t):.3f} .. {max(t):.3f})"
print(f"{args.reps} alternated repetitions behind 2 warm-up rounds, median (min .. max); alpha = {args.alpha}, "
      f"{args.nestep} E-steps x {args.nfstep} rate-parameter steps")
if args.part in ("single", "both"):
    for N, nb in zip(args.shapes[0::2], args.shapes[1::2]):
        c = inputs(N, nb, N + nb)
        tl, tc = [], []
        for i in range(args.reps + 2):
            t_loop, out_loop = timed(lambda: host_loop(c))
            t_chain, out_chain = timed(lambda: chain(c))
            if i >= 2:   # two warm-up rounds of both
                tl.append(t_loop)
                tc.append(t_chain)
        assert gp.cholesky(out_chain[1])[3] == 0 and torch.equal(out_chain[1], out_chain[1].T)
        print(f"single N {N:5d} nb {nb:5d}: host loop {fmt(tl)} | one chain {fmt(tc)} | loop / chain "
              f"{statistics.median(tl) / statistics.median(tc):5.2f} | chain against loop: V {rel(out_chain[1], out_loop[1]):.1e} "
              f"m {rel(out_chain[0], out_loop[0]):.1e} logA {abs(out_chain[2] - out_loop[2]):.1e}", flush=True)
        del c, out_loop, out_chain
if args.part in ("group", "both"):
    N, nb = args.group_shape
    cs = [inputs(N, nb, 7 * u + N + nb) for u in range(args.units)]
    units = [{"r": c["r"], "KKtilde_inv": c["a"], "aL": c["aL"], "L": c["L"], "Linv": c["Linv"], "kv0": c["kv0"], "V": c["V"],
              "m": c["m"], "f_mean": c["f"], "logA0": LOG_A0} for c in cs]
    engines = gp._group_engines(args.units, max(N, nb))

    def singles():
        return [gp._request_run_single(gp._chain_damped_prepare(alpha=args.alpha, n_steps=args.nestep,
                                                                n_fparam_steps=args.nfstep, engine=e, **u))
                for u, e in zip(units, engines)]

    def group():
        return gp._estep_chain_damped_group(units, args.alpha, args.nestep, args.nfstep)
    ts, tg = [], []
    for i in range(args.reps + 2):
        t_single, out_single = timed(singles)
        t_group, out_group = timed(group)
        if i >= 2:
            ts.append(t_single)
            tg.append(t_group)
    same = all(torch.equal(x, y) for s, g in zip(out_single, out_group) for x, y in zip(s[:5], g[:5]))
    same = same and all(s[5] == g[5] for s, g in zip(out_single, out_group))
    print(f"group N {N:5d} nb {nb:5d}, {args.units} units: {args.units} single chain calls {fmt(ts)} | one group call {fmt(tg)} | "
          f"single / group {statistics.median(ts) / statistics.median(tg):5.2f} | every unit of the group has the bits of its "
          f"single call: {same}", flush=True)
