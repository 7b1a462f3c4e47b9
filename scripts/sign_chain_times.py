"""One basis rebuild with the projector step (eigtop._kept_subspace) as device calls (utils._sign_steps) and as the host
loop, alternated in one process: the sweeps route (eigtop.top_eigenpairs, basis="subspace", sweeps chained either way)
cold and warm at the lab's inducing-set size and at N = 2048 / 4096 / 8192, the dense route (eigtop.kept_eigenspace_dense)
at N = 1024 / 1536; with the share of a rebuild spent in _kept_subspace.  Then 3 and 16 units at k = 1024 (head + 11
steps + tail) as one utils._sign_steps_group call against as many single calls.

    python scripts/sign_chain_times.py [--sizes 2100,2048,4096,8192] [--dense 1024,1536] [--reps 7] [--groups 3,16]

Every figure is a synchronised wall time in ms; the first repetition of each setting is listed apart (warm-up)."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gaussian_processes_amd import utils as gp, synthetic as syn, eigtop

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="2100,2048,4096,8192")
ap.add_argument("--dense", default="1024,1536")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--groups", default="3,16")
args = ap.parse_args()
dev = torch.device("cuda:0")
lower, upper = syn.limits()
ints = lambda s: [int(v) for v in s.split(",") if v]


def kt(X, scale):
    th = {k: torch.tensor(float(v), dtype=torch.float64) for k, v in syn.theta0().items()}
    th["sigma_0"] = th["sigma_0"] * scale
    th["-2log2beta"] = th["-2log2beta"] + (scale - 1.0)
    C, mask = gp.localker(th, upper, lower, 16)
    Xm = X[:, mask].contiguous()
    return gp.acosker(th, Xm, Xm, C=C)


# the time spent inside _kept_subspace, synchronised at both ends (the share of a rebuild the projector step takes)
inside = [0.0]
kept_subspace = eigtop._kept_subspace


def timed_kept_subspace(*a, **k):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = kept_subspace(*a, **k)
    torch.cuda.synchronize(); inside[0] += (time.perf_counter() - t0) * 1e3
    return out


eigtop._kept_subspace = timed_kept_subspace


def rebuild(K, chain, start=None, dense=False):
    hook = gp._sign_steps if chain else None
    inside[0] = 0.0
    torch.cuda.synchronize(); t0 = time.perf_counter()
    if dense:
        out = eigtop.kept_eigenspace_dense(K, 1e-4, gp.matmul, gp.cholesky, gemm_into=gp.gemm_into, sign_chain=hook)
    else:
        out = eigtop.top_eigenpairs(K, 1e-4, gp.matmul, gp.cholesky, basis="subspace", gemm_into=gp.gemm_into, start=start,
                                    sweep_chain=gp._basis_sweeps, sign_chain=hook)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, inside[0], out


def fmt(ts):
    steady = sorted(ts[1:])
    return f"first {ts[0]:7.2f}  steady min {steady[0]:7.2f} median {steady[len(steady) // 2]:7.2f} max {steady[-1]:7.2f}  (n {len(steady)})"


def med(ts):
    return sorted(ts[1:])[len(ts[1:]) // 2]


for N, dense in [(n, False) for n in ints(args.sizes)] + [(n, True) for n in ints(args.dense)]:
    X = torch.from_numpy(syn.stimuli(N, 256)).to(dev)
    K0, K1 = kt(X, 1.0), kt(X, 1.002)
    gp.reserve(N, 1)
    _, _, base = rebuild(K0, False, dense=dense)
    if base is None or base[1] is None:
        print(f"N {N}: the subspace route declined"); continue
    modes = ("cold",) if dense else ("cold", "warm")
    state = None if dense else base[2]["state"]
    times = {(mode, chain): [] for mode in modes for chain in (True, False)}
    part = {(mode, chain): [] for mode in modes for chain in (True, False)}
    outs = {}
    for rep in range(args.reps):
        for chain in (True, False):                  # alternated: chain, loop, chain, loop, ...
            for mode in modes:
                ms, ins, out = rebuild(K1, chain, state if mode == "warm" else None, dense=dense)
                times[mode, chain].append(ms)
                part[mode, chain].append(ins)
                outs[mode, chain] = out
    for mode in modes:
        a, b = outs[mode, True], outs[mode, False]
        same = torch.equal(a[1], b[1]) and torch.equal(a[2]["K_tilde_b"], b[2]["K_tilde_b"])
        print(f"N {N} {'dense' if dense else mode}: k {a[2]['k']} kept {a[2]['n']} sweeps {a[2]['sweeps']} sign iterations "
              f"{a[2]['sign_iterations']} bit-equal on/off {same}")
        for chain, name in ((True, "chain"), (False, "loop ")):
            print(f"    {name}  {fmt(times[mode, chain])}")
            print(f"           in _kept_subspace: median {med(part[mode, chain]):7.2f} = "
                  f"{100.0 * med(part[mode, chain]) / med(times[mode, chain]):4.1f} % of the rebuild")

k = 1024
cs = eigtop._sign_schedule(eigtop._SIGN_L0, 0, 40)[0]
for n_units in ints(args.groups):
    units = []
    for seed in range(n_units):
        g = torch.Generator().manual_seed(seed)
        Z, _ = torch.linalg.qr(torch.randn(k, k, dtype=torch.float64, generator=g))
        lam = torch.cat([torch.logspace(2, 0, k // 2, dtype=torch.float64), torch.logspace(-4, -6, k - k // 2, dtype=torch.float64)])
        S = (Z * lam) @ Z.T
        units.append({"S": ((S + S.T) * 0.5).to(dev).contiguous(), "tau": 1e-2 * (1.0 + 0.01 * seed), "cs": cs})
    tg, ts = [], []
    for rep in range(args.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        group = gp._sign_steps_group(units)
        torch.cuda.synchronize(); tg.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        alone = [gp._sign_steps(u["S"], u["tau"], None, None, cs, 0) for u in units]
        torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    same = all(torch.equal(x, y) for g, s in zip(group, alone) for x, y in zip(g, s))
    print(f"{n_units} units at k = {k}, head + {len(cs)} steps + tail: bit-equal group/single {same}")
    print(f"    one group call         {fmt(tg)}")
    print(f"    {n_units:2d} single calls        {fmt(ts)}")
