"""One basis rebuild (eigtop.top_eigenpairs, basis="subspace") with the sweeps of a pass as one device call
(utils._basis_sweeps) and as the host loop, alternated in one process: cold, and warm from the state of a nearby kernel
matrix, at the lab's inducing-set size and at N = 2048 / 4096 / 8192; then three units at (2048, 1024) as one
utils._basis_sweeps_group call against three single calls.

    python scripts/sweep_chain_times.py [--sizes 2100,2048,4096,8192] [--reps 7] [--no-group]

Every figure is a synchronised wall time in ms; the first repetition of each setting is listed apart (warm-up)."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gaussian_processes_amd import utils as gp, synthetic as syn, eigtop

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="2100,2048,4096,8192")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--no-group", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
lower, upper = syn.limits()


def kt(X, scale):
    th = {k: torch.tensor(float(v), dtype=torch.float64) for k, v in syn.theta0().items()}
    th["sigma_0"] = th["sigma_0"] * scale
    th["-2log2beta"] = th["-2log2beta"] + (scale - 1.0)
    C, mask = gp.localker(th, upper, lower, 16)
    Xm = X[:, mask].contiguous()
    return gp.acosker(th, Xm, Xm, C=C)


def rebuild(K, chain, start=None):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = eigtop.top_eigenpairs(K, 1e-4, gp.matmul, gp.cholesky, basis="subspace", gemm_into=gp.gemm_into, start=start,
                                sweep_chain=gp._basis_sweeps if chain else None)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(ts):
    steady = sorted(ts[1:])
    return f"first {ts[0]:7.2f}  steady min {steady[0]:7.2f} median {steady[len(steady) // 2]:7.2f} max {steady[-1]:7.2f}  (n {len(steady)})"


for N in (int(v) for v in args.sizes.split(",")):
    X = torch.from_numpy(syn.stimuli(N, 256)).to(dev)
    K0, K1 = kt(X, 1.0), kt(X, 1.002)
    gp.reserve(N, 1)
    _, base = rebuild(K0, False)
    if base is None or base[0] is not None:
        print(f"N {N}: the subspace route declined"); continue
    state = base[2]["state"]
    times = {(mode, chain): [] for mode in ("cold", "warm") for chain in (True, False)}
    outs = {}
    for rep in range(args.reps):
        for chain in (True, False):                  # alternated: chain, loop, chain, loop, ...
            for mode in ("cold", "warm"):
                ms, out = rebuild(K1, chain, state if mode == "warm" else None)
                times[mode, chain].append(ms)
                outs[mode, chain] = out
    for mode in ("cold", "warm"):
        a, b = outs[mode, True], outs[mode, False]
        same = torch.equal(a[1], b[1]) and torch.equal(a[2]["K_tilde_b"], b[2]["K_tilde_b"])
        print(f"N {N} {mode}: k {a[2]['k']} kept {a[2]['n']} sweeps {a[2]['sweeps']} products {a[2]['products']} "
              f"bit-equal on/off {same}")
        print(f"    chain  {fmt(times[mode, True])}")
        print(f"    loop   {fmt(times[mode, False])}")

if not args.no_group:
    N, k, m = 2048, 1024, 6
    units = []
    for seed in range(3):
        X = torch.from_numpy(syn.stimuli(N, 256, seed=seed)).to(dev)
        K = kt(X, 1.0)
        Q0 = eigtop._cholqr(eigtop._hash_matrix(N, k, K.device, K.dtype), gp.matmul, gp.cholesky, 2)
        a = float((Q0 * gp.matmul(K, Q0)).sum(0).min())
        units.append({"K": K, "Q": Q0, "shifts": [0.0] + eigtop._chebyshev_shifts(0.5 * a, m - 1)})
    tg, ts = [], []
    for rep in range(args.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        group = gp._basis_sweeps_group(units)
        torch.cuda.synchronize(); tg.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        alone = [gp._basis_sweeps(u["K"], u["Q"], None, u["shifts"], True) for u in units]
        torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    same = all(torch.equal(x, y) for g, s in zip(group, alone) for x, y in zip(g, s))
    print(f"three units at ({N}, {k}), {m} sweeps + tail: bit-equal group/single {same}")
    print(f"    one group call      {fmt(tg)}")
    print(f"    three single calls  {fmt(ts)}")
