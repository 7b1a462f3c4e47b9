"""What the lambda_max certificate of the block route (eigtop._kept_subspace: one k x k Cholesky factorisation per basis
rebuild) costs: utils._stabilised_basis cold and warm on the fit's own kernel matrix at N = 2048 / 4096 with this tree's
eigtop.py and with another version of that file (the parent commit's), alternated in one process.

    python scripts/basis_certificate_times.py --other path/to/other/eigtop.py [--sizes 2048,4096] [--reps 9]

Every figure is a synchronised wall time in ms; the first repetition of each setting is listed apart (warm-up)."""
import argparse, importlib.util, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gaussian_processes_amd import utils as gp, synthetic as syn, eigtop

ap = argparse.ArgumentParser()
ap.add_argument("--other", required=True)
ap.add_argument("--sizes", default="2048,4096")
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()
spec = importlib.util.spec_from_file_location("eigtop_other", args.other)
other = importlib.util.module_from_spec(spec)
spec.loader.exec_module(other)
dev = torch.device("cuda:0")
lower, upper = syn.limits()


def kt(X, scale):
    th = {k: torch.tensor(float(v), dtype=torch.float64) for k, v in syn.theta0().items()}
    th["sigma_0"] = th["sigma_0"] * scale
    th["-2log2beta"] = th["-2log2beta"] + (scale - 1.0)
    C, mask = gp.localker(th, upper, lower, 16)
    Xm = X[:, mask].contiguous()
    return gp.acosker(th, Xm, Xm, C=C)


def rebuild(module, K, start=None):
    gp.eigtop = module
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = gp._stabilised_basis(K, start=start)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out, gp._BASIS.route, gp._BASIS.state


def fmt(ts):
    steady = sorted(ts[1:])
    return f"first {ts[0]:7.2f}  steady min {steady[0]:7.2f} median {steady[len(steady) // 2]:7.2f} max {steady[-1]:7.2f}  (n {len(steady)})"


for N in [int(v) for v in args.sizes.split(",") if v]:
    X = torch.from_numpy(syn.stimuli(N, 256)).to(dev)
    K0, K1 = kt(X, 1.0), kt(X, 1.002)
    gp.reserve(N, 1)
    _, _, route, state = rebuild(eigtop, K0)
    print(f"N {N}: route {route}")
    times = {(mode, name): [] for mode in ("cold", "warm") for name in ("this", "other")}
    outs = {}
    for rep in range(args.reps):
        for name, module in (("this", eigtop), ("other", other)):          # alternated: this, other, this, other, ...
            for mode in ("cold", "warm"):
                ms, out, route, _ = rebuild(module, K1, state if mode == "warm" else None)
                times[mode, name].append(ms)
                outs[mode, name] = (out, route)
    for mode in ("cold", "warm"):
        (a, ra), (b, rb) = outs[mode, "this"], outs[mode, "other"]
        same = a[1].shape == b[1].shape and torch.equal(a[1], b[1])
        diff = float((a[1] - b[1]).abs().max()) if a[1].shape == b[1].shape else float("nan")
        print(f"N {N} {mode}: routes {ra} / {rb} kept {a[1].shape[1]} / {b[1].shape[1]} B bit-equal {same} max |dB| {diff:.1e}")
        for name in ("this", "other"):
            print(f"    {name:5s}  {fmt(times[mode, name])}")
gp.eigtop = eigtop
