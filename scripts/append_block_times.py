"""Growing a fitted model by k images: one block step against k rank-1 steps (profiles/r18_append_block.txt):
`python scripts/append_block_times.py [--eigval-tol T]`.

Two levels, each at n = 512, 2048, 4096 and k = 8, 32, 128 on the arc-cosine kernel matrix of synthetic 16 x 16 stimuli:
  factor   utils.cholesky_append_block once  |  utils.cholesky_append k times, on factors already embedded in
           (n + k)-sized tensors (no copies in the timed region: the rank-1 loop at its best)
  prepare  utils.extend_inducing_set with k images once  |  with one image k times, each call starting from the model
           the previous one prepared (no refit between them: the preparation alone)
Warm, alternated in one process: every repetition runs the block form and then the loop form; median and range of the
host clock around work that ends in a device synchronisation.  The model is a stand-in with the keys
extend_inducing_set reads (identity basis, the factor of K~ kept), not a fit: the preparation does not depend on how
(m, V) came about.  The route column says whether the all-kept proof held on the grown factor (identity) or the
general basis search ran behind the append.  Where the bounds of that proof do not hold at utils.EIGVAL_TOL for the
largest grown matrix of a size, the tolerance is lowered for that size (a quarter of what the bounds would accept, or
--eigval-tol) and the line of the size says so: the point is the cost of the append route, which is only taken while
the proof holds."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gaussian_processes_amd import synthetic as syn, utils as gp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--eigval-tol", type=float, default=None)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--sizes", type=int, nargs="+", default=[512, 2048, 4096])
ap.add_argument("--blocks", type=int, nargs="+", default=[8, 32, 128])
args = ap.parse_args()
DEFAULT_TOL = gp.EIGVAL_TOL
dev = torch.device("cuda:0")
lower, upper = syn.limits()
PX = 16
theta = {k: torch.tensor(float(v), dtype=torch.float64) for k, v in syn.theta0().items()}
C, mask = gp.localker(theta, upper, lower, PX)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(block, loop, reps):
    tb, tl = [], []
    for i in range(reps + 2):
        b, ob = timed(block)
        l, ol = timed(loop)
        if i >= 2:   # two warm-up rounds of both
            tb.append(b)
            tl.append(l)
    fmt = lambda t: f"{statistics.median(t):9.3f} ms ({min(t):.3f} .. {max(t):.3f})"
    return fmt(tb), fmt(tl), statistics.median(tl) / statistics.median(tb), ob, ol


def as_model(prev, grown):
    ik = grown["init_kernel"]
    return dict(prev, xtilde=grown["xtilde"], m_b=grown["m"], V_b=grown["V"], B=ik["B"], basis_route=ik["basis_route"],
                final_kernel={"K_tilde": ik["K_tilde"], "Kvec": ik["Kvec"], "chol": ik["chol"]})


print(f"{args.reps} alternated repetitions behind 2 warm-up rounds, median (min .. max)", flush=True)
for n in args.sizes:
    kmax = max(args.blocks)
    X = torch.from_numpy(syn.stimuli(n + kmax, PX * PX)).to(dev)
    Xm = X[:, mask].contiguous()
    K = gp.acosker(theta, Xm, Xm, C=C)
    K = ((K + K.T) * 0.5).contiguous()
    Kvec = gp.acosker(theta, Xm, x2=None, C=C, diag=True).reshape(-1)
    L0, Li0, _, info = gp.cholesky(K[:n, :n].contiguous(), want_inverse=True)
    assert info == 0
    _, Lif, _, info = gp.cholesky(K, want_inverse=True)
    assert info == 0
    lam_max_ub = min(float(torch.diagonal(K).sum()), float(K.abs().sum(1).max()))
    lam_min_lb = 1.0 / (float(Lif.abs().sum(0).max()) * float(Lif.abs().sum(1).max()))
    accept = min(lam_min_lb / lam_max_ub, lam_min_lb)
    gp.EIGVAL_TOL = DEFAULT_TOL if accept > 4 * DEFAULT_TOL else (args.eigval_tol if args.eigval_tol is not None else accept / 4)
    print(f"n {n}: at {n + kmax} images lambda_min >= {lam_min_lb:.3e}, lambda_max <= {lam_max_ub:.3e}; EIGVAL_TOL {gp.EIGVAL_TOL:.3g}"
          f"{'' if gp.EIGVAL_TOL == DEFAULT_TOL else f' (default {DEFAULT_TOL:g} would not prove full rank)'}", flush=True)
    del Lif
    g = torch.Generator().manual_seed(1)
    m0 = torch.randn(n, dtype=torch.float64, generator=g).to(dev)
    V0 = torch.eye(n, dtype=torch.float64, device=dev)
    model = {"xtilde": X[:n].contiguous(), "hyperparams_tuple": (theta, lower, upper), "C": C, "mask": mask,
             "B": gp._mark_identity(torch.eye(n, dtype=torch.float64, device=dev)), "basis_route": "identity", "m_b": m0, "V_b": V0,
             "final_kernel": {"K_tilde": K[:n, :n].contiguous(), "Kvec": Kvec[:n].contiguous(), "chol": {"L": L0, "Linv": Li0}}}
    for k in args.blocks:
        N = n + k
        Lb = torch.zeros((N, N), dtype=torch.float64, device=dev); Lib = torch.zeros_like(Lb)
        Lb[:n, :n], Lib[:n, :n] = L0, Li0
        Ll, Lil = Lb.clone(), Lib.clone()
        cols = K[:N, n:N].contiguous()
        col = [K[:n + j + 1, n + j].contiguous() for j in range(k)]

        def f_block():
            return gp.cholesky_append_block(Lb, Lib, cols)

        def f_loop():
            for j in range(k):
                nn = n + j + 1
                out = gp.cholesky_append(Ll[:nn, :nn], Lil[:nn, :nn], col[j])
            return out

        tb, tl, ratio, ob, ol = alternate(f_block, f_loop, args.reps)
        assert ob[1] == 0 and ol[1] == 0
        dL = float((Lb - Ll).abs().max() / Ll.abs().max())
        dLi = float((Lib - Lil).abs().max() / Lil.abs().max())
        print(f"factor  n {n:5d} k {k:4d}: block {tb} | {k} x rank-1 {tl} | loop / block {ratio:6.2f} | "
              f"max |dL| {dL:.1e} |dLinv| {dLi:.1e}", flush=True)

        def p_block():
            return gp.extend_inducing_set(model, X[n:N])

        def p_loop():
            cur = model
            for j in range(k):
                grown = gp.extend_inducing_set(cur, X[n + j])
                cur = as_model(cur, grown)
            return grown

        reps = args.reps if n * k < 4096 * 128 else max(3, args.reps // 2)
        tb, tl, ratio, ob, ol = alternate(p_block, p_loop, reps)
        kb, kl = ob["init_kernel"], ol["init_kernel"]
        dKi = float((kb["K_tilde_inv_b"] - kl["K_tilde_inv_b"]).abs().max() / kl["K_tilde_inv_b"].abs().max()) \
            if kb["K_tilde_inv_b"].shape == kl["K_tilde_inv_b"].shape else float("nan")
        print(f"prepare n {n:5d} k {k:4d}: block {tb} | {k} x one image {tl} | loop / block {ratio:6.2f} | "
              f"route {kb['basis_route']} / {kl['basis_route']}, max |dK~^-1| {dKi:.1e}", flush=True)
