"""Dump the GEMM launch log and the result bits of every host path that issues GEMM launches.  Needs the GPU.

    python scripts/launch_log_dump.py OUT.txt [--root TREE]

For each case below a fresh child process (the log switch GPFIT_GEMM_LOG is read once per process) runs one entry
point on small inputs from gaussian_processes_amd.synthetic and the parent writes, per case: the `[gpfit gemm]` lines
the child printed, then float.hex() of every scalar and the SHA-256 of every array it returned.  Run it on the builds
of two commits (--root: the tree whose package and built library are imported; default: this repository) and compare
the files, or the digest printed at the end, to show that a change of the host code launches the same products in
the same order and computes the same bits.  Children run one after another, each under its own time limit; the
parent stops at the first child that does not exit 0.  GPFIT_* is removed from the environment first."""
import argparse
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 300

# name -> (value of GPFIT_GEMM_LOG, further environment).  The log counts evaluations of the fit_eval family
# (gpfit_fit_eval*, _projected, _sparse: the first is 1); groups, the pull-backs, the E-steps and gpfit_potrf do not
# count, so called first in their process they are evaluation 0.
CASES = {
    "fit_eval f64 N=256": (1, {}),
    "fit_eval f64 N=640": (1, {}),
    "fit_eval f64 N=1408": (1, {}),
    "fit_eval f64 N=2100": (1, {}),
    "fit_eval f64 N=640 no gradients": (1, {}),
    "fit_eval f64 N=1408 second call reuse_V": (2, {}),
    "fit_eval f32 N=640": (1, {}),
    "fit_eval mixed N=2100": (1, {}),
    "group of 3 N=640": (0, {}),
    "group of 3 N=2100": (0, {}),
    "group of 16 N=256": (0, {}),
    "fit_eval f64 N=640 TS_MIN=256": (1, {"GPFIT_TS_MIN": "256"}),
    "group of 3 N=640 TS_MIN=256": (0, {"GPFIT_TS_MIN": "256"}),
    "fit_eval f64 N=640 NO_PAIR": (1, {"GPFIT_NO_PAIR": "1"}),
    "fit_eval f64 N=640 NO_BATCH": (1, {"GPFIT_NO_BATCH": "1"}),
    "grad_pullback N=640": (0, {}),
    "fit_eval_projected N=1024 kept=200": (1, {}),
    "fit_eval_sparse nt=640 ntilde=384 kept=200": (1, {}),
    "estep N=640": (0, {}),
    "estep N=2100": (0, {}),
    "estep_projected 640x256": (0, {}),
    "potrf N=640": (0, {}),
    "potrf N=640 with inverse": (0, {}),
    "acosker_pullback 640x384": (0, {}),
}


def child(name, root):
    sys.path.insert(0, root)
    import ctypes
    import numpy as np
    import torch
    from gaussian_processes_amd import _lib, synthetic as syn
    from gaussian_processes_amd.engine import GPFitEngine, fit_eval_group
    from oracle import gp_oracle as orc

    dev = torch.device("cuda:0")
    KEYS = syn.THETA_KEYS
    LOWER, UPPER = syn.limits()
    LOGA, LAM0 = syn.F_PARAMS["logA"], syn.F_PARAMS["lambda0"]
    d = 64
    grid = syn.grid_for(d)
    rows, cols = (grid, grid) if not isinstance(grid, (tuple, list)) else grid
    lib = _lib.load()

    def T(a):
        return torch.from_numpy(np.asarray(a, dtype=np.float64))

    def cell(N, c):
        """r, m, V, theta of cell c, the stimuli and their masked copy at theta0, as the GPU tests build them"""
        X = T(syn.stimuli(N, d))
        r, m = syn.cell_inputs(N, c)
        th0 = syn.theta0(c)
        C0, mask0 = orc.spatial_metric(th0, LOWER, UPPER, grid)
        Xm = X[:, mask0].contiguous()
        V = 0.5 * orc.arccos_gram(th0, Xm, Xm, C0)
        return X.to(dev), T(r).to(dev), T(m).to(dev), V.to(dev), syn.theta_eval(c), Xm.to(dev), C0.to(dev), th0

    def noise(seed, *shape):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)

    def spd(seed, n, scale):
        G = noise(seed, n, n)
        return torch.eye(n, dtype=torch.float64) + scale * (G @ G.T) / n

    def emit(label, v):
        if isinstance(v, torch.Tensor):
            torch.cuda.synchronize()
            print(f"RESULT {label} sha256 {hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest()}")
        else:
            print(f"RESULT {label} {float(v).hex()}")

    def emit_fit(tag, out):
        for k in ("loss", "loglik", "KL", "logdet_K", "logdet_V", "tr_KinvV", "mKinvm", "d"):
            emit(f"{tag}{k}", out[k])
        for k in KEYS:
            emit(f"{tag}grad[{k}]", out["grad"][k])
        for k in ("lam_m", "lam_var", "f"):
            if out.get(k) is not None:
                emit(f"{tag}{k}", out[k])

    def theta_arr(th):
        return _lib.darr([float(th[k]) for k in KEYS])

    def closure_inputs(n_ind, nk):
        B = torch.linalg.qr(noise(11, n_ind, nk))[0].contiguous().to(dev)
        return B, (0.1 * noise(12, nk)).to(dev), spd(13, nk, 0.05).to(dev)

    words = name.split()
    N = int(name.split("N=")[1].split()[0]) if "N=" in name else 0
    if name.startswith("fit_eval f") or name.startswith("fit_eval mixed"):
        X, r, m, V, th, *_ = cell(N, 0)
        if words[1] == "f32":
            X, r, m, V = (t.float() for t in (X, r, m, V))
        kw = {"grad_precision": "f32"} if words[1] == "mixed" else {}
        eng = GPFitEngine(N, d)
        out = eng.fit_eval(th, LOWER, UPPER, grid, X, r, m, V, LOGA, LAM0, want_grad="no gradients" not in name, **kw)
        if "reuse_V" in name:
            out = eng.fit_eval(th, LOWER, UPPER, grid, X, r, m, V, LOGA, LAM0, reuse_V=True)
        emit_fit("", out)
    elif name.startswith("group of"):
        units = int(words[2])
        cs = [cell(N, c) for c in range(units)]
        engs = [GPFitEngine(N, d) for _ in range(units)]
        outs = fit_eval_group(engs, [c[4] for c in cs], LOWER, UPPER, grid, cs[0][0], [c[1] for c in cs], [c[2] for c in cs],
                              [c[3] for c in cs], LOGA, LAM0)
        for u, out in enumerate(outs):
            emit_fit(f"unit{u} ", out)
    elif name.startswith("grad_pullback"):
        X, _, _, _, th, *_ = cell(N, 0)
        W = noise(N + d, N, N)
        W = ((W + W.T) / (2 * N)).to(dev)
        gvec = noise(N, N).to(dev)
        eng = GPFitEngine(N, d)
        out6 = (ctypes.c_double * 6)()
        _lib.check(lib.gpfit_grad_pullback(eng._ctx, eng._stream(), theta_arr(th), int(rows), int(cols), X.data_ptr(), X.stride(0), N,
                                           W.data_ptr(), W.stride(0), gvec.data_ptr(), out6), "gpfit_grad_pullback")
        for i, k in enumerate(KEYS):
            emit(f"out6[{k}]", out6[i])
    elif name.startswith("fit_eval_projected") or name.startswith("fit_eval_sparse"):
        sparse = name.startswith("fit_eval_sparse")
        n_t, n_ind, nk = (640, 384, 200) if sparse else (1024, 1024, 200)
        X, r, _, _, th, *_ = cell(n_t, 0)
        Xt = X[:n_ind].contiguous()
        B, m_b, V_b = closure_inputs(n_ind, nk)
        eng = GPFitEngine(n_t, d)
        out = (ctypes.c_double * 16)()
        head = (eng._ctx, eng._stream(), theta_arr(th), theta_arr(LOWER), theta_arr(UPPER), int(rows), int(cols), X.data_ptr(), X.stride(0),
                n_t)
        tail = (r.data_ptr(), B.data_ptr(), B.stride(0), nk, m_b.data_ptr(), V_b.data_ptr(), V_b.stride(0), float(LOGA), float(LAM0), out)
        if sparse:
            _lib.check(lib.gpfit_fit_eval_sparse(*head, Xt.data_ptr(), Xt.stride(0), n_ind, *tail), "gpfit_fit_eval_sparse")
        else:
            _lib.check(lib.gpfit_fit_eval_projected(*head, *tail), "gpfit_fit_eval_projected")
        for i in range(16):
            emit(f"out[{i}]", out[i])
    elif name.startswith("estep N="):
        _, r, m, V, _, Xm, C0, th0 = cell(N, 0)
        K = orc.arccos_gram(th0, Xm.cpu(), Xm.cpu(), C0.cpu()).to(dev).contiguous()
        f = torch.exp(0.1 * noise(21, N)).to(dev)
        m_new, V_new = torch.empty(N, dtype=torch.float64, device=dev), torch.empty((N, N), dtype=torch.float64, device=dev)
        eng = GPFitEngine(N, d)
        _lib.check(lib.gpfit_estep(eng._ctx, eng._stream(), K.data_ptr(), K.stride(0), N, r.data_ptr(), m.data_ptr(), f.data_ptr(),
                                   float(LOGA), m_new.data_ptr(), V_new.data_ptr(), V_new.stride(0)), "gpfit_estep")
        emit("m_new", m_new)
        emit("V_new", V_new)
    elif name.startswith("estep_projected"):
        n, nb = 640, 256
        r = T(syn.cell_inputs(n, 0)[0]).to(dev)
        a = (noise(31, n, nb) / nb ** 0.5).to(dev)
        L = torch.linalg.cholesky(spd(32, nb, 0.5)).contiguous().to(dev)
        aL = (a @ L).contiguous()
        m_b, f = (0.1 * noise(33, nb)).to(dev), torch.exp(0.1 * noise(34, n)).to(dev)
        m_new, V_new = torch.empty(nb, dtype=torch.float64, device=dev), torch.empty((nb, nb), dtype=torch.float64, device=dev)
        eng = GPFitEngine(n, d)
        _lib.check(lib.gpfit_estep_projected(eng._ctx, eng._stream(), a.data_ptr(), a.stride(0), aL.data_ptr(), aL.stride(0), L.data_ptr(),
                                             L.stride(0), n, nb, r.data_ptr(), m_b.data_ptr(), f.data_ptr(), float(LOGA), m_new.data_ptr(),
                                             V_new.data_ptr(), V_new.stride(0), None, None, None), "gpfit_estep_projected")
        emit("m_new", m_new)
        emit("V_new", V_new)
    elif name.startswith("potrf"):
        V = cell(N, 0)[3]
        inv = "inverse" in name
        L = torch.zeros((N, N), dtype=torch.float64, device=dev)
        Li = torch.zeros((N, N), dtype=torch.float64, device=dev) if inv else None
        logdet, info = ctypes.c_double(), ctypes.c_int()
        eng = GPFitEngine(N, d)
        _lib.check(lib.gpfit_potrf(eng._ctx, eng._stream(), V.data_ptr(), V.stride(0), N, L.data_ptr(), L.stride(0),
                                   Li.data_ptr() if inv else None, Li.stride(0) if inv else 0, ctypes.byref(logdet), ctypes.byref(info)),
                   "gpfit_potrf")
        emit("logdet", logdet.value)
        emit("info", info.value)
        emit("L", L)
        if inv:
            emit("Linv", Li)
    elif name.startswith("acosker_pullback"):
        n1, n2 = 640, 384
        _, _, _, _, _, Xm, C0, th0 = cell(n1, 0)
        x2 = Xm[:n2].contiguous()
        dm = Xm.shape[1]
        W = (noise(41, n1, n2) / n1).to(dev)
        t1 = noise(42, n1).to(dev)
        M = torch.zeros((dm, dm), dtype=torch.float64, device=dev)
        out3 = (ctypes.c_double * 3)()
        eng = GPFitEngine(n1, d)
        _lib.check(lib.gpfit_acosker_pullback(eng._ctx, eng._stream(), float(th0["sigma_0"]), Xm.data_ptr(), Xm.stride(0), n1, x2.data_ptr(),
                                              x2.stride(0), n2, dm, C0.data_ptr(), C0.stride(0), W.data_ptr(), W.stride(0), t1.data_ptr(),
                                              M.data_ptr(), M.stride(0), out3), "gpfit_acosker_pullback")
        emit("M", M)
        for i in range(3):
            emit(f"out3[{i}]", out3[i])
    else:
        raise SystemExit(f"unknown case {name!r}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--root", default=os.path.join(HERE, ".."), help="tree whose package and built library are used")
    ap.add_argument("--case", help="(internal) run this case in this process")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    if args.case:
        return child(args.case, root)
    env0 = {k: v for k, v in os.environ.items() if not k.startswith("GPFIT_")}
    out = open(args.out, "w") if args.out else None
    digest, lines = hashlib.sha256(), 0
    for name, (log, extra) in CASES.items():
        env = dict(env0, GPFIT_GEMM_LOG=str(log), **extra)
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--case", name], env=env, capture_output=True,
                             text=True, timeout=CHILD_TIMEOUT)
        if res.returncode != 0:
            sys.stderr.write(res.stderr[-4000:])
            raise SystemExit(f"case {name!r}: exit status {res.returncode}; stopping")
        body = [ln for ln in res.stderr.splitlines() if ln.startswith("[gpfit gemm]")] + \
               [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
        logged = sum(ln.startswith("[gpfit gemm]") for ln in body)
        print(f"{name}: {logged} launches logged, {len(body) - logged} results", flush=True)
        for ln in [f"== {name} (GPFIT_GEMM_LOG={log}" + "".join(f" {k}={v}" for k, v in extra.items()) + ")"] + body:
            digest.update((ln + "\n").encode())
            lines += 1
            if out:
                out.write(ln + "\n")
    print(f"cases {len(CASES)} lines {lines}")
    print(f"sha256 {digest.hexdigest()}")


if __name__ == "__main__":
    main()
