"""The registry of probes behind tests/test_gpu_context_state.py: one call of every entry point of
include/gpfit_mi355x.h that takes a context (or a table of contexts), on a context the test supplies.

A fit keeps one ``gpfit_ctx`` for its whole run: closures, E-step chains, the tracked loss, basis sweeps, sign steps,
pool scoring and block appends follow one another on it, at changing sizes and precisions, and each finds the work
buffers holding what another call left.  The tests of the kernels and of the entry points make one kind of call on a
fresh context, whose N x N buffers ``gpfit_ctx_create`` zero-fills.  The probes here are what test_gpu_context_state.py
runs behind a poisoned workspace, between two evaluations that share V's cached factor, and beside a pending
evaluation.

A probe is ``Probe(name, entry, cache, units, build)``.  ``build(engines)`` marshals one call on ``engines`` (one per
unit; a single probe has one) and returns a ``Call``: ``run()`` makes the call and returns its return code -- nothing is
checked and nothing raises -- and ``outs`` names everything the call writes, each pre-filled with ``SENTINEL`` (or, for
state the call updates in place, holding its input): device tensors as they are, host arrays of doubles (compared as
``float.hex()``) and of ints.  The entry point is reached through the request layer of ``utils.py`` (``*_prepare`` with
``engine=``, ``_chain_call``, the ``*_batch_raw`` marshals) where that layer lets the caller own the outputs, and through
ctypes with the wrapper's own argument list where the wrapper allocates them; either way the context is the one of the
engine given, which every builder asserts.  ``cache``: what the call does to the cached factor of V (``lv_valid``,
``lv32_valid``, ``lv_n``, ``lv_bytes``: LVbuf, Vbuf, scal[S_LOGDET_V]) as the source reads -- ``KEEPS``: no line of the entry
point clears the flags; ``DROPS``: it clears them, or it is an evaluation of another size or precision, which must not
reuse.  The test measures which of the two happens.

Sizes: the smallest with padding on every axis.  N = 200 stimuli (np = 256: 56 padded rows; 208 for the sweeps, which
take multiples of 16) on an 8 x 8 pixel grid whose mask keeps 56 pixels (d < d_full, dp = 64); nb = 70 columns in the
projected forms, Nt = 150 inducing images in the sparse closure, k = 48 for sweeps and sign steps, P = 130 pool rows,
k = 5 appended columns; contexts of capacity ``CAP`` = 384, so that np_cap > np and the region behind the padded problem exists (and is poisoned).  The large probe
(``LARGE``, poison test only) is the closure at N = 2100, d = 64 on a context of capacity 2304: the padded size 2176
splits unevenly and reaches the block forms (the top node in blocks, the block row solve, no top inverse block), whose
buffer roles exist from 2048 up.  Inputs are seeded: ``synthetic``, ``estep_damped_cases.make_case``, the oracle's metric
and kernel, ``test_sign_chain_cpu.gap_matrix``.  Everything on the host is computed once (``host()``), uploaded once
(``dev()``) and never written: a builder clones what its call updates in place."""
import collections
import ctypes
import functools
import math

import numpy as np
import torch

import estep_damped_cases as dcases
from gaussian_processes_amd import _lib, eigtop, synthetic as syn
from oracle import gp_oracle as orc
from test_sign_chain_cpu import TAU, gap_matrix

KEEPS, DROPS = "keeps", "drops"
POISON = (0xFF, 0x47)       # NaN in fp64 and fp32; a finite value far from the data (fmin / fmax and comparisons swallow NaN)
SENTINEL = -7.25
INT_SENTINEL = -77
N, NB, NT, KS, P, KA = 200, 70, 150, 48, 130, 5
NS = 208                    # rows of the sweeps probe: gpfit_subspace_sweeps takes multiples of 16 (np = 256 as for N)
ROWS, COLS = 8, 8
D_FULL = ROWS * COLS
CAP = 384
N_LARGE, CAP_LARGE = 2100, 2304
N_BASE = 150                # the evaluation the cache test repeats: np = 256 as the probes', another lv_n
GROUP_UNITS = 3
LOWER, UPPER = syn.limits()
KEYS = syn.THETA_KEYS
LOG_A, LAMBDA0 = syn.F_PARAMS["logA"], syn.F_PARAMS["lambda0"]
CS = eigtop._sign_schedule(eigtop._SIGN_L0, 0, 40)[0][:2]
LBFGS = (0.1, 1e-7, 1e-9)
NFP = 10
ALPHA = 0.5


def theta_small(unit=0):
    """A receptive field narrow enough for the mask to drop pixels of the 8 x 8 grid (56 of 64 stay)."""
    th = dict(syn.theta0())
    th["-2log2beta"] = -2.0 * math.log(2 * 0.25)
    th["eps_0x"] = 0.3
    th["Amp"] = 1.0 + 0.01 * unit
    return th


Probe = collections.namedtuple("Probe", "name entry cache units build")


class Call:
    def __init__(self, run, **outs):
        self.run, self.outs = run, outs


# ---------------------------------------------------------------------------------------------- inputs
def _qr(rng, rows, cols):
    return np.ascontiguousarray(np.linalg.qr(rng.standard_normal((rows, cols)))[0])


def _sym(M):
    return (M + M.T) / 2


@functools.lru_cache(maxsize=None)
def host():
    """Every input of the small probes, numpy fp64 (torch on the host for the oracle's pieces)."""
    rng = np.random.default_rng(20240)
    th = theta_small()
    X = syn.stimuli(N, D_FULL, seed=3)
    Xpool = syn.stimuli(P, D_FULL, seed=4)
    r, m = syn.cell_inputs(N)
    C, mask, dC = orc.spatial_metric(th, LOWER, UPPER, (ROWS, COLS), grad=True)
    mask = mask.numpy().astype(bool)
    d = int(mask.sum())
    assert 32 < d < D_FULL, d                       # a partial mask, dp = 64
    Xm, Xpm = np.ascontiguousarray(X[:, mask]), np.ascontiguousarray(Xpool[:, mask])
    Kx = _sym(orc.arccos_gram(th, torch.from_numpy(Xm), torch.from_numpy(Xm), C).numpy())
    full = dcases.make_case(N, N, 1e4, "newton")
    proj = dcases.make_case(N, NB, 1e4, "newton")
    L = np.linalg.cholesky(proj["K"])
    Linv = np.tril(np.linalg.solve(L, np.eye(NB)))
    Kinv = _sym(np.linalg.inv(proj["K"]))
    Xs = syn.stimuli(NS, D_FULL, seed=6)[:, mask]
    Ks = _sym(orc.arccos_gram(th, torch.from_numpy(Xs), torch.from_numpy(Xs), C).numpy())
    Q0 = _qr(rng, NS, KS)
    W = rng.standard_normal((N, N))
    Lf = np.linalg.cholesky(full["K"])
    Lfi = np.tril(np.linalg.solve(Lf, np.eye(N)))

    def embedded(n):
        """The factor of the leading n x n block and its inverse in N x N arrays (the rows behind them zero)."""
        A, Ai = np.zeros((N, N)), np.zeros((N, N))
        A[:n, :n], Ai[:n, :n] = Lf[:n, :n], Lfi[:n, :n]    # (the factor of a leading block is the leading block of the factor)
        return A, Ai
    h = dict(
        theta=th, mask=mask, d=d, X=X, Xpool=Xpool, Xm=Xm, Xpm=Xpm, r=r, m=m, C=C.numpy(),
        dC=np.ascontiguousarray(np.stack([dC[k].numpy() for k in orc.DC_KEYS])), Kx=Kx, V=0.5 * Kx,
        full_K=full["K"], full_V=full["V"], full_m=full["m"], full_f=full["f"], full_r=full["r"],
        a=proj["a"], aL=proj["a"] @ L, L=L, Linv=Linv, pK=proj["K"], pKinv=Kinv, pV=proj["V"], pm=proj["m"], pf=proj["f"],
        pr=proj["r"], kv0=0.05 + 0.1 * rng.random(N), lam_m=proj["a"] @ proj["m"], lam_var=0.05 + 0.1 * rng.random(N),
        B=_qr(rng, N, NB), Bt=_qr(rng, NT, NB), Ks=Ks, Q0=Q0, shift=0.6 * float(np.min(np.sum(Q0 * (Ks @ Q0), 0))),
        W=_sym(W), gvec=rng.random(N), Wrect=rng.standard_normal((N, P)), t1=0.1 * rng.random(N),
        poolS=_sym(Kinv @ (proj["V"] - proj["K"]) @ Kinv), poolw=Kinv @ proj["m"], counts=np.arange(0.0, 20.0))
    for key, n in (("app1", N - 1), ("appk", N - KA)):
        h[key + "_L"], h[key + "_Li"] = embedded(n)
    return h


def T(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


@functools.lru_cache(maxsize=None)
def dev():
    """The inputs on the device, uploaded once; read only."""
    h = host()
    d = {k: T(v) for k, v in h.items() if isinstance(v, np.ndarray) and v.dtype == np.float64}
    d["mask"] = torch.from_numpy(h["mask"]).cuda()
    d["S_sign"] = [gap_matrix(KS, 1.0, seed=u, scale=1.0 + 0.25 * u).cuda().contiguous() for u in range(GROUP_UNITS)]
    for key in ("X", "r", "m", "V"):
        d[key + "32"] = d[key].to(torch.float32)
    return d


@functools.lru_cache(maxsize=None)
def dev_sized(n, seed):
    """(X, r, m, V) of a closure at another size, fp64 and fp32: the large probe, the evaluation of the cache test."""
    th = dict(syn.theta0()) if n == N_LARGE else theta_small()
    X = syn.stimuli(n, D_FULL, seed=seed)
    r, m = syn.cell_inputs(n, cell=seed)
    C, mask = orc.spatial_metric(th, LOWER, UPPER, (ROWS, COLS))
    Xm = torch.from_numpy(np.ascontiguousarray(X[:, mask.numpy().astype(bool)]))
    V = 0.5 * _sym(orc.arccos_gram(th, Xm, Xm, C).numpy())
    t64 = tuple(T(a) for a in (X, r, m, V))
    return th, t64, tuple(t.to(torch.float32) for t in t64)


# ---------------------------------------------------------------------------------------------- helpers
def gp():
    from gaussian_processes_amd import utils
    return utils


def lib():
    return _lib.load()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def doubles(n):
    return (ctypes.c_double * n)(*([SENTINEL] * n))


def ints(n):
    return (ctypes.c_int * n)(*([INT_SENTINEL] * n))


def out_tensor(*shape, dtype=torch.float64):
    return torch.full(shape, SENTINEL, dtype=dtype, device="cuda")


def tdict(theta):
    return {k: torch.tensor(float(theta[k]), dtype=torch.float64) for k in KEYS}


def fparams(logA=LOG_A, lambda0=LAMBDA0):
    return {"logA": torch.tensor(logA, dtype=torch.float64), "lambda0": torch.tensor(lambda0, dtype=torch.float64)}


def one(engines):
    assert len(engines) == 1
    return engines[0]


def placed(q, eng):
    """The request runs on the engine under test."""
    assert q["engine"] is eng and q["engine"]._ctx.value == eng._ctx.value
    return q


def ctx_table(engines):
    return [e._ctx for e in engines]


def buffer_names():
    """The names ``gpfit_dev_ctx_fill`` knows, from the library's own enumerator."""
    names, buf = [], ctypes.create_string_buffer(64)
    while lib().gpfit_dev_ctx_buffer_name(len(names), buf, 64) == 0:
        names.append(buf.value.decode())
    return names


def fill_workspace(eng, byte):
    """Every floating-point work buffer of the engine's context filled with ``byte``."""
    for name in buffer_names():
        rc = lib().gpfit_dev_ctx_fill(eng._ctx, name.encode(), byte)
        assert rc == 0, (name, rc, _lib.last_error())


def collect(call):
    """What the call's outputs hold now, detached from the buffers: tensors as copies, doubles as hex, ints as ints."""
    torch.cuda.synchronize()
    got = {}
    for name, v in call.outs.items():
        if isinstance(v, torch.Tensor):
            got[name] = v.detach().clone()
        elif isinstance(v, ctypes.Array) and v._type_ is ctypes.c_double:
            got[name] = [float(x).hex() for x in v]
        else:
            got[name] = [int(x) for x in v]
    return got


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def differences(got, want):
    """The names whose bits differ (NaN equal to NaN of the same bits; hex strings compare NaN as 'nan')."""
    assert got.keys() == want.keys()
    bad = []
    for name in got:
        a, b = got[name], want[name]
        if isinstance(a, torch.Tensor):
            if a.shape != b.shape or not torch.equal(bits(a), bits(b)):
                both_nan = a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())
                if not both_nan:
                    bad.append(name)
        elif a != b:
            bad.append(name)
    return bad


def untouched(got):
    """The outputs that still hold nothing but the sentinel."""
    def is_sentinel(v):
        if isinstance(v, torch.Tensor):
            return bool((v == SENTINEL).all())
        return all(x in (float(SENTINEL).hex(), INT_SENTINEL) for x in v)
    return [name for name, v in got.items() if is_sentinel(v)]


# ---------------------------------------------------------------------------------------------- the closures
def _fit_eval_call(eng, theta, tensors, flags):
    """gpfit_fit_eval / _f32 (by the tensors' type) with the argument list of GPFitEngine.fit_eval_async."""
    X, r, m, V = tensors
    n = X.shape[0]
    out = doubles(16)
    vecs = out_tensor(3, n, dtype=X.dtype)
    entry = lib().gpfit_fit_eval_f32 if X.dtype == torch.float32 else lib().gpfit_fit_eval
    th, lo, up = (_lib.darr([t[k] for k in KEYS]) for t in (theta, LOWER, UPPER))

    def run():
        return entry(eng._ctx, stream(), th, lo, up, ROWS, COLS, X.data_ptr(), X.stride(0), n, r.data_ptr(), m.data_ptr(),
                     V.data_ptr(), V.stride(0), LOG_A, LAMBDA0, flags, out, vecs[0].data_ptr(), vecs[1].data_ptr(),
                     vecs[2].data_ptr())
    return Call(run, out=out, vectors=vecs)


def fit_eval(flags, f32=False, large=False):
    def build(engines):
        if large:
            theta, t64, t32 = dev_sized(N_LARGE, 5)
            return _fit_eval_call(one(engines), theta, t32 if f32 else t64, flags)
        D = dev()
        return _fit_eval_call(one(engines), theta_small(), tuple(D[k + ("32" if f32 else "")] for k in ("X", "r", "m", "V")), flags)
    return build


def base_eval(eng, instance, reuse_V=False, async_call=False):
    """The evaluation the cache and pending tests repeat: ``instance`` "f64", "mixed" or "f32", at N_BASE."""
    theta, t64, t32 = dev_sized(N_BASE, 9)
    flags = 1 | (2 if reuse_V else 0) | (4 if async_call else 0) | (8 if instance == "mixed" else 0)
    return _fit_eval_call(eng, theta, t32 if instance == "f32" else t64, flags)


def _fit_batch(engines, f32, flags):
    """gpfit_fit_eval_batch / _f32 with the argument list of engine.fit_eval_group_begin, each unit collected."""
    D, nu = dev(), len(engines)
    sfx = "32" if f32 else ""
    X, r, V = D["X" + sfx], D["r" + sfx], D["V" + sfx]
    ms = [(D["m" + sfx] * (1.0 + 0.5 * u)).contiguous() for u in range(nu)]
    theta = _lib.darr([theta_small(u)[k] for u in range(nu) for k in KEYS])
    lo, up = (_lib.darr([t[k] for k in KEYS]) for t in (LOWER, UPPER))
    out, rcs = doubles(16 * nu), ints(nu)
    entry = lib().gpfit_fit_eval_batch_f32 if f32 else lib().gpfit_fit_eval_batch

    def ptrs(ts):
        return (ctypes.c_void_p * nu)(*[t.data_ptr() for t in ts])

    def run():
        rc = entry(gp()._ctx_table(ctx_table(engines)), nu, stream(), theta, lo, up, ROWS, COLS, ptrs([X] * nu), X.stride(0), N,
                   ptrs([r] * nu), ptrs(ms), ptrs([V] * nu), V.stride(0), _lib.darr([LOG_A + 0.1 * u for u in range(nu)]),
                   _lib.darr([LAMBDA0] * nu), flags, out, rcs)
        if rc != 0:
            return rc
        for u, e in enumerate(engines):      # the batch call only enqueues: every pending unit is collected
            if rcs[u] == 0:
                o = (ctypes.c_double * 16)()
                rc = lib().gpfit_fit_eval_finish(e._ctx, o) or rc
                out[16 * u:16 * u + 16] = list(o)
        return rc
    return Call(run, out=out, rcs=rcs)


def _closure_unit(u, sparse):
    D = dev()
    th = tdict(theta_small(u))
    unit = dict(theta=th, lims=(LOWER, UPPER), n_px_side=(ROWS, COLS), x=D["X"], r=D["r"], B=D["Bt"] if sparse else D["B"],
                m_b=D["pm"] * (1.0 + 0.5 * u), V_b=D["pV"], f_params=fparams(LOG_A + 0.1 * u))
    if sparse:
        unit["xtilde"] = D["X"][:NT].contiguous()
    return unit


def closure(sparse):
    def build(engines):
        eng = one(engines)
        q = placed(gp()._closure_prepare(engine=eng, **_closure_unit(0, sparse)), eng)
        out = doubles(16)
        x, B, V = q["x"], q["B"], q["V_b"]
        entry = lib().gpfit_fit_eval_sparse if sparse else lib().gpfit_fit_eval_projected
        xt = (q["xt"].data_ptr(), q["xt"].stride(0), q["Nt"]) if sparse else ()

        def run():     # the argument list of utils._closure_run_single
            return entry(eng._ctx, q["stream"], _lib.darr(q["theta"]), _lib.darr(q["lower"]), _lib.darr(q["upper"]), q["rows"],
                         q["cols"], x.data_ptr(), x.stride(0), q["N"], *xt, q["r"].data_ptr(), B.data_ptr(), B.stride(0),
                         q["n_kept"], q["m_b"].data_ptr(), V.data_ptr(), V.stride(0), q["logA"], q["lambda0"], out)
        return Call(run, out=out)
    return build


def closure_batch(sparse):
    def build(engines):
        qs = [placed(gp()._closure_prepare(engine=e, **_closure_unit(u, sparse)), e) for u, e in enumerate(engines)]
        out, rcs = doubles(16 * len(qs)), ints(len(qs))
        return Call(lambda: gp()._closure_batch_raw(ctx_table(engines), qs, out, rcs)[0], out=out, rcs=rcs)
    return build


def grad_pullback(engines):
    eng, D = one(engines), dev()
    th, out = _lib.darr([theta_small()[k] for k in KEYS]), doubles(6)
    X, W, g = D["X"], D["W"], D["gvec"]
    return Call(lambda: lib().gpfit_grad_pullback(eng._ctx, stream(), th, ROWS, COLS, X.data_ptr(), X.stride(0), N, W.data_ptr(),
                                                  W.stride(0), g.data_ptr(), out), out=out)


# ---------------------------------------------------------------------------------------------- the kernel functions
def localker(engines):
    eng, h = one(engines), host()
    d = h["d"]
    th = _lib.darr([h["theta"][k] for k in KEYS])
    mbuf = (ctypes.c_uint8 * D_FULL)(*[int(v) for v in h["mask"]])
    C, dC = out_tensor(d, d), out_tensor(5, d, d)
    return Call(lambda: lib().gpfit_localker(eng._ctx, stream(), th, ROWS, COLS, mbuf, d, C.data_ptr(), dC.data_ptr()), C=C, dC=dC)


def acosker_rect(engines):
    eng, D, d = one(engines), dev(), host()["d"]
    x1, x2, C, dC = D["Xm"], D["Xpm"], D["C"], D["dC"]
    K, dK = out_tensor(N, P), out_tensor(6, N, P)

    def run():
        rc = lib().gpfit_acosker(eng._ctx, stream(), 1.0, x1.data_ptr(), x1.stride(0), N, x2.data_ptr(), x2.stride(0), P, d,
                                 C.data_ptr(), C.stride(0), dC.data_ptr(), K.data_ptr(), K.stride(0), dK.data_ptr())
        torch.cuda.synchronize()       # (the call only enqueues)
        return rc
    return Call(run, K=K, dK=dK)


def acosker_pullback(engines):
    eng, D, d = one(engines), dev(), host()["d"]
    x1, x2, C, W, t1 = D["Xm"], D["Xpm"], D["C"], D["Wrect"], D["t1"]
    M, out = out_tensor(d, d), doubles(3)
    return Call(lambda: lib().gpfit_acosker_pullback(eng._ctx, stream(), 1.0, x1.data_ptr(), x1.stride(0), N, x2.data_ptr(),
                                                     x2.stride(0), P, d, C.data_ptr(), C.stride(0), W.data_ptr(), W.stride(0),
                                                     t1.data_ptr(), M.data_ptr(), M.stride(0), out), M=M, out=out)


def acosker_diag(engines):
    eng, D, d = one(engines), dev(), host()["d"]
    x1, C, dC = D["Xm"], D["C"], D["dC"]
    Kvec, dKvec = out_tensor(N), out_tensor(6, N)

    def run():
        rc = lib().gpfit_acosker_diag(eng._ctx, stream(), 1.0, x1.data_ptr(), x1.stride(0), N, d, C.data_ptr(), C.stride(0),
                                      dC.data_ptr(), Kvec.data_ptr(), dKvec.data_ptr())
        torch.cuda.synchronize()       # (the call only enqueues)
        return rc
    return Call(run, Kvec=Kvec, dKvec=dKvec)


# ---------------------------------------------------------------------------------------------- factorisations
def potrf(engines):
    eng, A = one(engines), dev()["full_K"]
    L, Li, logdet, info = out_tensor(N, N), out_tensor(N, N), doubles(1), ints(1)
    return Call(lambda: lib().gpfit_potrf(eng._ctx, stream(), A.data_ptr(), A.stride(0), N, L.data_ptr(), L.stride(0), Li.data_ptr(),
                                          Li.stride(0), logdet, info), L=L, Linv=Li, logdet=logdet, info=info)


def potrf_append(engines):
    eng, D = one(engines), dev()
    L, Li, kcol = D["app1_L"].clone(), D["app1_Li"].clone(), D["full_K"][:, N - 1].contiguous()
    logdet, info = (ctypes.c_double * 1)(1.5), ints(1)
    return Call(lambda: lib().gpfit_potrf_append(eng._ctx, stream(), L.data_ptr(), L.stride(0), Li.data_ptr(), Li.stride(0), N - 1,
                                                 kcol.data_ptr(), logdet, info), L=L, Linv=Li, logdet=logdet, info=info)


def potrf_append_block(engines):
    eng, D = one(engines), dev()
    L, Li, Kcols = D["appk_L"].clone(), D["appk_Li"].clone(), D["full_K"][:, N - KA:].contiguous()
    logdet, info = (ctypes.c_double * 1)(1.5), ints(1)
    return Call(lambda: lib().gpfit_potrf_append_block(eng._ctx, stream(), L.data_ptr(), L.stride(0), Li.data_ptr(), Li.stride(0),
                                                       N - KA, KA, Kcols.data_ptr(), Kcols.stride(0), logdet, info),
                L=L, Linv=Li, logdet=logdet, info=info)


# ---------------------------------------------------------------------------------------------- E-steps
def estep(engines):
    eng, D = one(engines), dev()
    K, r, m, f = D["full_K"], D["full_r"], D["full_m"], D["full_f"]
    m_new, V_new = out_tensor(N), out_tensor(N, N)
    return Call(lambda: lib().gpfit_estep(eng._ctx, stream(), K.data_ptr(), K.stride(0), N, r.data_ptr(), m.data_ptr(), f.data_ptr(),
                                          dcases.LOG_A, m_new.data_ptr(), V_new.data_ptr(), V_new.stride(0)), m=m_new, V=V_new)


def estep_projected(engines):
    eng, D = one(engines), dev()
    a, aL, L, r, m, f, kv0 = (D[k] for k in ("a", "aL", "L", "pr", "pm", "pf", "kv0"))
    m_new, V_new, lam = out_tensor(NB), out_tensor(NB, NB), out_tensor(2, N)
    return Call(lambda: lib().gpfit_estep_projected(eng._ctx, stream(), a.data_ptr(), a.stride(0), aL.data_ptr(), aL.stride(0),
                                                    L.data_ptr(), L.stride(0), N, NB, r.data_ptr(), m.data_ptr(), f.data_ptr(),
                                                    dcases.LOG_A, m_new.data_ptr(), V_new.data_ptr(), V_new.stride(0), kv0.data_ptr(),
                                                    lam[0].data_ptr(), lam[1].data_ptr()), m=m_new, V=V_new, moments=lam)


def estep_projected_damped(engines):
    eng, D = one(engines), dev()
    a, aL, L, Li, V, r, m, f = (D[k] for k in ("a", "aL", "L", "Linv", "pV", "pr", "pm", "pf"))
    m_new, V_new, info = out_tensor(NB), out_tensor(NB, NB), ints(1)
    return Call(lambda: lib().gpfit_estep_projected_damped(
        eng._ctx, stream(), a.data_ptr(), a.stride(0), aL.data_ptr(), aL.stride(0), L.data_ptr(), L.stride(0), Li.data_ptr(),
        Li.stride(0), V.data_ptr(), V.stride(0), N, NB, r.data_ptr(), m.data_ptr(), f.data_ptr(), dcases.LOG_A, ALPHA,
        m_new.data_ptr(), V_new.data_ptr(), V_new.stride(0), info), m=m_new, V=V_new, info=info)


def fparam_eval(engines):
    eng, D = one(engines), dev()
    lm, lv, r = D["lam_m"], D["lam_var"], D["pr"]
    f, out = out_tensor(N), doubles(7)
    return Call(lambda: lib().gpfit_fparam_eval(eng._ctx, stream(), lm.data_ptr(), lv.data_ptr(), r.data_ptr(), N, dcases.LOG_A, 1, 0.0,
                                                f.data_ptr(), out), f=f, out=out)


def fparam_lbfgs(engines):
    eng, D = one(engines), dev()
    lm, lv, r = D["lam_m"], D["lam_var"], D["pr"]
    f, out = out_tensor(N), doubles(9)
    return Call(lambda: lib().gpfit_fparam_lbfgs(eng._ctx, stream(), lm.data_ptr(), lv.data_ptr(), r.data_ptr(), N, dcases.LOG_A, 0, 0.0,
                                                 NFP, NFP, *LBFGS, f.data_ptr(), out), f=f, out=out)


def _chain_request(kind, eng, u):
    """A chain request of two steps on ``eng``; the state the call updates is the request's own (utils._chain_request)."""
    D, g = dev(), gp()
    logA0, m_scale = dcases.LOG_A + 0.1 * u, 1.0 + 0.5 * u
    if kind == "chain_full":
        q = g._chain_full_prepare(D["full_r"], D["full_K"], D["kv0"], D["full_m"] * m_scale, D["full_f"], logA0, 2, NFP, engine=eng)
    elif kind == "chain":
        q = g._chain_prepare(D["pr"], D["a"], D["aL"], D["L"], D["kv0"], D["pm"] * m_scale, D["pf"], logA0, 2, NFP, engine=eng)
    else:
        q = g._chain_damped_prepare(D["pr"], D["a"], D["aL"], D["L"], D["Linv"], D["kv0"], D["pV"], D["pm"] * m_scale, D["pf"],
                                    logA0, ALPHA, 2, NFP, engine=eng)
    for key in ("lam_m", "lam_var") + (("V",) if kind != "chain_damped" else ()):
        q[key].fill_(SENTINEL)           # (allocated uninitialised by the request)
    return placed(q, eng)


def _chain_outs(qs, rec):
    outs = {"rec": rec}
    for u, q in enumerate(qs):
        outs.update({f"{key}{u}": q[key] for key in ("m", "f", "V", "lam_m", "lam_var")})
    return outs


def chain(kind):
    def build(engines):
        q = _chain_request(kind, one(engines), 0)
        rec = doubles(12 * 2)
        return Call(lambda: gp()._chain_call(kind, None, [q], rec)[0], **_chain_outs([q], rec))
    return build


def chain_batch(kind):
    def build(engines):
        qs = [_chain_request(kind, e, u) for u, e in enumerate(engines)]
        rec = doubles(12 * 2 * len(qs))
        return Call(lambda: gp()._chain_call(kind, ctx_table(engines), qs, rec)[0], **_chain_outs(qs, rec))
    return build


# ---------------------------------------------------------------------------------------------- the tracked loss
def _loss_request(eng, u):
    D = dev()
    return placed(gp()._loss_prepare(D["pr"], D["pf"], D["lam_m"], fparams(dcases.LOG_A + 0.1 * u), D["pm"] * (1.0 + 0.5 * u), D["pV"],
                                     D["pK"], D["pKinv"], engine=eng), eng)


def elbo(engines):
    eng = one(engines)
    q = _loss_request(eng, 0)
    out, info = doubles(10), ints(2)
    K = q["K"]

    def run():       # the argument list of utils._loss_run_single
        return lib().gpfit_elbo(eng._ctx, q["stream"], q["m"].data_ptr(), q["V"].data_ptr(), q["V"].stride(0), K.data_ptr(), K.stride(0),
                                q["Kinv"].data_ptr(), q["Kinv"].stride(0), q["nb"], 0, 0.0, q["r"].data_ptr(), q["f"].data_ptr(),
                                q["lam_m"].data_ptr(), q["N"], q["logA"], q["lambda0"], out, info)
    return Call(run, out=out, info=info)


def elbo_batch(engines):
    qs = [_loss_request(e, u) for u, e in enumerate(engines)]
    out, info = doubles(10 * len(qs)), ints(2 * len(qs))
    return Call(lambda: gp()._loss_batch_raw(ctx_table(engines), qs, out, info)[0], out=out, info=info)


# ---------------------------------------------------------------------------------------------- the basis rebuild
def _sweeps_request(eng, u):
    D, s = dev(), host()["shift"]
    q = placed(gp()._sweeps_prepare(D["Ks"], D["Q0"], None, (0.0, s * (1.0 - 0.2 * u)), True, engine=eng), eng)
    for key in ("Y", "W", "S"):
        q[key].fill_(SENTINEL)
    return q


def _block_outs(qs, keys, rec):
    outs = {"rec": rec}
    for u, q in enumerate(qs):
        outs.update({f"{key}{u}": q[key] for key in keys})
    return outs


def sweeps(engines):
    eng = one(engines)
    q, rec = _sweeps_request(eng, 0), ints(2)
    K, sigma = q["K"], _lib.darr(q["shifts"])

    def run():       # the argument list of utils._sweeps_run_single
        return lib().gpfit_subspace_sweeps(eng._ctx, q["stream"], K.data_ptr(), K.stride(0), q["N"], q["k"], q["Q"].data_ptr(),
                                           q["Y"].data_ptr(), q["W"].data_ptr(), q["S"].data_ptr(), len(q["shifts"]), sigma,
                                           q["flags"], rec)
    return Call(run, **_block_outs([q], ("Q", "Y", "W", "S"), rec))


def sweeps_batch(engines):
    qs = [_sweeps_request(e, u) for u, e in enumerate(engines)]
    rec = ints(2 * len(qs))
    return Call(lambda: gp()._sweeps_batch_raw(ctx_table(engines), qs, rec)[0], **_block_outs(qs, ("Q", "Y", "W", "S"), rec))


def _sign_request(eng, u):
    q = placed(gp()._sign_prepare(dev()["S_sign"][u], TAU * (1.0 + 0.25 * u), None, None, CS, 0, engine=eng), eng)
    for key in ("X", "X2", "W"):
        q[key].fill_(SENTINEL)
    return q


def sign(engines):
    eng = one(engines)
    q, rec = _sign_request(eng, 0), ints(2)

    def run():       # the argument list of utils._sign_run_single
        return lib().gpfit_sign_steps(eng._ctx, q["stream"], q["S"].data_ptr(), q["k"], q["tau"], q["X"].data_ptr(),
                                      q["X2"].data_ptr(), q["W"].data_ptr(), len(q["c"]), _lib.darr(q["c"]), q["its0"], q["flags"],
                                      rec)
    return Call(run, **_block_outs([q], ("X", "X2", "W"), rec))


def sign_batch(engines):
    qs = [_sign_request(e, u) for u, e in enumerate(engines)]
    rec = ints(2 * len(qs))
    return Call(lambda: gp()._sign_batch_raw(ctx_table(engines), qs, rec)[0], **_block_outs(qs, ("X", "X2", "W"), rec))


# ---------------------------------------------------------------------------------------------- the pool
def _pool_request(u):
    """Whole pool images with the mask, masked inducing images, a basis of NB columns (utils._score_pool_prepare)."""
    D = dev()
    folded = {"S": D["poolS"], "w": (D["poolw"] * (1.0 + 0.5 * u)).contiguous(), "B": D["B"], "k": NB}
    q = gp()._score_pool_prepare(D["Xpool"], D["Xm"], D["C"], tdict(theta_small()), folded, D["mask"])
    assert q["pix"] is not None and q["d"] < q["d_full"] and q["P"] == P
    q["A"], q["lambda0"] = math.exp(LOG_A + 0.1 * u), LAMBDA0
    return q


def score_pool(engines):
    eng, q, r = one(engines), _pool_request(0), dev()["counts"]
    xs, xt, C, pix, S, w, B = (q[key] for key in ("xstar", "xtilde", "C", "pix", "S", "w", "B"))
    o = out_tensor(4, P)

    def run():       # the argument list of utils._score_pool_call
        return lib().gpfit_score_pool(eng._ctx, stream(), q["sigma0"], xs.data_ptr(), xs.stride(0), P, pix.data_ptr(), q["d_full"],
                                      xt.data_ptr(), xt.stride(0), q["nt"], q["d"], C.data_ptr(), C.stride(0), B.data_ptr(),
                                      B.stride(0), q["k"], S.data_ptr(), S.stride(0), w.data_ptr(), q["A"], q["lambda0"],
                                      r.data_ptr(), r.numel(), 0, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                      o[3].data_ptr())
    return Call(run, mu_sigma2_rate_U=o)


def score_pool_batch(engines):
    qs, r = [_pool_request(u) for u in range(len(engines))], dev()["counts"]
    o = out_tensor(len(qs), 4, P)
    cols = [[o[u][j] for u in range(len(qs))] for j in range(4)]
    return Call(lambda: gp()._score_pool_batch_raw(ctx_table(engines), qs, r, 0, *cols), mu_sigma2_rate_U=o)


def pool_covariance(engines):
    eng, q = one(engines), _pool_request(0)
    xs, xt, C, pix, S, B = (q[key] for key in ("xstar", "xtilde", "C", "pix", "S", "B"))
    Sigma = out_tensor(P, P)
    return Call(lambda: lib().gpfit_pool_covariance(eng._ctx, stream(), q["sigma0"], xs.data_ptr(), xs.stride(0), P, pix.data_ptr(),
                                                    q["d_full"], xt.data_ptr(), xt.stride(0), q["nt"], q["d"], C.data_ptr(),
                                                    C.stride(0), B.data_ptr(), B.stride(0), q["k"], S.data_ptr(), S.stride(0),
                                                    Sigma.data_ptr(), Sigma.stride(0)), Sigma=Sigma)


# ---------------------------------------------------------------------------------------------- the registry
G = GROUP_UNITS
PROBES = (
    Probe("fit_eval_f64", "gpfit_fit_eval", DROPS, 1, fit_eval(1)),
    Probe("fit_eval_mixed", "gpfit_fit_eval", DROPS, 1, fit_eval(1 | 8)),
    Probe("fit_eval_f32", "gpfit_fit_eval_f32", DROPS, 1, fit_eval(1, f32=True)),
    Probe("fit_eval_nograd", "gpfit_fit_eval", DROPS, 1, fit_eval(0)),
    Probe("grad_pullback", "gpfit_grad_pullback", DROPS, 1, grad_pullback),
    Probe("fit_eval_projected", "gpfit_fit_eval_projected", DROPS, 1, closure(False)),
    Probe("fit_eval_sparse", "gpfit_fit_eval_sparse", DROPS, 1, closure(True)),
    # the three kernel functions: no line of them clears the flags, and none of their buffers holds V's factor
    Probe("localker", "gpfit_localker", KEEPS, 1, localker),
    Probe("acosker", "gpfit_acosker", KEEPS, 1, acosker_rect),
    Probe("acosker_diag", "gpfit_acosker_diag", KEEPS, 1, acosker_diag),
    Probe("acosker_pullback", "gpfit_acosker_pullback", DROPS, 1, acosker_pullback),
    Probe("potrf", "gpfit_potrf", KEEPS, 1, potrf),
    Probe("potrf_append", "gpfit_potrf_append", KEEPS, 1, potrf_append),
    Probe("potrf_append_block", "gpfit_potrf_append_block", KEEPS, 1, potrf_append_block),
    Probe("estep", "gpfit_estep", KEEPS, 1, estep),
    Probe("estep_projected", "gpfit_estep_projected", DROPS, 1, estep_projected),
    Probe("estep_projected_damped", "gpfit_estep_projected_damped", DROPS, 1, estep_projected_damped),
    Probe("fparam_eval", "gpfit_fparam_eval", KEEPS, 1, fparam_eval),
    Probe("fparam_lbfgs", "gpfit_fparam_lbfgs", KEEPS, 1, fparam_lbfgs),
    Probe("estep_chain", "gpfit_estep_chain", DROPS, 1, chain("chain")),
    Probe("estep_chain_full", "gpfit_estep_chain_full", KEEPS, 1, chain("chain_full")),
    Probe("estep_chain_damped", "gpfit_estep_chain_damped", DROPS, 1, chain("chain_damped")),
    Probe("elbo", "gpfit_elbo", DROPS, 1, elbo),
    Probe("subspace_sweeps", "gpfit_subspace_sweeps", KEEPS, 1, sweeps),
    Probe("sign_steps", "gpfit_sign_steps", KEEPS, 1, sign),
    Probe("score_pool", "gpfit_score_pool", KEEPS, 1, score_pool),
    Probe("pool_covariance", "gpfit_pool_covariance", KEEPS, 1, pool_covariance),
    # group probes: three units, one context each
    Probe("fit_eval_batch", "gpfit_fit_eval_batch", DROPS, G, lambda engines: _fit_batch(engines, False, 1)),
    Probe("fit_eval_batch_f32", "gpfit_fit_eval_batch_f32", DROPS, G, lambda engines: _fit_batch(engines, True, 1)),
    Probe("fit_eval_projected_batch", "gpfit_fit_eval_projected_batch", DROPS, G, closure_batch(False)),
    Probe("fit_eval_sparse_batch", "gpfit_fit_eval_sparse_batch", DROPS, G, closure_batch(True)),
    Probe("estep_chain_batch", "gpfit_estep_chain_batch", DROPS, G, chain_batch("chain")),
    Probe("estep_chain_full_batch", "gpfit_estep_chain_full_batch", KEEPS, G, chain_batch("chain_full")),
    Probe("estep_chain_damped_batch", "gpfit_estep_chain_damped_batch", DROPS, G, chain_batch("chain_damped")),
    Probe("elbo_batch", "gpfit_elbo_batch", DROPS, G, elbo_batch),
    Probe("subspace_sweeps_batch", "gpfit_subspace_sweeps_batch", KEEPS, G, sweeps_batch),
    Probe("sign_steps_batch", "gpfit_sign_steps_batch", KEEPS, G, sign_batch),
    Probe("score_pool_batch", "gpfit_score_pool_batch", KEEPS, G, score_pool_batch),
)
# the poison test only
LARGE = (
    Probe("fit_eval_f64_2100", "gpfit_fit_eval", DROPS, 1, fit_eval(1, large=True)),
    Probe("fit_eval_mixed_2100", "gpfit_fit_eval", DROPS, 1, fit_eval(1 | 8, large=True)),
)
BY_NAME = {p.name: p for p in PROBES + LARGE}
SINGLE = tuple(p for p in PROBES if p.units == 1)
GROUPS = tuple(p for p in PROBES if p.units > 1)

# Entry points that take a context and have no probe, each with its reason.
EXEMPT = {
    "gpfit_ctx_destroy": "ends the context: nothing is left behind for a next call",
    "gpfit_fit_eval_finish": "the second half of an asynchronous gpfit_fit_eval: every closure probe goes through it, and the "
                             "pending test calls it by name",
    "gpfit_set_profile": "a host-side switch: launches nothing",
    "gpfit_get_profile": "reads host-side counters: launches nothing (the cache test reads its flops)",
    "gpfit_get_phases": "reads event timings of a phase-timed evaluation: launches nothing",
    "gpfit_last_enqueue_ms": "reads a host-side timing: launches nothing",
    "gpfit_dev_ctx_copy": "test hook: the means by which tests reach the work buffers",
    "gpfit_dev_ctx_fill": "test hook: the poison itself",
    "gpfit_dev_potrf": "test hook: the recursion on the caller's own buffers, reached by gpfit_potrf and every closure",
    "gpfit_dev_elementwise": "test hook: single launchers on the caller's own buffers",
    "gpfit_dev_skinny": "test hook: single launchers on the caller's own buffers",
    "gpfit_dev_projected": "test hook: single launchers on the caller's own buffers",
}
