"""Inputs shared by the tests of the group form of the pool-scoring call (test_predict_group_cases_cpu.py,
test_gpu_predict_pool_group.py): several units -- the cells of a population -- on ONE pool of ``P`` whole images of 8 x 8
pixels.

Every unit follows the recipe of ``predict_cases.make_case`` (metric and mask from the oracle's ``localker``, posterior
``V = (K~_b^-1 + G)^-1`` formed in ``np.longdouble``, the top-``k`` eigenbasis when ``k < nt``) with its own inducing images,
posterior, ``sigma_0``, link parameters (``A``, ``lambda0`` around ``synthetic.F_PARAMS``) and its own pixel mask.  The metric's
mask keeps all 64 pixels of such an image, so a unit drops pixels itself, as
test_gpu_predict_pool.test_whole_images_with_a_mask_equal_masked_images does: ``C`` restricted to the kept pixels is a metric
like any other.  A unit is a dict that the helpers of ``predict_cases`` (``moments_longdouble``, ``moments_reassociated``,
``fold_f64``) take as a case.

Groups, as (nt, k, kept pixels) per unit -- the smallest shapes at which the group mechanisms can fail:
  PROJECTED3  P = 130: (200, 77, 64), (190, 100, 55), (256, 128, 40).  One bucket (padded 256 / 128 / 64): the true sizes
              all differ, one unit sits exactly on the tile edges, the row tiles are ragged.
  IDENTITY3   P = 300, identity basis: nt = k = 384, 300, 257 with 64, 64, 55 pixels.  One bucket (384); chunk_rows = 128
              gives three chunks, and the k ranges are 1, 2 and 3 tiles.
  SIXTEEN     P = 130: sixteen identity-basis units with nt from 65 to 128 -- the largest group.
  MIXED       PROJECTED3's units, an identity unit (200, 200, 64) and a projected unit keeping 30 pixels
              (round_up = 32): three buckets behind one score_pool_cells call.

``acosker`` -- the reference's, the oracle's and the library's -- symmetrises a square kernel matrix, and
``moments_longdouble`` asserts P != nt for that reason.  IDENTITY3's second unit has nt = P = 300: its references are taken
over the two halves of the pool (``reference_rows``), which are the same rows and the same arithmetic."""
import functools
import math

import numpy as np

import predict_cases as cases
from gaussian_processes_amd import synthetic as syn
from oracle import gp_oracle as orc
from test_kernel_reference_cpu import acosker_ld

LD = np.longdouble
PX = 8
NINE = (0, 5, 9, 17, 30, 31, 32, 50, 63)      # the pixels test_whole_images_with_a_mask_equal_masked_images drops

PROJECTED3 = ("PROJECTED3", 130, ((200, 77, 64), (190, 100, 55), (256, 128, 40)))
IDENTITY3 = ("IDENTITY3", 300, ((384, 384, 64), (300, 300, 64), (257, 257, 55)))
SIXTEEN = ("SIXTEEN", 130, tuple((n, n, 64) for n in (65, 70, 77, 81, 88, 90, 96, 99, 101, 107, 110, 113, 119, 120, 127, 128)))
MIXED = ("MIXED", 130, PROJECTED3[2] + ((200, 200, 64), (200, 77, 30)))
GROUPS = (PROJECTED3, IDENTITY3, SIXTEEN, MIXED)
BUCKETS = {"PROJECTED3": [(64, 256, 128, True)] * 3, "IDENTITY3": [(64, 384, 384, False)] * 3,
           "SIXTEEN": [(64, 128, 128, False)] * 16,
           "MIXED": [(64, 256, 128, True)] * 3 + [(64, 256, 256, False), (32, 256, 128, True)]}


def kept_pixels(kept):
    """The mask of a unit that keeps ``kept`` of the 64 pixels."""
    keep = np.ones(PX * PX, dtype=bool)
    if kept == 55:
        keep[list(NINE)] = False
    elif kept != PX * PX:
        keep[np.random.default_rng(kept).choice(PX * PX, PX * PX - kept, replace=False)] = False
    assert int(keep.sum()) == kept
    return keep


@functools.lru_cache(maxsize=None)
def pool(P):
    X = syn.stimuli(P, PX * PX, seed=31 + P)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def make_unit(P, nt, k, kept, index):
    """One unit on the pool of ``P`` images; ``index`` (its place in the group) varies sigma_0, the link and the seeds."""
    theta = dict(syn.theta0(), sigma_0=1.0 + 0.05 * index)
    xtilde = syn.stimuli(nt, PX * PX, seed=500 + 7 * index + nt)
    C_full, mask = orc.spatial_metric(theta, cases.LOWER, cases.UPPER, PX)
    assert bool(mask.all())                     # the metric keeps every pixel of an 8 x 8 image
    keep = kept_pixels(kept)
    C = np.ascontiguousarray(C_full.numpy().astype(np.float64)[keep][:, keep])
    Kt = np.asarray(acosker_ld(theta["sigma_0"], xtilde[:, keep], xtilde[:, keep], C)[0], dtype=np.float64)
    Kt = (Kt + Kt.T) / 2
    rng = np.random.default_rng(900 + 13 * index + nt + k)
    if k == nt:
        B, Kb = None, Kt
    else:
        ev, evec = np.linalg.eigh(Kt)
        B, Kb = np.ascontiguousarray(evec[:, nt - k:]), np.diag(ev[nt - k:])
    Kinv_ld = cases.inv_spd_ld(Kb)
    R = rng.standard_normal((k, k))
    G = (R @ R.T).astype(LD) / LD(10 * k)
    V = np.asarray(cases.inv_spd_ld(Kinv_ld + G), dtype=np.float64)
    Kinv = np.asarray(Kinv_ld, dtype=np.float64)
    return dict(P=P, nt=nt, k=k, px=PX, d=kept, theta=theta, xstar=pool(P), xtilde=xtilde, C=C, mask=keep, B=B, K=Kb,
                Kinv=(Kinv + Kinv.T) / 2, m=rng.standard_normal(k), V=(V + V.T) / 2,
                logA=syn.F_PARAMS["logA"] + 0.1 * index, lambda0=syn.F_PARAMS["lambda0"] - 0.05 * index)


def make_group(group):
    """The units of a group, in its order."""
    _, P, shapes = group
    return [make_unit(P, nt, k, kept, i) for i, (nt, k, kept) in enumerate(shapes)]


def reference_rows(c):
    """Row ranges over which a unit's references are evaluated: the whole pool, or its halves where P == nt."""
    P = c["P"]
    return (slice(0, P),) if P != c["nt"] else (slice(0, P // 2), slice(P // 2, P))


@functools.lru_cache(maxsize=None)
def reference(P, nt, k, kept, index):
    """The long-double moments of a unit, computed once and shared (never written)."""
    c = make_unit(P, nt, k, kept, index)
    parts = [cases.moments_longdouble(c, rows) for rows in reference_rows(c)]
    mu, s2 = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    mu.setflags(write=False)
    s2.setflags(write=False)
    return mu, s2


def group_reference(group):
    _, P, shapes = group
    return [reference(P, nt, k, kept, i) for i, (nt, k, kept) in enumerate(shapes)]


def moments_reassociated(c):
    """predict_cases.moments_reassociated over the unit's reference rows."""
    parts = [cases.moments_reassociated(dict(c, xstar=c["xstar"][rows])) for rows in reference_rows(c)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def bucket(c):
    """What score_pool_cells sorts a unit by: round_up(d, 32), round_up(nt, 128), round_up(k, 128), with a basis."""
    up = lambda v, m: int(math.ceil(v / m) * m)   # noqa: E731
    return (up(c["d"], 32), up(c["nt"], 128), up(c["k"], 128), c["B"] is not None)
