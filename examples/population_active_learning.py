"""The closed loop of examples/active_learning.py for a population: several cells recorded on the same images, and an image
shown on the rig is shown to all of them.  A round fits nothing twice:

  1. ``utils.varGP_cells``: the cells' start fits, together;
  2. ``utils.fold_posterior`` per cell;
  3. ``utils.score_pool_cells``: every remaining image scored for every cell -- the cells of a bucket in ONE device call
     (gpfit_score_pool_batch) -- and the utilities summed over the cells (gpfit_utility_sum);
  4. the ``--per-round`` images of largest population utility (``torch.topk``);
  5. ``utils.extend_inducing_set`` per cell with those images;
  6. ``utils.varGP_cells``: the refits, together.

    python examples/population_active_learning.py --cells 16 --pool 1200 --start 300 --rounds 3 --per-round 8
    python examples/population_active_learning.py --cells 16 --loop      # step 3 cell after cell (utils.score_pool), for the A/B
    python examples/population_active_learning.py --cells 16 --batch-aware

It prints the time of every phase of a round and the units each scoring call carried (``utils.last_pool_group_sizes``).
Both ways pick the same images: a cell's utilities have the same bits either way, and so has their sum.
``--batch-aware`` replaces steps 3 and 4 by ``utils.select_round`` (at most 16 cells): the same scoring, then the round's
images picked one by one from the shortlist of largest population utility, each conditioned on those already chosen
(gpfit_pool_covariance per cell, one gpfit_select_batch for all of them)."""
import argparse
import contextlib
import io
import os
import sys
import time
import warnings

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=4)
ap.add_argument("--pool", type=int, default=1200, help="images available")
ap.add_argument("--start", type=int, default=300, help="images of the initial fits")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--px", type=int, default=8, help="pixels per side")
ap.add_argument("--per-round", type=int, default=8, help="images added per round")
ap.add_argument("--max-units", type=int, default=16, help="cells per device call of the fits and of the scoring")
ap.add_argument("--loop", action="store_true", help="score cell after cell with utils.score_pool and sum on the host side")
ap.add_argument("--batch-aware", action="store_true",
                help="pick a round's images one by one, each conditioned on those already chosen (utils.select_round)")
args = ap.parse_args()
if args.per_round < 1 or args.cells < 1:
    ap.error("--per-round and --cells must be at least 1")
if args.batch_aware and (args.loop or args.cells > 16 or args.per_round > 128):
    ap.error("--batch-aware takes at most 16 cells and 128 images per round, and not --loop")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_processes_amd import utils as U  # noqa: E402
from gaussian_processes_amd import synthetic as syn  # noqa: E402

dev = torch.device("cuda")
d = args.px * args.px
X = torch.from_numpy(syn.stimuli(args.pool, d)).to(dev)
R = [torch.from_numpy(syn.cell_inputs(args.pool, cell)[0]).to(dev) for cell in range(args.cells)]
lower, upper = syn.limits()
all_idx = torch.arange(args.pool)
in_use = all_idx[: args.start]
r_counts = torch.arange(0, 100, dtype=torch.float64).to(dev)
quiet = lambda: contextlib.redirect_stdout(io.StringIO())  # noqa: E731


def start(cell):
    theta = {k: torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for k, v in syn.theta0(cell).items()}
    fit = {"ntilde": args.start, "maxiter": 3, "nEstep": 2, "nMstep": 3, "nFparamstep": 3, "kernfun": "acosker", "cellid": cell,
           "n_px_side": args.px, "display_hyper": False, "in_use_idx": in_use, "xtilde_idx": in_use}
    return {"fit_parameters": fit, "xtilde": X[in_use].clone(), "hyperparams_tuple": (theta, lower, upper),
            "f_params": {"logA": torch.tensor(syn.F_PARAMS["logA"]), "lambda0": torch.tensor(syn.F_PARAMS["lambda0"])}}


def fit_cells(kwargs_list):
    with quiet(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t0 = time.time()
        fits = U.varGP_cells(X[in_use], [r[in_use] for r in R], kwargs_list, max_units=args.max_units)
        torch.cuda.synchronize()
    failed = [cell for cell, (_, err) in enumerate(fits) if err["is_error"]]
    assert not failed, f"fits of cells {failed} failed"
    return [m for m, _ in fits], time.time() - t0


def logmarginal(models):
    return sum(float(m["values_track"]["loss_track"]["logmarginal"][-1]) for m in models) / len(models)


models, t_fit = fit_cells([start(cell) for cell in range(args.cells)])
print(f"{args.cells} cells, start fits on {args.start} images: {t_fit:.2f} s, mean log marginal {logmarginal(models):.3f}")
for rnd in range(args.rounds):
    remaining = all_idx[~torch.isin(all_idx, in_use)]
    if remaining.numel() == 0:
        break
    xstar = X[remaining]
    with quiet(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t0 = time.time()
        cells = [{"xtilde": X[in_use], "C": m["C"], "theta": m["hyperparams_tuple"][0], "f_params": m["f_params"], "mask": m["mask"],
                  "folded": U.fold_posterior(m["K_tilde_b"], m["K_tilde_inv_b"], m["m_b"], m["V_b"], m["B"])} for m in models]
        torch.cuda.synchronize()
        t_fold = time.time() - t0
        t0 = time.time()
        take = min(args.per_round, remaining.shape[0])
        if args.batch_aware:
            chosen = U.select_round(xstar, cells, take, r_counts)
            total, sizes = chosen["scores"]["population_utility"], list(U.last_pool_group_sizes)
            picks = chosen["picked"].cpu()
            best = remaining[picks[picks >= 0]]
            take = best.shape[0]
        elif args.loop:
            total, sizes = None, []
            for c in cells:
                u = U.score_pool(xstar, c["xtilde"], c["C"], c["theta"], c["folded"], c["f_params"], r_masked=r_counts,
                                 mask=c["mask"])["utility"]
                total = u if total is None else total + u
                sizes.append(1)
        else:
            scored = U.score_pool_cells(xstar, cells, r_masked=r_counts, max_units=args.max_units)
            failed = [cell for cell, err in enumerate(scored["errors"]) if err is not None]
            assert not failed, f"cells {failed} could not be scored: {scored['errors'][failed[0]]}"
            total, sizes = scored["population_utility"], list(U.last_pool_group_sizes)
        if not args.batch_aware:
            best = remaining[torch.topk(total, take).indices.cpu()]
        torch.cuda.synchronize()
        t_score = time.time() - t0
        t0 = time.time()
        in_use = torch.cat((in_use, best))
        nxt = []
        for m in models:
            grown = U.extend_inducing_set(m, X[best[0]] if take == 1 else X[best])
            kw = {"fit_parameters": dict(m["fit_parameters"]), "hyperparams_tuple": m["hyperparams_tuple"],
                  "f_params": m["f_params"], **grown}
            kw["fit_parameters"].update({"ntilde": in_use.shape[0], "in_use_idx": in_use, "xtilde_idx": in_use, "maxiter": 2})
            nxt.append(kw)
        torch.cuda.synchronize()
        t_prep = time.time() - t0
    models, t_fit = fit_cells(nxt)
    print(f"round {rnd + 1}: folded {args.cells} posteriors in {t_fold * 1e3:.1f} ms; scored {remaining.shape[0]} images for "
          f"{args.cells} cells in {t_score * 1e3:.1f} ms ({'select_round' if args.batch_aware else 'score_pool per cell' if args.loop else 'score_pool_cells'}, units per "
          f"call {sizes}; max population utility {float(total.max()):.4f}, images {[int(i) for i in best]}); refits prepared in "
          f"{t_prep * 1e3:.1f} ms, {args.cells} refits on {in_use.shape[0]} images in {t_fit:.2f} s, "
          f"mean log marginal {logmarginal(models):.3f}")
