"""Generate ``g11_estep_damped.npz`` by running the REAL reference's damped E-step on seeded inputs.

Run where the reference is mounted, as ``make_golden.py`` (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_damped.py

It imports the reference's ``utils.py`` unmodified (the directory ``make_golden.py`` names, or ``GPFIT_REFERENCE``),
calls its own ``Estep(..., V=V, alpha=a)`` (utils.py:1432-1436) on one problem of ``estep_damped_cases.make_case``
(N = 200, nb = 130, cond 1e4, V a previous Newton result) for a in {0.5, 0.05}, and stores the inputs with the
reference's ``(m_new, V_new)``.  Arrays only; no reference source is copied."""
import contextlib
import io
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.environ.get("GPFIT_REFERENCE", "/root/reference/Spatial_GP_repo"))
sys.dont_write_bytecode = True

with contextlib.redirect_stdout(io.StringIO()):
    import utils as ref  # noqa: E402  (the reference)

import estep_damped_cases as cases  # noqa: E402

N, NB, COND, V_KIND = 200, 130, 1e4, "newton"


def main():
    c = cases.make_case(N, NB, COND, V_KIND)
    t = {k: torch.tensor(v, dtype=torch.float64) for k, v in c.items() if k != "logA"}
    f_params = {"logA": torch.tensor(c["logA"], dtype=torch.float64)}
    out = dict(r=c["r"], a=c["a"], m=c["m"], f=c["f"], K=c["K"], V=c["V"], logA=np.float64(c["logA"]),
               alphas=np.array(cases.ALPHAS))
    for i, alpha in enumerate(cases.ALPHAS):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m_new, V_new = ref.Estep(t["r"], t["a"], t["m"], f_params, t["f"], K_tilde=t["K"], V=t["V"], alpha=alpha)
        out[f"m_new_{i}"] = m_new.detach().numpy()
        out[f"V_new_{i}"] = V_new.detach().numpy()
    path = os.path.join(HERE, "g11_estep_damped.npz")
    np.savez_compressed(path, **out)
    print(f"g11_estep_damped.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
