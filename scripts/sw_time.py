"""Time sample weights and cross-validation (DESIGN.md "Sample weights and cross-validation").

    PYTHONPATH=convex-optimization_amd python scripts/sw_time.py [--m 8192 --n 16384 --l 32 --dtype f64]

1. The weighted against the unweighted certified solve: ``sample_weight=None`` against all-ones
   weights, with and without screening, at mu = ratio * mu_max for every ratio of --ratios. The four
   arms share A, b and start from x = 0; after one pre-warm call per arm they alternate for --rounds
   rounds in one process, so all see the same machine state, and the spread of an arm over its rounds
   is the yardstick for a difference between arms. Seconds are taken inside the native call
   (info["tt"]). With ones the iterations must equal None's (the same bits under screen=False).
2. A --folds-fold glx.cv_path over --n-mus values of mu beside one full-data glx.path on the same
   grid: wall time, total iterations and the passes over A weighted by width. K folds of (K - 1) / K
   of the rows would ideally cost K (K - 1) / K paths; a fold here streams all m rows, the held-out
   ones with weight 0, so the ratio to expect is K.
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "convex-optimization_amd"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--l", type=int, default=32)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--ratios", default="0.5,0.1")
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--maxit", type=int, default=20000)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--n-mus", type=int, default=10)
    ap.add_argument("--skip-cv", action="store_true")
    ap.add_argument("--seed", type=int, default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import glx
    from glx.driver import SEED, gen_data
    from glx.screen import _Prepared

    m, n, l = a.m, a.n, a.l
    _, _, _, _, A, b, _u, _x0, *_ = gen_data(SEED if a.seed is None else a.seed, m, n, l)
    tdt = torch.float64 if a.dtype == "f64" else torch.float32
    Ad, bd = (torch.from_numpy(v).to("cuda", tdt) for v in (A, b))
    del A, b
    ones = np.ones(m, dtype=np.float64 if a.dtype == "f64" else np.float32)
    mu_top = glx.mu_max(Ad, bd)
    out = {"shape": [m, n, l], "dtype": a.dtype, "tol": a.tol, "rounds": a.rounds, "mu_max": mu_top,
           "mu_max_ones": glx.mu_max(Ad, bd, sample_weight=ones), "ratios": {},
           "device": torch.cuda.get_device_name(0)}

    arms = {"none_screen": _Prepared(Ad, bd, True), "ones_screen": _Prepared(Ad, bd, True, sw=ones),
            "none_plain": _Prepared(Ad, bd, False), "ones_plain": _Prepared(Ad, bd, False, sw=ones)}
    out["step"] = {name: prep.t for name, prep in arms.items()}
    for ratio in (float(v) for v in a.ratios.split(",")):
        mu = ratio * mu_top
        res = {name: {"native_s": []} for name in arms}
        for name, prep in arms.items():          # the pre-warm call of each arm
            _, info = prep.solve(mu, None, a.tol, a.maxit, 10)
            res[name].update({k: info[k] for k in ("iterations", "checks", "compactions", "kept_history", "kept",
                                                   "width", "passes", "rel_gap", "converged")})
        for _ in range(a.rounds):
            for name, prep in arms.items():
                torch.cuda.synchronize()
                _, info = prep.solve(mu, None, a.tol, a.maxit, 10)
                res[name]["native_s"].append(round(info["tt"], 5))
        for name in arms:
            w = res[name]["native_s"]
            res[name]["median_s"] = float(np.median(w))
            res[name]["spread_s"] = round(max(w) - min(w), 5)
        out["ratios"]["%g" % ratio] = res
        print("ratio %g done" % ratio, file=sys.stderr, flush=True)
    del arms
    torch.cuda.empty_cache()

    if not a.skip_cv:
        def figures(infos):
            return {"iterations": int(sum(i["iterations"] for i in infos)),
                    "passes": round(float(sum(i["passes"] for i in infos)), 1),
                    "native_s": round(float(sum(i["tt"] for i in infos)), 4)}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        path = glx.path(Ad, bd, n_mus=a.n_mus, tol=a.tol, maxit=a.maxit)
        torch.cuda.synchronize()
        out["path"] = {"wall_s": round(time.perf_counter() - t0, 3), **figures([p[2] for p in path])}
        print("path done", file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        cv = glx.cv_path(Ad, bd, folds=a.folds, n_mus=a.n_mus, tol=a.tol, maxit=a.maxit)
        torch.cuda.synchronize()
        out["cv"] = {"wall_s": round(time.perf_counter() - t0, 3), "folds": a.folds,
                     **figures([i for fold in cv["info"] for i in fold]), "best": cv["best"], "one_se": cv["one_se"],
                     "mean": [round(float(v), 6) for v in cv["mean"]], "se": [round(float(v), 6) for v in cv["se"]],
                     "converged": bool(all(i["converged"] for fold in cv["info"] for i in fold))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
