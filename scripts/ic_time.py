"""Time the certified solve with an unpenalised intercept (DESIGN.md "Intercept").

    PYTHONPATH=convex-optimization_amd python scripts/ic_time.py [--m 8192 --n 16384 --l 32 --dtype f64]

Four arms on one (m, n, l): ``fit_intercept`` False and True on the offset instance (gen_data's A with
one default_rng(11) offset per column, b with three times one per column: the arms differ in step and
screening, not only in launches) and on the unshifted gen_data instance (where the intercept is nearly
zero and only the two extra launches per iteration differ). Each arm solves to --tol at every ratio of
--ratios times ITS OWN mu_max from x = 0. After one pre-warm call per arm they alternate for --rounds
rounds in one process, so all see the same machine state; the spread of an arm over its rounds is the
yardstick for a difference between arms. Seconds are taken inside the native call (info["tt"]).
``--trace-arm`` runs one intercept solve of at most --maxit iterations on the offset instance and
exits: the run to put under a kernel trace for the per-launch times. Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

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
    ap.add_argument("--trace-arm", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch
    import glx
    from glx.driver import SEED, gen_data
    from glx.screen import _Prepared

    m, n, l = a.m, a.n, a.l
    _, _, _, _, A, b, _u, _x0, *_ = gen_data(SEED, m, n, l)
    tdt = torch.float64 if a.dtype == "f64" else torch.float32
    g = np.random.default_rng(11)
    As = A + g.standard_normal(n)[None, :]
    bs = b + 3.0 * g.standard_normal(l)[None, :]
    data = {"offset": tuple(torch.from_numpy(v).to("cuda", tdt) for v in (As, bs))}
    del As, bs
    if a.trace_arm:
        Ad, bd = data["offset"]
        mu = 0.5 * glx.mu_max(Ad, bd, fit_intercept=True)
        _, info = glx.solve_certified(Ad, bd, mu, tol=a.tol, maxit=a.maxit, fit_intercept=True)
        print(json.dumps({"trace_arm": True, "iterations": info["iterations"], "rel_gap": info["rel_gap"]}))
        return
    data["plain"] = tuple(torch.from_numpy(v).to("cuda", tdt) for v in (A, b))
    del A, b
    out = {"shape": [m, n, l], "dtype": a.dtype, "tol": a.tol, "rounds": a.rounds, "arms": {}, "ratios": {},
           "device": torch.cuda.get_device_name(0)}
    arms = {}
    for inst, (Ad, bd) in data.items():
        for flag in (False, True):
            name = "%s_%s" % (inst, "intercept" if flag else "origin")
            prep = _Prepared(Ad, bd, True, intercept=flag)
            top = glx.mu_max(Ad, bd, fit_intercept=flag)
            arms[name] = (prep, top)
            out["arms"][name] = {"mu_max": top, "lambda_max": prep.lam, "step": prep.t}
    for ratio in (float(v) for v in a.ratios.split(",")):
        res = {name: {"native_s": []} for name in arms}
        for name, (prep, top) in arms.items():          # the pre-warm call of each arm
            _, info = prep.solve(ratio * top, None, a.tol, a.maxit, 10)
            res[name].update({k: info[k] for k in ("iterations", "checks", "compactions", "kept_history", "kept",
                                                   "width", "passes", "rel_gap", "converged")})
            if "intercept" in info:
                res[name]["intercept_max"] = float(np.max(np.abs(info["intercept"])))
        for _ in range(a.rounds):
            for name, (prep, top) in arms.items():
                torch.cuda.synchronize()
                _, info = prep.solve(ratio * top, None, a.tol, a.maxit, 10)
                res[name]["native_s"].append(round(info["tt"], 5))
        for name in arms:
            w = res[name]["native_s"]
            res[name]["median_s"] = float(np.median(w))
            res[name]["spread_s"] = round(max(w) - min(w), 5)
        out["ratios"]["%g" % ratio] = res
        print("ratio %g done" % ratio, file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
