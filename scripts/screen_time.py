"""Time the certified solve (glx.solve_certified, glx_certified_solve) with and without gap-safe
screening: seconds to a relative duality gap of --tol, the two arms alternating in one process.

    PYTHONPATH=convex-optimization_amd python scripts/screen_time.py [--m 8192 --n 16384 --l 32 --dtype f64]

The instance is the demo driver's (glx.driver.gen_data) at the given shape, at mu = ratio * mu_max
for every ratio of --ratios. Both arms share A, b, the step 1 / lambda_max and start from x = 0;
the screened arm also shares the column norms (computed once, as glx.path does; their one launch is
timed separately below). After one pre-warm call per arm (code objects, the allocator), the arms
alternate for --rounds rounds, so both see the same machine state; the spread of an arm over its
rounds is the yardstick for a difference between the arms. Per solve: the wall time of the native
call (it synchronises the stream: what a caller waits for), iterations, compactions and the passes
over A weighted by width. Also: one k_col_norms launch and one compaction (glx_gather_cols of A to
the first compaction's width, on an evenly spread ascending list), with HIP events. Prints one JSON
line.
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
    ap.add_argument("--seed", type=int, default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import glx
    from glx import kernels
    from glx.driver import SEED, gen_data
    from glx.screen import _Prepared

    m, n, l = a.m, a.n, a.l
    _, _, _, _, A, b, _u, _x0, *_ = gen_data(SEED if a.seed is None else a.seed, m, n, l)
    tdt = torch.float64 if a.dtype == "f64" else torch.float32
    Ad, bd = (torch.from_numpy(v).to("cuda", tdt) for v in (A, b))
    del A, b
    mu_top = glx.mu_max(Ad, bd)
    arms = {"screen": _Prepared(Ad, bd, True), "plain": _Prepared(Ad, bd, False)}

    def events(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) * 1e3 / reps, 2)

    out = {"shape": [m, n, l], "dtype": a.dtype, "tol": a.tol, "rounds": a.rounds, "mu_max": mu_top,
           "step": arms["plain"].t, "plan": arms["screen"].solve(mu_top, None, a.tol, 0, 10)[1]["plan"],
           "ratios": {}, "device": torch.cuda.get_device_name(0)}
    first_width = None
    for ratio in (float(v) for v in a.ratios.split(",")):
        mu = ratio * mu_top
        res = {name: {"wall_s": [], "native_s": []} for name in arms}
        for name, prep in arms.items():          # the pre-warm call of each arm
            _, info = prep.solve(mu, None, a.tol, a.maxit, 10)
            res[name].update({k: info[k] for k in ("iterations", "checks", "compactions", "kept_history", "kept",
                                                   "width", "rounds", "passes", "rel_gap", "converged")})
        for _ in range(a.rounds):
            for name, prep in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, info = prep.solve(mu, None, a.tol, a.maxit, 10)
                res[name]["wall_s"].append(round(time.perf_counter() - t0, 5))
                res[name]["native_s"].append(round(info["tt"], 5))
        for name in arms:
            w = res[name]["native_s"]
            res[name]["median_s"] = float(np.median(w))
            res[name]["spread_s"] = round(max(w) - min(w), 5)
        out["ratios"]["%g" % ratio] = res
        hist = res["screen"]["kept_history"]
        if first_width is None and hist:
            first_width = (hist[0] + 63) // 64 * 64

    out["col_norms_us"] = events(lambda: kernels.col_norms(Ad), 20)
    if first_width:
        idx = torch.linspace(0, n - 1, first_width, device="cuda").to(torch.int32)
        dst = torch.empty((m, first_width), dtype=tdt, device="cuda")
        out["compaction"] = {"width": first_width,
                             "gather_us": events(lambda: kernels.gather_cols(Ad, idx, out=dst), 20)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
