"""Time the dual ALM solver (gl_Alm_dual) on the GPU: setup seconds, outer iterations/s and inner
steps/s over the loop, with the inner step fused into Qn y (fused = 1) and as its own kernel
(fused = 2), at (512, 1024, 2), the reference report's own shape (l = 2 takes the generic arm
whatever ``fused`` says), and at one l = 32 shape, (2048, 4096, 32) by default.

    PYTHONPATH=convex-optimization_amd python scripts/alm_time.py [--m 2048 --n 4096 --l 32]

The instances are the demo driver's (glx.driver.gen_data, mu = 1e-2). After one short pre-warm
solve per arm (code objects, the Cholesky's workspace), the two arms alternate in one process for
--rounds rounds, so both see the same machine state; the spread of an arm over its
rounds is the yardstick for a difference between the arms. Prints one JSON line per shape: per arm
the k, the setup seconds, the whole-call seconds and the loop rates of every round.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "convex-optimization_amd"))


def time_shape(m: int, n: int, l: int, rounds: int, maxit: int) -> None:
    import torch
    from glx import alm
    from glx.driver import SEED, gen_data

    _, _, _, mu, A, b, _u, x0, *_ = gen_data(SEED, m, n, l, 1e-2)
    Ad, bd, xd = (torch.from_numpy(v).to("cuda", torch.float64) for v in (A, b, x0))
    arms = {"fused": 1, "row_kernel": 2}
    for f in arms.values():
        alm.solve(xd, Ad, bd, mu, {"fused": f, "maxit": 2})
    out = {name: {"k": [], "setup_s": [], "tt": [], "outer_per_s": [], "inner_per_s": [], "fval": []} for name in arms}
    plan = {}
    for _ in range(rounds):
        for name, f in arms.items():
            _, k, o = alm.solve(xd, Ad, bd, mu, {"fused": f, "maxit": maxit})
            g = o["glx"]
            loop = o["tt"] - g["setup_s"]
            out[name]["k"].append(k)
            out[name]["setup_s"].append(round(g["setup_s"], 6))
            out[name]["tt"].append(round(o["tt"], 6))
            out[name]["outer_per_s"].append(round(k / loop, 3))
            out[name]["inner_per_s"].append(round(g["inner_steps"] / loop, 1))
            out[name]["fval"].append(float(o["fval"]))
            plan[name] = g["plan"]
    print(json.dumps({"shape": [m, n, l], "rounds": rounds, "arms": out,
                      "fused_ran": {nm: "inner step=fused" in p for nm, p in plan.items()},
                      "plan": plan["fused"], "device": torch.cuda.get_device_name(0)}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=2048)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--l", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--maxit", type=int, default=100)
    a = ap.parse_args()
    time_shape(512, 1024, 2, a.rounds, a.maxit)
    time_shape(a.m, a.n, a.l, a.rounds, a.maxit)


if __name__ == "__main__":
    main()
