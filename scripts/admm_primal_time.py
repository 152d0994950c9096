"""Time the primal ADMM solver (gl_Admm_primal) on the GPU: setup seconds and iterations/s over the
loop, in the direct form (form = 1: the n x n inverse) and the Woodbury form (form = 2: the m x m
inverse and two passes over A).

    PYTHONPATH=convex-optimization_amd python scripts/admm_primal_time.py [--m 8192 --n 16384 --l 32]

The instance is the demo driver's (glx.driver.gen_data, mu = 1e-2) at the given shape, in fp64 with
default options. After one short pre-warm solve per arm (code objects, the Cholesky's workspace),
the two arms alternate in one process for --rounds rounds, so both see the same machine state; the
spread of an arm over its rounds is the yardstick for a difference between the arms. Prints one
JSON line: per arm the k, the fval, the setup seconds and the loop rate k / loop_s of every round.
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
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--maxit", type=int, default=100)
    a = ap.parse_args()

    import torch
    from glx import _lib, admm_primal
    from glx.driver import SEED, gen_data

    _, _, _, mu, A, b, _u, x0, *_ = gen_data(SEED, a.m, a.n, a.l, 1e-2)
    Ad, bd, xd = (torch.from_numpy(v).to("cuda", torch.float64) for v in (A, b, x0))
    arms = {"direct": 1, "woodbury": 2}
    for f in arms.values():
        admm_primal.solve(xd, Ad, bd, mu, {"form": f, "maxit": 3})
    out = {name: {"k": [], "setup_s": [], "it_per_s": [], "fval": []} for name in arms}
    plan = {}
    for _ in range(a.rounds):
        for name, f in arms.items():
            _, k, o = admm_primal.solve(xd, Ad, bd, mu, {"form": f, "maxit": a.maxit})
            g = o["glx"]
            out[name]["k"].append(k)
            out[name]["setup_s"].append(round(g["setup_s"], 6))
            out[name]["it_per_s"].append(round(k / g["loop_s"], 3))
            out[name]["fval"].append(float(o["fval"]))
            plan[name] = g["plan"]
    auto = _lib.admm_primal_describe(_lib.GLX_F64, a.m, a.n, a.l).split(";")[0]
    print(json.dumps({"shape": [a.m, a.n, a.l], "dtype": "f64", "rounds": a.rounds, "arms": out, "auto": auto,
                      "plan": plan, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
