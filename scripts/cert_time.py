"""Time the optimality certificate (glx.certificate, glx_certificate) on the GPU: microseconds per
certificate with its row terms fused into the A^T r epilogue (fused = 1) and behind the plain
product (fused = 2), and the split between the pass over A and the pass over A^T.

    PYTHONPATH=convex-optimization_amd python scripts/cert_time.py [--m 8192 --n 16384 --l 32 --dtype f64]

The instance is the demo driver's (glx.driver.gen_data, mu = 1e-2) at the given shape, x its x0 with
nine rows in ten zeroed. After one pre-warm call per arm (code objects, the allocator), the two
arms alternate in one process for --rounds rounds, so both see the same machine state; the spread
of an arm over its rounds is the yardstick for a difference between the arms. Per round and arm:
--reps calls of glx_certificate on preallocated buffers, timed on the host (the call synchronises
the stream: this is what a caller waits for) and with HIP events around the same calls (device
time). The A^T pass alone is timed with events around glx_certificate_step (form 1: k_atr_cert)
where the plan fuses, around glx_gradient plus the row kernel elsewhere; the A pass is the rest.
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes
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
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=500)
    a = ap.parse_args()

    import numpy as np
    import torch
    from glx import _lib, kernels
    from glx.certificate import compose, workspace
    from glx.driver import SEED, gen_data

    m, n, l = a.m, a.n, a.l
    _, _, _, mu, A, b, _u, x0, *_ = gen_data(SEED, m, n, l, 1e-2)
    x0[np.arange(n) % 10 != 0] = 0
    tdt = torch.float64 if a.dtype == "f64" else torch.float32
    gdt = _lib.GLX_F64 if a.dtype == "f64" else _lib.GLX_F32
    Ad, bd, xd = (torch.from_numpy(v).to("cuda", tdt) for v in (A, b, x0))
    del A, b
    lib = _lib.lib()
    ws = workspace(gdt, m, n, l, Ad.device)
    rec = (ctypes.c_double * 8)()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def cert(fused):
        _lib.check(lib.glx_certificate(gdt, m, n, l, Ad.data_ptr(), xd.data_ptr(), bd.data_ptr(), float(mu),
                                       fused, None, None, rec, ws.data_ptr(), ws.numel(), stream))

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / reps * 1e6
        return round(wall, 2), round(e0.elapsed_time(e1) * 1e3 / reps, 2)

    plan = {f: _lib.certificate_describe(gdt, m, n, l, f) for f in (1, 2)}
    fuses = "rows=fused" in plan[1]
    arms = {"fused": 1, "unfused": 2} if fuses else {"unfused": 2}
    out = {name: {"wall_us": [], "device_us": []} for name in arms}
    figures = {}
    for name, f in arms.items():
        cert(f)
        figures[name] = compose(list(rec), mu)
    for _ in range(a.rounds):
        for name, f in arms.items():
            w, d = timed(lambda: cert(f), a.reps)
            out[name]["wall_us"].append(w)
            out[name]["device_us"].append(d)

    # the A^T pass alone, on r = A x - b
    R, _ = kernels.residual(Ad, xd, bd)
    G = torch.empty((n, l), dtype=tdt, device="cuda")
    sums = torch.zeros(6, dtype=torch.float64, device="cuda")
    if fuses:
        def atr():
            _lib.check(lib.glx_certificate_step(gdt, m, n, l, Ad.data_ptr(), R.data_ptr(), G.data_ptr(),
                                                xd.data_ptr(), float(mu), 1, None, sums.data_ptr(),
                                                ws.data_ptr(), ws.numel(), stream))
        how = "glx_certificate_step form 1 (k_atr_cert)"
    else:
        nb = ctypes.c_size_t(0)
        _lib.check(lib.glx_kernel_workspace_bytes(gdt, m, n, l, ctypes.byref(nb)))
        kws = torch.empty(int(nb.value), dtype=torch.uint8, device="cuda")

        def atr():
            _lib.check(lib.glx_gradient(gdt, m, n, l, Ad.data_ptr(), R.data_ptr(), G.data_ptr(), kws.data_ptr(),
                                        kws.numel(), stream))
            _lib.check(lib.glx_certificate_step(gdt, m, n, l, None, None, G.data_ptr(), xd.data_ptr(),
                                                float(mu), 0, None, sums.data_ptr(), ws.data_ptr(), ws.numel(),
                                                stream))
        how = "glx_gradient + glx_certificate_step form 0"
    atr()
    atr_us = [timed(atr, a.reps)[1] for _ in range(a.rounds)]
    print(json.dumps({"shape": [m, n, l], "dtype": a.dtype, "rounds": a.rounds, "reps": a.reps, "arms": out,
                      "atr_pass_device_us": atr_us, "atr_pass_by": how, "plan": plan,
                      "figures": {k: {q: v[q] for q in ("primal", "gap", "rel_gap", "kkt_max", "scale")}
                                  for k, v in figures.items()},
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
