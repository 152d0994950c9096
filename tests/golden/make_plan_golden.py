"""Record what the launch planner decides as fixtures: tests/golden/plan_golden.json (host-only)
and tests/golden/plan_sessions.json (needs the GPU: it creates sessions, it does not run them).

The fixtures pin the planner of the commit BEFORE the tile-table refactor, so they are recorded
from a build of that commit and never from the refactored code: check that commit out, build it,
copy this script into its tests/golden/ and run

    python tests/golden/make_plan_golden.py              # plan_golden.json
    python tests/golden/make_plan_golden.py --sessions   # plan_sessions.json (on the GPU)

tests/test_host_cpu.py::test_plan_matches_recorded_planner replays plan_golden.json and
tests/test_gpu_kernels.py::test_session_plan_matches_recorded_planner replays plan_sessions.json;
both require identical strings, byte counts and error codes.

plan_golden.json: {"cases": [[dtype, m, n, l, env, describe, kernel_ws, [ws_proxgd, ws_fproxgd],
ws_variant_arg], ...]} where describe / kernel_ws / ws_* are the value, or {"rc": code} where the
library returns an error; ws_variant_arg is [ws_proxgd, ws_fproxgd] with opts.ax_variant = the
code of env["GLX_AX_VARIANT"] and no environment override (null for the other cases:
glx_plan_describe and glx_kernel_workspace_bytes take no variant argument).
"""
from __future__ import annotations

import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

SHAPES = [(8192, 16384, 32), (4096, 8192, 16), (65536, 8192, 1),                     # NS, C2, C4
          (1024, 16384, 32), (2048, 16384, 32), (4096, 16384, 32), (16384, 16384, 32),  # shards
          (1024, 8224, 32), (8192, 16400, 32), (8192, 16416, 32), (1000, 1000, 32), (301, 517, 3),
          (333, 250, 17), (129, 640, 32), (129, 64, 16), (64, 128, 32), (192, 4096, 16),
          (777, 640, 8), (2048, 256, 1), (8, 16, 16),
          (131072, 16384, 32)]                                                        # host-only
SHORT = [(8192, 16384, 32), (4096, 8192, 16), (1024, 16384, 32), (1024, 8224, 32)]
AX_CODES = [0, 1, 2, 3, 1820, 21820, 21410, 1420, 1220, 52224, 52228, 51328, 52324, 92278, 92268, 92478]
AXB_CODES = [c for c in AX_CODES if c >= 1000]
ATR_CODES = [3, 8, 108, 1008, 1114, 1028, 38, 1038, 1048, 7777]   # 1048: not built; 7777: nonsense
KNOBS = [{"GLX_AX_DMA": "0"}, {"GLX_AX_DMA32": "0"}, {"GLX_SHARD_TILE": "0"}, {"GLX_AXL_BLOCKS": "128"},
         {"GLX_AX_S": "3"}, {"GLX_AXB_S": "5"}, {"GLX_ATR_S": "2"}]
OVERRIDES = ([{"GLX_AX_VARIANT": str(c)} for c in AX_CODES] + [{"GLX_AXB_VARIANT": str(c)} for c in AXB_CODES] +
             [{"GLX_ATR_VARIANT": str(c)} for c in ATR_CODES] + KNOBS)
PLANNER_ENV = ["GLX_AX_VARIANT", "GLX_AXB_VARIANT", "GLX_ATR_VARIANT", "GLX_AX_S", "GLX_AXB_S", "GLX_ATR_S",
               "GLX_AXL_BLOCKS", "GLX_AX_DMA", "GLX_AX_DMA32", "GLX_SHARD_TILE", "GLX_AX_XCD", "GLX_AX_ROT",
               "GLX_ATR_NARROW", "GLX_ATR_FUSE_SPLIT", "GLX_FUSED_TRIAL"]

# (solver, dtype name, m, n, l, env): the smallest shapes at which each method-level A^T R choice
# of a session fires, and the overrides that switch it off
SESSIONS = [(s, dt, m, n, l, env)
            for (dt, m, n, l, env) in [("float32", 128, 1024, 16, {}), ("float32", 128, 16384, 16, {}),
                                       ("float64", 128, 8192, 16, {}), ("float64", 128, 4096, 16, {}),
                                       ("float64", 128, 8192, 16, {"GLX_ATR_NARROW": "0"}),
                                       ("float32", 128, 1024, 16, {"GLX_ATR_S": "2"})]
            for s in ("gl_ProxGD_primal", "gl_FProxGD_primal")]


def set_env(env):
    for k in PLANNER_ENV:
        os.environ.pop(k, None)
    os.environ.update(env)


def _value(rc, v):
    return v if rc == 0 else {"rc": rc}


def record_case(dtype, m, n, l, env):
    """One row of plan_golden.json, from the library this tree has built."""
    from glx import _lib
    from glx.solver import make_opts
    h = _lib.lib()

    def session_ws(variant):
        out = []
        for meth in (_lib.GLX_PROXGD, _lib.GLX_FPROXGD):
            p = _lib.GlxProblem(dtype=dtype, method=meth, m=m, n=n, l=l, A=256, b=256, x=256, mu0=0.01)
            o = make_opts(meth, {})
            o.ax_variant = variant
            nb = ctypes.c_size_t(0)
            rc = h.glx_workspace_bytes(ctypes.byref(p), ctypes.byref(o), ctypes.byref(nb))
            out.append(_value(rc, nb.value))
        return out

    set_env(env)
    try:
        buf = ctypes.create_string_buffer(512)
        rc = h.glx_plan_describe(dtype, m, n, l, buf, len(buf))
        desc = _value(rc, buf.value.decode())
        nb = ctypes.c_size_t(0)
        rc = h.glx_kernel_workspace_bytes(dtype, m, n, l, ctypes.byref(nb))
        kws = _value(rc, nb.value)
        ws = session_ws(0)
        ws_arg = None
        if "GLX_AX_VARIANT" in env:
            set_env({})
            ws_arg = session_ws(int(env["GLX_AX_VARIANT"]))
    finally:
        set_env({})
    return [dtype, m, n, l, env, desc, kws, ws, ws_arg]


def record_session(solver, dtname, m, n, l, env):
    import torch
    from glx.solver import Session
    dt = getattr(torch, dtname)
    set_env(env)
    try:
        A = torch.zeros((m, n), dtype=dt, device="cuda")
        b = torch.zeros((m, l), dtype=dt, device="cuda")
        x = torch.zeros((n, l), dtype=dt, device="cuda")
        s = Session(solver, x, A, b, 1e-2, {})
        d = s.describe()
        s.close()
    finally:
        set_env({})
    return d


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "convex-optimization_amd"))
    if "--sessions" in sys.argv[1:]:
        rows = [[s, dt, m, n, l, env, record_session(s, dt, m, n, l, env)] for (s, dt, m, n, l, env) in SESSIONS]
        path = os.path.join(HERE, "plan_sessions.json")
        with open(path, "w") as fh:
            fh.write('{"sessions": [\n' + ",\n".join(json.dumps(r) for r in rows) + "\n]}\n")
    else:
        rows = [record_case(dt, m, n, l, {}) for dt in (0, 1) for (m, n, l) in SHAPES]
        rows += [record_case(dt, m, n, l, env) for env in OVERRIDES for dt in (0, 1) for (m, n, l) in SHORT]
        path = os.path.join(HERE, "plan_golden.json")
        with open(path, "w") as fh:
            fh.write('{"cases": [\n' + ",\n".join(json.dumps(r) for r in rows) + "\n]}\n")
    print(path, len(rows))


if __name__ == "__main__":
    main()
