"""Record what a session's mode resolves to as fixtures: tests/golden/mode_golden.json.

The fixture pins the session mode of the commit BEFORE csrc/session_mode.cpp existed (the
decisions then lived in Session<T>'s constructor, carve and a dozen free functions of solver.cpp),
so it is recorded from a build of that commit and never from the refactored code: check that
commit out, build it, copy this script (and make_plan_golden.py, whose shapes it uses) into its
tests/golden/ and run

    python tests/golden/make_mode_golden.py          # part A ("cases"), host only
    python tests/golden/make_mode_golden.py --gpu    # parts B ("sessions") and C ("runs"), on the GPU

Each call rewrites its own parts of the file and keeps the others (--out PATH: write there).

Part A, "cases": [method, dtype, m, n, l, opts, env, comm, ws, differs] with comm = null or
[nranks, rank] of a host-transport communicator (glx_comm_create_host: no device), ws =
glx_workspace_bytes or {"rc": code}. differs = 1 marks the rows of the one deliberate difference:
ProxGD's "row-sharded ProxGD needs n % ranks == 0 ..." error, which that commit raises from
glx_session_create only (its glx_workspace_bytes, recorded here, still answers); the refactored
glx_workspace_bytes raises it too, with the code and text part B recorded from glx_session_create.

Part B, "sessions": {"name", "solver", "dtype", "m", "n", "l", "opts", "env", "comm", "describe"}:
Session.describe() of a session on zero tensors that is created and never run, or {"rc", "msg"}
where creation fails. comm = 1: a host-transport communicator of world size 1.

Part C, "runs": the part B sessions whose A is under 16 MiB plus three whose knob does not show
in describe(), on seeded data: {"name", ..., "f_hist": [float.hex], "counters": {...}, "skip": [...]}
after run(30) and finish(). The part is recorded twice in the same process; f_hist must repeat bit
for bit (the script stops otherwise: pick another seed or shape), a counter that does not repeat
is listed in "skip" (allowed only with dc_window > 0 in the describe string).

tests/test_host_cpu.py::test_mode_matches_recorded_sessions replays part A and resolves part B's
strings on the host (glx_mode_describe); tests/test_gpu_kernels.py::
test_session_mode_matches_recorded_sessions replays parts B and C on the GPU.
"""
from __future__ import annotations

import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
try:
    import make_plan_golden as plan_gen
finally:
    sys.path.pop(0)

FIXTURE = os.path.join(HERE, "mode_golden.json")
SEED = 20261019
STEPS = 30

# every variable of SessionKnobs: (off value, one non-default value)
KNOBS = {"GLX_DC_BATCH": ("0", "4"), "GLX_SHARD_ROWS": ("2", "1"), "GLX_SPLIT_F32": ("0", "1"),
         "GLX_SPLIT_CAND": ("0", "1"), "GLX_SPLIT_FISTA": ("0", "1"), "GLX_SPLIT_NNZ": ("0", "0.01"),
         "GLX_AE_FUSED": ("0", "1"), "GLX_AE_HYB_ROWS": ("0", "100"), "GLX_GEMV_FUSED": ("0", "1"),
         "GLX_UNFUSED_SPEC": ("0", "1"), "GLX_FUSED_TRIAL": ("0", "1"), "GLX_READBACK": ("sync", "spin"),
         "GLX_ATTACH_PUB": ("0", "1"), "GLX_SPEC_GRAD": ("0", "1"), "GLX_SPEC_AX_PUB": ("0", "1"),
         "GLX_SHARD_DERIVE": ("0", "1"), "GLX_DEFER_RED": ("0", "1"), "GLX_AX_KEEP_MIB": ("0", "64"),
         "GLX_ATR_KEEP_MIB": ("0", "64")}
MODE_ENV = sorted(set(KNOBS) | set(plan_gen.PLANNER_ENV) | {"GLX_GATHER"})
KNOB_ENVS = [{k: v} for k, vals in KNOBS.items() for v in vals]

OPTION_SETS = [{}, {"exact_objective": 1}, {"step_type": "fixed"}, {"split_cand": 1}, {"split_cand": 2},
               {"dc_window": 4}, {"dc_window": -1}, {"shard_rows": 1}, {"shard_rows": 2}, {"shard_model": 8}]
COMMS = [[1, 0], [2, 1], [8, 3], [3, 1]]   # (3, 1): n % ranks != 0 occurs
PROX, FPROX, SGD = 0, 1, 2
NS, C1, SHARD = (8192, 16384, 32), (512, 1024, 2), (1024, 16384, 32)


def cases():
    """Part A's grid: (method, dtype, m, n, l, opts, env, comm)."""
    out = [(meth, dt, m, n, l, {}, {}, None) for meth in range(5) for dt in (0, 1) for (m, n, l) in plan_gen.SHAPES]
    out += [(meth, dt, m, n, l, o, {}, None) for o in OPTION_SETS[1:] for meth in (PROX, FPROX, SGD)
            for dt in (0, 1) for (m, n, l) in plan_gen.SHORT]
    out += [(meth, dt, m, n, l, {}, env, None) for env in KNOB_ENVS
            for (meth, dt) in ((PROX, 1), (FPROX, 1), (FPROX, 0)) for (m, n, l) in (NS, C1)]
    out += [(SGD, dt, 2048, 256, 1, {}, {"GLX_GEMV_FUSED": v}, None) for dt in (0, 1) for v in KNOBS["GLX_GEMV_FUSED"]]
    out += [(meth, dt, m, n, l, o, {}, c) for c in COMMS for o in OPTION_SETS if o != {"split_cand": 2}
            for meth in (PROX, FPROX) for dt in (0, 1)
            for (m, n, l) in (SHARD, NS, (128, 4100, 32), (4096, 8192, 16))]
    out += [(meth, 1, *SHARD, o, env, c) for env in KNOB_ENVS for meth in (PROX, FPROX)
            for (o, c) in (({}, [1, 0]), ({}, [2, 1]), ({"shard_model": 8}, [1, 0]))]
    return out


def differs(meth, opts, env, comm, n):
    """The rows of the one deliberate difference (module docstring): ProxGD with a communicator,
    row sharding asked for (shard_rows = 1), more than one (modelled) rank, and n that does not
    divide by them. No row of the grid combines that with a device-control window."""
    if meth != PROX or comm is None:
        return 0
    want = int(env.get("GLX_SHARD_ROWS", opts.get("shard_rows", 0)))
    ranks = comm[0] if comm[0] > 1 else max(1, opts.get("shard_model", 0))
    assert not (want == 1 and (opts.get("dc_window", 0) > 0 or "GLX_DC_BATCH" in env))
    return int(want == 1 and ranks > 1 and (ranks > 64 or n % ranks != 0))


def set_env(env):
    for k in MODE_ENV:
        os.environ.pop(k, None)
    os.environ.update(env)


_comms = {}
_IDENTITY = None


def host_comm(nranks, rank):
    """A host-transport communicator (created once per (nranks, rank), kept for the process); its
    all-reduce callback leaves the buffer as it is, which is the sum over one rank."""
    global _IDENTITY
    from glx import _lib
    if _IDENTITY is None:
        _IDENTITY = _lib.HOST_ALLREDUCE_FN(lambda buf, count, dtype, user: 0)
    if (nranks, rank) not in _comms:
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().glx_comm_create_host(ctypes.byref(h), nranks, rank,
                                                   ctypes.cast(_IDENTITY, ctypes.c_void_p), None))
        _comms[(nranks, rank)] = h
    return _comms[(nranks, rank)]


class _Comm:   # what glx.solver.Session takes as comm
    def __init__(self, handle):
        self.handle = handle


def problem(meth, dtype, m, n, l, opts, comm):
    """(GlxProblem on dummy aligned pointers, GlxOpts) of a case."""
    from glx import _lib
    from glx.solver import make_opts
    p = _lib.GlxProblem(dtype=dtype, method=meth, m=m, n=n, l=l, A=256, b=256, x=256, mu0=0.01,
                        comm=host_comm(*comm) if comm else None)
    return p, make_opts(meth, opts)


def record_case(meth, dtype, m, n, l, opts, env, comm):
    """One row of part A, from the library this tree has built."""
    from glx import _lib
    set_env(env)
    try:
        p, o = problem(meth, dtype, m, n, l, opts, comm)
        nb = ctypes.c_size_t(0)
        rc = _lib.lib().glx_workspace_bytes(ctypes.byref(p), ctypes.byref(o), ctypes.byref(nb))
        msg = _lib.lib().glx_last_error().decode() if rc else ""
    finally:
        set_env({})
    return [meth, dtype, m, n, l, opts, env, comm, nb.value if rc == 0 else {"rc": rc}, differs(meth, opts, env, comm, n)], msg


def hybrid_shape():
    """The smallest f64 l = 32 shape (n = 16384, m in steps of 64) whose one-source tile is the
    LDS-DMA tile the hybrid A e needs; NS where none is smaller."""
    from glx import _lib
    set_env({})
    for m in range(64, NS[0], 64):
        if "ax1=k_ax_dma" in _lib.plan_describe(_lib.GLX_F64, m, NS[1], 32):
            return (m, NS[1], 32)
    return NS


def sessions():
    """Part B: the smallest shape at which each branch of the mode fires."""
    P, F, S = "gl_ProxGD_primal", "gl_FProxGD_primal", "gl_SGD_primal"
    rows = []

    def add(name, solver, dt, shape, opts=None, env=None, comm=0):
        rows.append({"name": name, "solver": solver, "dtype": dt, "m": shape[0], "n": shape[1], "l": shape[2],
                     "opts": opts or {}, "env": env or {}, "comm": comm})

    for i, (s, dt, m, n, l, env) in enumerate(plan_gen.SESSIONS):
        add("fused%d" % i, s, dt, (m, n, l), env=env)
    add("unfused", P, "float64", C1)
    add("unfused_off", P, "float64", C1, env={"GLX_UNFUSED_SPEC": "0"})
    add("unfused_dc0", P, "float64", C1, env={"GLX_DC_BATCH": "0"})
    sp = (256, 2048, 32)
    add("split_bm", P, "float64", sp, env={"GLX_SPLIT_CAND": "1"})
    add("split_rows", P, "float64", sp, env={"GLX_SPLIT_CAND": "1", "GLX_GATHER": "rows"})
    add("split_lists", P, "float64", sp, env={"GLX_SPLIT_CAND": "1", "GLX_GATHER": "lists"})
    add("fsplit", F, "float64", sp, env={"GLX_SPLIT_CAND": "1"})
    add("fsplit_odd_m", F, "float64", (200, 2048, 32), env={"GLX_SPLIT_CAND": "1"})   # gather_rows_ok fails
    add("fsplit_off", F, "float64", sp, env={"GLX_SPLIT_CAND": "1", "GLX_SPLIT_FISTA": "0"})
    add("fsplit_f32", F, "float32", sp, env={"GLX_SPLIT_CAND": "1", "GLX_SPLIT_F32": "1"})
    add("fsplit_f32_off", F, "float32", sp, env={"GLX_SPLIT_CAND": "1"})
    hyb = hybrid_shape()
    add("hyb", P, "float64", hyb)
    add("hyb_off", P, "float64", hyb, env={"GLX_AE_HYB_ROWS": "0"})
    add("hyb_100", P, "float64", hyb, env={"GLX_AE_HYB_ROWS": "100"})
    add("egat", P, "float64", hyb, env={"GLX_AE_FUSED": "1"})
    for s, tag in ((P, "p"), (F, "f")):
        add("comm_" + tag, s, "float64", SHARD, comm=1)
        add("comm_model_" + tag, s, "float64", SHARD, opts={"shard_model": 8}, comm=1)
        add("comm_model_noderive_" + tag, s, "float64", SHARD, opts={"shard_model": 8},
            env={"GLX_SHARD_DERIVE": "0"}, comm=1)
        add("comm_off_" + tag, s, "float64", SHARD, opts={"shard_rows": 2}, comm=1)
        add("comm_dc_" + tag, s, "float64", SHARD, opts={"dc_window": 4}, comm=1)
        add("comm_misfit_" + tag, s, "float64", (128, 4100, 32), opts={"shard_rows": 1, "shard_model": 8}, comm=1)
    one = (128, 4096, 16)
    add("readback_sync", P, "float64", one, env={"GLX_READBACK": "sync"})
    add("attach_off", P, "float64", one, env={"GLX_ATTACH_PUB": "0"})
    add("fused_off", P, "float64", one, env={"GLX_FUSED_TRIAL": "0"})
    add("defer_off", P, "float64", one, env={"GLX_DEFER_RED": "0"})
    add("dc4", P, "float64", one, opts={"dc_window": 4})
    add("sgd", S, "float64", (2048, 256, 1))
    add("sgd_two_pass", S, "float64", (2048, 256, 1), env={"GLX_GEMV_FUSED": "0"})
    return rows


def run_only():
    """Part C's extra sessions: mode fields that describe() does not show."""
    base = {"solver": "gl_ProxGD_primal", "dtype": "float64", "m": 128, "n": 4096, "l": 16, "opts": {}, "comm": 0}
    return [dict(base, name="spec_grad_off", env={"GLX_SPEC_GRAD": "0"}),
            dict(base, name="spec_ax_pub_off", env={"GLX_SPEC_AX_PUB": "0"}),
            dict(base, name="split_nnz", env={"GLX_SPLIT_NNZ": "0.01"})]


def small(row):
    return row["m"] * row["n"] * (8 if row["dtype"] == "float64" else 4) < 16 * 2**20


def open_session(row, seeded):
    """Session of a part B / C row (the environment must already be set); raises GlxError."""
    import torch
    from glx.solver import Session
    dt = getattr(torch, row["dtype"])
    m, n, l = row["m"], row["n"], row["l"]
    if seeded:
        g = torch.Generator(device="cuda").manual_seed(SEED)
        # ||A||^2 ~ 700, so that the methods' default steps (1e-3, 2e-3) sit on either side of 1 / L:
        # the line searches accept some trials and reject others
        A = torch.randn((m, n), dtype=torch.float64, device="cuda", generator=g)
        A = (A * (700.0 ** 0.5 / (m ** 0.5 + n ** 0.5))).to(dt)
        b = torch.randn((m, l), dtype=torch.float64, device="cuda", generator=g).to(dt)
        x = (0.1 * torch.randn((n, l), dtype=torch.float64, device="cuda", generator=g)).to(dt)
    else:
        A, b, x = (torch.zeros(s, dtype=dt, device="cuda") for s in ((m, n), (m, l), (n, l)))
    comm = _Comm(host_comm(1, 0)) if row["comm"] else None
    return Session(row["solver"], x, A, b, 1e-2, dict(row["opts"]), comm=comm)


def record_session(row):
    """describe() of the session created and never run, or {"rc", "msg"}."""
    from glx import _lib
    set_env(row["env"])
    try:
        s = open_session(row, seeded=False)
        d = s.describe()
        s.close()
    except _lib.GlxError as e:
        d = {"rc": e.code, "msg": str(e).split(": ", 1)[1]}
    finally:
        set_env({})
    return d


def record_run(row):
    """(describe, f_hist as float.hex, counters with record_waits) after run(STEPS) and finish()."""
    set_env(row["env"])
    try:
        s = open_session(row, seeded=True)
        d = s.describe()
        s.run(STEPS)
        res = s.finish()
        cnt = dict(s.counters(), record_waits=res["record_waits"])
        s.close()
    finally:
        set_env({})
    return d, [float(v).hex() for v in res["f_hist"]], cnt


def mode_describe(row):
    """What the host-only entry resolves for a part B row: the string, or {"rc", "msg"}."""
    from glx import _lib
    set_env(row["env"])
    try:
        p, o = problem(_lib.METHODS[row["solver"]], _lib.GLX_F64 if row["dtype"] == "float64" else _lib.GLX_F32,
                       row["m"], row["n"], row["l"], row["opts"], [1, 0] if row["comm"] else None)
        try:
            return _lib.mode_describe(p, o)
        except _lib.GlxError as e:
            return {"rc": e.code, "msg": str(e).split(": ", 1)[1]}
    finally:
        set_env({})


def write(parts, path):
    keys = ("cases", "sessions", "runs")
    body = ",\n".join('"%s": [\n%s\n]' % (k, ",\n".join(json.dumps(r) for r in parts.get(k, []))) for k in keys)
    with open(path, "w") as fh:
        fh.write("{" + body + "}\n")


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "convex-optimization_amd"))
    args = sys.argv[1:]
    out = args[args.index("--out") + 1] if "--out" in args else FIXTURE
    parts = json.load(open(FIXTURE)) if os.path.exists(FIXTURE) else {}
    if "--gpu" in args:
        parts["sessions"] = [dict(r, describe=record_session(r)) for r in sessions()]
        for r in parts["sessions"]:
            print(r["name"], r["describe"], flush=True)
        runs = []
        for r in [r for r in sessions() if small(r)] + run_only():
            if isinstance(record_session(r), dict):
                continue   # creation fails: nothing to run
            d, fh, cnt = record_run(r)
            d2, fh2, cnt2 = record_run(r)
            if fh != fh2 or d != d2:
                raise SystemExit("%s: f_hist does not repeat; choose another seed or shape" % r["name"])
            skip = sorted(k for k in cnt if cnt[k] != cnt2[k])
            if skip and "dc_window=0" in d:
                raise SystemExit("%s: counters %s do not repeat without a device-control window" % (r["name"], skip))
            runs.append(dict(r, describe=d, f_hist=fh, counters=cnt, skip=skip))
            print(r["name"], fh[-1], cnt, skip, flush=True)
        parts["runs"] = runs
    else:
        parts["cases"] = [record_case(*c)[0] for c in cases()]
    write(parts, out)
    print(out, {k: len(v) for k, v in parts.items()})


if __name__ == "__main__":
    main()
