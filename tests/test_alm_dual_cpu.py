"""CPU-only checks of the dual ALM solver's host surface (no GPU is touched).

* ``tests/alm_dual_ref.py``, the NumPy statement of the restructured iteration (Qn = rho (I + rho
  A^T A)^-1 built once by Woodbury from K, J = rho H, Gram-based spectral norms), reproduces the
  reference's recorded runs: ``k`` exactly, ``f_hist`` and ``fval`` within 1e-9 relative (measured
  <= 2.2e-11, the m > n case; recorded per case in ``alm_dual_index.json``), x within 1e-9 of
  max |x|;
* defaults, option merging, the struct layout, the workspace, every refusal (fp32 among them, in the
  solve, the describe entry and the kernel-level entries alike) and where ``glx_alm_describe`` says
  the inner step is fused.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import alm_dual_ref

with open(os.path.join(GOLDEN, "alm_dual_index.json")) as _fh:
    INDEX = json.load(_fh)
CASES = sorted(INDEX)


def load_case(name):
    """(meta, arrays, A, b, x0, mu): A and x0 redrawn and pinned by hash, b as stored."""
    from glx.driver import gen_data
    meta = INDEX[name]
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        arrs = {k: z[k] for k in z.files}
    _, _, _, mu, A, _b, _u, x0, *_ = gen_data(meta["seed"], meta["m"], meta["n"], meta["l"], meta["mu"])
    for key, arr in (("A", A), ("x0", x0), ("b", arrs["b"])):
        h = hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()
        assert h == meta["sha256"][key], "generator drifted for %s" % key
    return meta, arrs, A, arrs["b"], x0, mu


def test_fixture_set():
    got = sorted((INDEX[c]["m"], INDEX[c]["n"], INDEX[c]["l"], INDEX[c]["opts"].get("rho", 100.0)) for c in CASES)
    want = sorted([(256, 512, 2, 100.0), (64, 128, 16, 100.0), (128, 256, 32, 100.0), (100, 130, 3, 100.0),
                   (192, 128, 16, 100.0), (96, 192, 1, 100.0), (64, 128, 16, 50.0)])
    assert got == want
    for c in CASES:   # "identical k" is a fair demand only away from a tie of the stop rule
        assert INDEX[c]["margin"] >= 5e-3
        assert INDEX[c]["restated_deviation"]["f_hist"] <= 1e-9
        assert os.path.getsize(os.path.join(GOLDEN, c + ".npz")) < 100 * 1024
    assert sorted(INDEX[c]["k"] for c in CASES if not INDEX[c]["opts"]) == sorted([38, 37, 38, 38, 41, 39])


@pytest.mark.parametrize("name", CASES)
def test_restated_iteration_reproduces_reference(name):
    meta, arrs, A, b, x0, mu = load_case(name)
    x, k, out = alm_dual_ref.gl_alm_dual(x0, A, b, mu, dict(meta["opts"]))
    assert k == int(arrs["k"])
    rel = lambda got, want: np.max(np.abs(np.asarray(got) - want) / np.abs(want))
    print("%s: f_hist %.2e, x %.2e, r %.2e, s %.2e" % (
        name, rel(out["f_hist"], arrs["f_hist"]), np.max(np.abs(x - arrs["x"])) / np.max(np.abs(arrs["x"])),
        rel(out["r_norm"], arrs["r_norm"]), rel(out["s_norm"], arrs["s_norm"])))
    # no looser than 1e-9, and within a small factor of what the index recorded on its own machine
    bar = min(1e-9, max(1e-12, 50 * meta["restated_deviation"]["f_hist"]))
    assert rel(out["f_hist"], arrs["f_hist"]) <= bar
    assert rel(out["f_hist_best"], arrs["f_hist_best"]) <= bar
    assert abs(out["fval"] - arrs["fval"]) <= bar * abs(arrs["fval"])
    assert np.max(np.abs(x - arrs["x"])) <= 1e-9 * np.max(np.abs(arrs["x"]))
    # the Gram-based norms of the restructured iteration against the reference's SVD-based ones:
    # more than two orders inside the 5e-3 margin every fixture keeps from thres
    assert rel(out["r_norm"], arrs["r_norm"]) <= 3e-5
    assert rel(out["s_norm"], arrs["s_norm"]) <= 3e-5


def test_restated_options():
    meta, arrs, A, b, x0, mu = load_case("alm_dual_64x128x16")
    given = {"maxit": 3, "unknown": object()}
    before = dict(given)
    x, k, out = alm_dual_ref.gl_alm_dual(x0, A, b, mu, given)
    assert given == before and k == 3 and len(out["f_hist"]) == 3
    assert np.allclose(out["f_hist"], arrs["f_hist"][:3], rtol=1e-9, atol=0)
    x, k, out = alm_dual_ref.gl_alm_dual(x0, A, b, mu, {"maxit": 0})
    assert k == 0 and np.array_equal(x, x0) and out["fval"] == alm_dual_ref.objective(A, b, x0, mu)
    assert alm_dual_ref.gl_alm_dual(x0, A, b, mu, {"max_total_iters": 2})[1] == 2


def test_default_opts_are_the_references():
    from glx import _lib
    o = _lib.alm_default_opts()
    ref = alm_dual_ref.DEFAULT_OPTS   # gl_ALM_dual.py:67-73
    assert (o.maxit, o.converge_len) == (ref["maxit"], ref["converge_len"]) == (100, 20)
    assert o.thres == ref["thres"] == 1e-3
    assert o.rho == ref["rho"] == 1e2
    assert o.tau == ref["tau"] == (1 + 5 ** 0.5) * 0.5
    assert (o.inner_iters, o.inner_step) == (500, 1e-2)   # :53, :57
    assert (o.fused, o.max_total_iters) == (0, 0)


def test_option_merging():
    from glx import alm
    given = {"maxit": 7, "rho": 50.0, "unknown_key": object(), "converge_thres": 1e-5, "fused": 2}
    before = dict(given)
    o = alm.make_opts(given)
    assert given == before                       # the caller's dict is not mutated
    assert (o.maxit, o.rho, o.fused) == (7, 50.0, 2)
    assert (o.converge_len, o.thres, o.inner_iters, o.inner_step) == (20, 1e-3, 500, 1e-2)   # untouched defaults
    o = alm.make_opts({"thres": 1e-4, "tau": 1.0, "converge_len": 3, "max_total_iters": 5, "inner_iters": 50,
                       "inner_step": 5e-3})
    assert (o.thres, o.tau, o.converge_len, o.max_total_iters, o.inner_iters, o.inner_step) == \
        (1e-4, 1.0, 3, 5, 50, 5e-3)


def test_struct_layout_matches_c():
    from glx import _lib
    fields = [f for f, _ in _lib.GlxAlmOpts._fields_]
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "glx.h"
int main(void) {
  printf("%zu", sizeof(glx_alm_opts));
''' + "".join('  printf(" %%zu", offsetof(glx_alm_opts, %s));\n' % f for f in fields) + r'''
  printf("\n");
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        exe = os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib.GlxAlmOpts
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields]


def _describe(dtype, m, n, l, opts=None):
    from glx import _lib
    buf = ctypes.create_string_buffer(2048)
    rc = _lib.lib().glx_alm_describe(dtype, m, n, l, ctypes.byref(opts) if opts is not None else None, buf, len(buf))
    return rc, (buf.value.decode() if rc == 0 else _lib.lib().glx_last_error().decode())


def _ws_bytes(dtype, m, n, l, opts=None):
    from glx import _lib
    nb = ctypes.c_size_t(0)
    rc = _lib.lib().glx_alm_workspace_bytes(dtype, m, n, l, ctypes.byref(opts) if opts is not None else None,
                                            ctypes.byref(nb))
    return rc, int(nb.value)


def test_describe_says_fused_exactly_where_the_plan_fuses():
    """l in {16, 32} and n a multiple of the 64-column panel."""
    from glx import _lib
    for l in (1, 2, 3, 8, 15, 16, 17, 31, 32):
        for n in (64, 67, 128, 130, 192, 256, 500, 512, 1024, 2048, 8192, 16384):
            rc, d = _describe(_lib.GLX_F64, 64, n, l)
            assert rc == 0, d
            assert ("inner step=fused" in d) == (l in (16, 32) and n % 64 == 0), (n, l, d)
            for field in ("K v=", "A u=", "A [x|u]=", "A^T z=", "Qn y="):
                assert field in d
    o = _lib.alm_default_opts()
    o.fused = 2
    d = _describe(_lib.GLX_F64, 64, 128, 16, o)[1]
    assert "inner step=row kernel (k_alm_inner_panel" in d
    o.fused = 1
    assert "inner step=fused (k_atr_alm" in _describe(_lib.GLX_F64, 64, 128, 16, o)[1]
    assert "inner step=row kernel (k_alm_inner)" in _describe(_lib.GLX_F64, 100, 130, 3, o)[1]


def test_workspace_grows_with_each_dimension():
    from glx import _lib
    rc, base = _ws_bytes(_lib.GLX_F64, 128, 256, 16)
    assert rc == 0 and base > 0
    for shape in ((256, 256, 16), (128, 512, 16), (128, 256, 32)):
        rc, nb = _ws_bytes(_lib.GLX_F64, *shape)
        assert rc == 0 and nb > base, shape
    assert _ws_bytes(_lib.GLX_F64, 128, 256, 0)[0] == 1      # GLX_E_INVALID
    assert _ws_bytes(_lib.GLX_F64, 128, 256, 33)[0] == 1
    assert _ws_bytes(7, 128, 256, 16)[0] == 1


def _solve_rc(m=64, n=128, l=16, dtype=None, comm=None, A=0x10000, K=0x1000, Qn=0x2000, ws=0x100000,
              ws_bytes=None, opts=None):
    """glx_alm_dual_solve on made-up (never dereferenced) device addresses: every refusal below is
    decided on the host before the first HIP call."""
    from glx import _lib
    dtype = _lib.GLX_F64 if dtype is None else dtype
    o = opts if opts is not None else _lib.alm_default_opts()
    if ws_bytes is None:
        ws_bytes = _ws_bytes(_lib.GLX_F64, m, n, min(max(l, 1), 32))[1]
    p = _lib.GlxProblem(dtype=dtype, method=0, m=m, n=n, l=l, A=A, b=0x20000, x=0x30000, mu0=1e-2, comm=comm)
    res = _lib.GlxResult()
    rc = _lib.lib().glx_alm_dual_solve(ctypes.byref(p), K, Qn, ctypes.byref(o), ws, ws_bytes, ctypes.byref(res), None)
    return rc, _lib.lib().glx_last_error().decode()


def test_refusals_are_invalid():
    from glx import _lib
    rc, msg = _solve_rc(comm=0x4000)
    assert rc == 1 and "comm" in msg
    assert _solve_rc(l=0)[0] == 1
    rc, msg = _solve_rc(l=33)
    assert rc == 1 and "32" in msg
    for kw in ({"K": None}, {"Qn": None}, {"A": None}):
        rc, msg = _solve_rc(**kw)
        assert rc == 1 and "null" in msg, kw
    for kw in ({"A": 0x10008}, {"K": 0x1004}, {"Qn": 0x2008}):
        rc, msg = _solve_rc(**kw)
        assert rc == 1 and "aligned" in msg, kw
    assert _solve_rc(ws=None)[0] == 1
    rc, msg = _solve_rc(ws_bytes=4096)
    assert rc == 1 and "workspace" in msg
    for field, bad in (("rho", 0.0), ("rho", -1.0), ("inner_iters", 0), ("inner_iters", -3), ("fused", 3),
                       ("fused", -1), ("maxit", -1)):
        o = _lib.alm_default_opts()
        setattr(o, field, bad)
        assert _solve_rc(opts=o)[0] == 1, (field, bad)
        assert _describe(_lib.GLX_F64, 64, 128, 16, o)[0] == 1, (field, bad)
        assert _ws_bytes(_lib.GLX_F64, 64, 128, 16, o)[0] == 1, (field, bad)


def test_fp32_is_refused_everywhere():
    """The solve, the describe entry, the workspace and the kernel-level entries alike, naming the
    conditioning, before any setup is spent."""
    from glx import _lib, alm
    F32 = _lib.GLX_F32
    h = _lib.lib()
    rc, msg = _solve_rc(dtype=F32)
    assert rc == 1 and "condition" in msg and "fp64" in msg
    rc, msg = _describe(F32, 64, 128, 16)
    assert rc == 1 and "condition" in msg
    assert _ws_bytes(F32, 64, 128, 16)[0] == 1
    nb = ctypes.c_size_t(0)
    assert h.glx_alm_inner_workspace_bytes(F32, 128, 16, ctypes.byref(nb)) == 1
    assert "condition" in h.glx_last_error().decode()
    assert h.glx_alm_inner_workspace_bytes(_lib.GLX_F64, 128, 16, ctypes.byref(nb)) == 0 and nb.value > 0
    a = 0x1000
    assert h.glx_alm_inner_step(F32, 128, 16, a, a, 1, a, a, a, 1.0, 0.5, 1e-2, 1e-2, 0, a, a, a, nb.value, None) == 1
    assert "condition" in h.glx_last_error().decode()
    assert h.glx_alm_inner_run(F32, 128, 16, a, a, 5, 1e-2, 1e-2, 0, a, a, nb.value, None) == 1
    assert "condition" in h.glx_last_error().decode()
    # the kernel-level entries' other refusals, on the host too
    F64 = _lib.GLX_F64
    assert h.glx_alm_inner_step(F64, 130, 3, a, None, 1, a, a, a, 1.0, 0.5, 1e-2, 1e-2, 1, a, 0x2000, 0x10000,
                                nb.value, None) == 1                      # form 1 where the plan takes none
    assert "fused" in h.glx_last_error().decode()
    assert h.glx_alm_inner_step(F64, 128, 16, a, a, 1, a, a, a, 1.0, 0.5, 1e-2, 1e-2, 0, a, a, 0x10000,
                                nb.value, None) == 1                      # y_out == y
    assert h.glx_alm_inner_step(F64, 128, 33, a, a, 1, a, a, a, 1.0, 0.5, 1e-2, 1e-2, 0, a, 0x2000, 0x10000,
                                nb.value, None) == 1
    assert h.glx_alm_inner_run(F64, 128, 16, a, a, 0, 1e-2, 1e-2, 0, a, 0x10000, nb.value, None) == 1
    assert h.glx_alm_inner_run(F64, 128, 16, a, a, 5, 1e-2, 1e-2, 0, a, 0x10000, 64, None) == 1
    # the Python layer raises before it touches a device or spends the setup
    with pytest.raises(_lib.GlxError, match="condition"):
        alm.solve(np.zeros((128, 16), np.float32), np.zeros((64, 128), np.float32),
                  np.zeros((64, 16), np.float32), 1e-2, {})


def test_driver_registry_is_unchanged():
    from glx import _lib
    assert "gl_ALM_dual" not in _lib.METHODS and len(_lib.METHODS) == 5
    assert _lib.lib().glx_abi_version() == 2


def test_drop_in_module_exports_the_references_name():
    import gl_ALM_dual
    import inspect
    assert list(inspect.signature(gl_ALM_dual.gl_Alm_dual).parameters) == ["x0", "A", "b", "mu", "opts"]
