"""CPU-only checks of the dual ADMM solver's host surface (no GPU is touched).

* ``tests/admm_ref.py``, the NumPy statement of the restructured iteration (explicit inverse,
  batched products, Gram-based spectral norms), reproduces the reference's recorded runs;
* ``glx_sym_lambda_max`` (the host Jacobi sweep of the stop rule) against ``numpy.linalg.eigvalsh``;
* defaults, option merging, the struct layout, the workspace's growth, the refusals and
  ``glx_admm_describe``.
"""
import ctypes
import json
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import admm_ref

with open(os.path.join(GOLDEN, "admm_index.json")) as _fh:
    INDEX = json.load(_fh)
CASES = sorted(INDEX)


def load_case(name):
    """(meta, arrays, A, b, x0, mu): A and x0 redrawn and pinned by hash, b as stored."""
    import hashlib
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
    shapes = {(INDEX[c]["m"], INDEX[c]["n"], INDEX[c]["l"]) for c in CASES}
    assert shapes == {(256, 512, 2), (64, 128, 16), (128, 256, 32), (100, 130, 3), (192, 128, 16), (96, 192, 1)}
    for c in CASES:   # "identical k" is a fair demand only away from a tie of the stop rule
        assert INDEX[c]["margin"] >= 1e-3


@pytest.mark.parametrize("name", CASES)
def test_restated_iteration_reproduces_reference(name):
    meta, arrs, A, b, x0, mu = load_case(name)
    x, k, out = admm_ref.gl_admm_dual(x0, A, b, mu, {})
    assert k == int(arrs["k"])
    fh = np.asarray(out["f_hist"])
    assert np.max(np.abs(fh - arrs["f_hist"]) / np.abs(arrs["f_hist"])) <= 1e-10
    assert np.max(np.abs(np.asarray(out["f_hist_best"]) - arrs["f_hist_best"]) / np.abs(arrs["f_hist_best"])) <= 1e-10
    assert np.max(np.abs(x - arrs["x"])) <= 1e-10 * np.max(np.abs(arrs["x"]))
    # the Gram-based norms against the reference's SVD-based ones
    assert np.allclose(out["r_norm"], arrs["r_norm"], rtol=1e-6, atol=0)
    assert np.allclose(out["s_norm"], arrs["s_norm"], rtol=1e-6, atol=1e-14)


def _lmax_inputs():
    rng = np.random.default_rng(20241020)
    mats = []
    for l in (1, 2, 3, 16, 32):
        r = rng.standard_normal((200, l))
        mats.append(("gram_l%d" % l, r.T @ r))
        r = rng.standard_normal((3, l)) * 1e-4          # rank-deficient for l > 3, small entries
        mats.append(("gram_lowrank_l%d" % l, r.T @ r))
    v = rng.standard_normal(16)
    mats.append(("rank1", np.outer(v, v)))
    mats.append(("zero", np.zeros((8, 8))))
    mats.append(("equal_diagonal", 2.5 * np.identity(7)))
    return mats


@pytest.mark.parametrize("name,G", _lmax_inputs(), ids=[n for n, _ in _lmax_inputs()])
def test_sym_lambda_max(name, G):
    from glx import kernels
    l = G.shape[0]
    got = kernels.sym_lambda_max(G)
    want = float(np.linalg.eigvalsh(G)[-1])
    assert abs(got - want) <= 8 * l * np.finfo(np.float64).eps * np.trace(G)


def test_sym_lambda_max_nan_and_refusals():
    from glx import _lib, kernels
    G = np.identity(3)
    G[1, 1] = np.nan
    assert math.isnan(kernels.sym_lambda_max(G))
    out = ctypes.c_double(0)
    g = (ctypes.c_double * 1)(1.0)
    assert _lib.lib().glx_sym_lambda_max(g, 0, ctypes.byref(out)) == 1
    assert _lib.lib().glx_sym_lambda_max(g, 33, ctypes.byref(out)) == 1
    assert _lib.lib().glx_sym_lambda_max(None, 1, ctypes.byref(out)) == 1


def test_default_opts_are_the_references():
    from glx import _lib
    o = _lib.admm_default_opts()
    ref = admm_ref.DEFAULT_OPTS   # gl_ADMM_dual.py:11-17
    assert (o.maxit, o.converge_len) == (ref["maxit"], ref["converge_len"]) == (100, 20)
    assert o.thres == ref["thres"] == 1e-3
    assert o.rho == ref["rho"] == 1e2
    assert o.tau == ref["tau"] == (1 + math.sqrt(5)) * 0.5
    assert (o.fused, o.max_total_iters) == (0, 0)


def test_option_merging():
    from glx import admm
    given = {"maxit": 7, "rho": 50.0, "unknown_key": object(), "fused": 2}
    before = dict(given)
    o = admm.make_opts(given)
    assert given == before                       # the caller's dict is not mutated
    assert (o.maxit, o.rho, o.fused) == (7, 50.0, 2)
    assert (o.converge_len, o.thres) == (20, 1e-3)   # untouched defaults
    o = admm.make_opts({"thres": 1e-4, "tau": 1.0, "converge_len": 3, "max_total_iters": 5})
    assert (o.thres, o.tau, o.converge_len, o.max_total_iters) == (1e-4, 1.0, 3, 5)


def test_struct_layout_matches_c():
    from glx import _lib
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "glx.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(glx_admm_opts), offsetof(glx_admm_opts, maxit),
         offsetof(glx_admm_opts, converge_len), offsetof(glx_admm_opts, thres), offsetof(glx_admm_opts, tau),
         offsetof(glx_admm_opts, rho), offsetof(glx_admm_opts, fused),
         offsetof(glx_admm_opts, max_total_iters), offsetof(glx_admm_opts, reserved));
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        exe = os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib.GlxAdmmOpts
    want = [ctypes.sizeof(S), S.maxit.offset, S.converge_len.offset, S.thres.offset, S.tau.offset,
            S.rho.offset, S.fused.offset, S.max_total_iters.offset, S.reserved.offset]
    assert got == want


def _ws_bytes(dtype, m, n, l, opts=None):
    from glx import _lib
    nb = ctypes.c_size_t(0)
    rc = _lib.lib().glx_admm_workspace_bytes(dtype, m, n, l, ctypes.byref(opts) if opts is not None else None,
                                             ctypes.byref(nb))
    return rc, int(nb.value)


def test_workspace_grows_with_each_dimension():
    from glx import _lib
    for dt in (_lib.GLX_F64, _lib.GLX_F32):
        rc, base = _ws_bytes(dt, 128, 256, 16)
        assert rc == 0 and base > 0
        for shape in ((256, 256, 16), (128, 512, 16), (128, 256, 32)):
            rc, nb = _ws_bytes(dt, *shape)
            assert rc == 0 and nb > base, shape
    assert _ws_bytes(_lib.GLX_F64, 128, 256, 16)[1] > _ws_bytes(_lib.GLX_F32, 128, 256, 16)[1]
    assert _ws_bytes(_lib.GLX_F64, 128, 256, 0)[0] == 1      # GLX_E_INVALID
    assert _ws_bytes(_lib.GLX_F64, 128, 256, 33)[0] == 1
    assert _ws_bytes(7, 128, 256, 16)[0] == 1


def _solve_rc(m=64, n=128, l=16, comm=None, K=0x1000, ws=0x100000, ws_bytes=None, opts=None):
    """glx_admm_dual_solve on made-up (never dereferenced) device addresses: every refusal below
    is decided on the host before the first HIP call."""
    from glx import _lib
    o = opts if opts is not None else _lib.admm_default_opts()
    if ws_bytes is None:
        ws_bytes = _ws_bytes(_lib.GLX_F64, m, n, max(l, 1))[1]
    p = _lib.GlxProblem(dtype=_lib.GLX_F64, method=0, m=m, n=n, l=l, A=0x10000, b=0x20000, x=0x30000,
                        mu0=1e-2, comm=comm)
    res = _lib.GlxResult()
    rc = _lib.lib().glx_admm_dual_solve(ctypes.byref(p), K, ctypes.byref(o), ws, ws_bytes, ctypes.byref(res), None)
    msg = _lib.lib().glx_last_error().decode()
    return rc, msg


def test_refusals_are_invalid():
    from glx import _lib
    rc, msg = _solve_rc(comm=0x4000)
    assert rc == 1 and "comm" in msg
    assert _solve_rc(l=0)[0] == 1
    rc, msg = _solve_rc(K=None)
    assert rc == 1 and "K" in msg
    rc, msg = _solve_rc(ws_bytes=4096)
    assert rc == 1 and "workspace" in msg
    o = _lib.admm_default_opts()
    o.fused = 3
    assert _solve_rc(opts=o)[0] == 1


def test_describe_names_the_projection():
    from glx import _lib
    d = _lib.admm_describe(_lib.GLX_F64, 128, 256, 32)
    assert "projection=fused" in d and "k_atr_admm" in d and "K v=" in d and "A^T z=" in d
    d2 = _lib.admm_describe(_lib.GLX_F64, 256, 512, 2)
    assert "fused" not in d2 and "k_admm_dual" in d2
    off = _lib.admm_default_opts()
    off.fused = 2
    d3 = _lib.admm_describe(_lib.GLX_F64, 128, 256, 32, off)
    assert "fused" not in d3 and "k_admm_dual" in d3
    # the fp32 tile kAtrTiles marks fused
    assert "projection=fused" in _lib.admm_describe(_lib.GLX_F32, 128, 256, 32)


def test_driver_registry_is_unchanged():
    from glx import _lib
    assert "gl_ADMM_dual" not in _lib.METHODS and len(_lib.METHODS) == 5
