"""CPU-only checks of the optimality certificate (no GPU is touched).

* ``tests/certificate_ref.py``, the NumPy statement of DESIGN.md "Certificate", at the stored
  minimiser of the default instance, at x = 0 with mu = mu_max, and at the recorded results of the
  reference's ADMM and ALM solvers;
* the C ABI's refusals, the workspace's growth and ``glx_certificate_describe``.
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN

import certificate_ref as cref


def _index(name):
    with open(os.path.join(GOLDEN, name)) as fh:
        return json.load(fh)


RECORDED = [(f, c) for f in ("admm_index.json", "admm_primal_index.json", "alm_dual_index.json")
            for c in sorted(_index(f))]


def test_gap_at_the_stored_minimiser():
    with np.load(os.path.join(GOLDEN, "default_xstar.npz")) as z:
        xs, fval, mu, seed = z["x"], float(z["fval"]), float(z["mu"]), int(z["seed"])
    A, b, _, _ = cref.instance(seed, 256, 512, 2, mu)
    c = cref.certificate(xs, A, b, mu)
    print("gap %.3e  gap/primal %.3e  scale-1 %.3e" % (c["gap"], c["gap"] / c["primal"], c["scale"] - 1))
    assert c["gap"] >= 0
    assert c["gap"] <= 1e-10 * c["primal"]
    assert c["dual"] <= fval <= c["primal"]


@pytest.mark.parametrize("shape", [(256, 512, 2), (100, 130, 3), (64, 128, 16)])
def test_zero_is_optimal_at_mu_max(shape):
    m, n, l = shape
    A, b, _, _ = cref.instance(97006855, m, n, l)
    mm = cref.mu_max(A, b)
    c = cref.certificate(np.zeros((n, l)), A, b, mm)
    assert c["gap"] == 0
    assert c["scale"] == 1
    assert c["kkt_max"] == 0
    assert c["nonzero_rows"] == 0


@pytest.mark.parametrize("index,name", RECORDED, ids=[c for _, c in RECORDED])
def test_gap_is_nonnegative_at_recorded_results(index, name):
    meta = _index(index)[name]
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        x, b = z["x"], z["b"]
    A, _, _, mu = cref.instance(meta["seed"], meta["m"], meta["n"], meta["l"], meta["mu"])
    c = cref.certificate(x, A, b, mu)
    print("%s: gap/primal %.3e kkt_max %.3e" % (name, c["gap"] / c["primal"], c["kkt_max"]))
    assert c["gap"] >= 0
    assert c["dual"] <= c["primal"]
    assert c["kkt_max"] >= 0 and c["kkt_fro"] >= c["kkt_max"]


# ---- the C ABI ----
def _bytes(dtype, m, n, l):
    from glx import _lib
    nb = ctypes.c_size_t(0)
    rc = _lib.lib().glx_certificate_workspace_bytes(dtype, m, n, l, ctypes.byref(nb))
    return rc, int(nb.value)


def _last_error():
    from glx import _lib
    msg = _lib.lib().glx_last_error()
    return msg.decode() if msg else ""


def test_workspace_grows_and_l_limit():
    from glx import _lib
    for dt in (_lib.GLX_F64, _lib.GLX_F32):
        rc, base = _bytes(dt, 256, 512, 16)
        assert rc == 0 and base > 0
        assert _bytes(dt, 512, 512, 16)[1] > base
        assert _bytes(dt, 256, 1024, 16)[1] > base
        assert _bytes(dt, 256, 512, 32)[1] > base
    assert _bytes(_lib.GLX_F64, 256, 512, 16)[1] > _bytes(_lib.GLX_F32, 256, 512, 16)[1]
    assert _bytes(_lib.GLX_F64, 256, 512, 128)[0] == 0
    rc, _ = _bytes(_lib.GLX_F64, 256, 512, 129)
    assert rc == 1 and "128" in _last_error()
    assert _lib.lib().glx_certificate_workspace_bytes(_lib.GLX_F64, 256, 512, 16, None) == 1


def test_describe_names_the_tile_and_the_row_form():
    from glx import _lib
    fused = _lib.certificate_describe(_lib.GLX_F64, 128, 256, 32)
    assert "fused" in fused and "k_atr_cert" in fused
    off = _lib.certificate_describe(_lib.GLX_F64, 128, 256, 32, 2)
    assert "row kernel" in off and "k_cert_panel" in off
    generic = _lib.certificate_describe(_lib.GLX_F64, 100, 130, 3, 1)
    assert "row kernel" in generic and "k_cert_row" in generic
    # the A^T tile is the ADMM solvers' (the same plan, so the same fuse condition)
    atr = _lib.admm_describe(_lib.GLX_F64, 128, 256, 32).split("A^T z=")[1].split(";")[0]
    assert ("A^T r=" + atr) in fused
    buf = ctypes.create_string_buffer(64)
    for bad in (-1, 3):
        assert _lib.lib().glx_certificate_describe(_lib.GLX_F64, 128, 256, 32, bad, buf, len(buf)) == 1
        assert "fused" in _last_error()
    assert _lib.lib().glx_certificate_describe(_lib.GLX_F64, 128, 256, 32, 0, None, 0) == 1


def test_refusals():
    """Every refusal is GLX_E_INVALID (1) with a message, decided on the host before anything is
    launched: the pointers below are never dereferenced."""
    from glx import _lib
    h = _lib.lib()
    m, n, l = 64, 128, 16
    _, nb = _bytes(_lib.GLX_F64, m, n, l)
    P, WS = 0x10000, 0x100000    # "device pointers": non-null, aligned
    out = (ctypes.c_double * 8)()

    def call(dtype=_lib.GLX_F64, m=m, n=n, l=l, A=P, X=P, b=P, mu=0.01, fused=0, ws=WS, wsb=nb):
        return h.glx_certificate(dtype, m, n, l, A, X, b, mu, fused, None, None, out, ws, wsb, None)

    cases = {
        "dtype": dict(dtype=7), "m": dict(m=0), "n": dict(n=-4), "l": dict(l=0), "l>128": dict(l=129),
        "A": dict(A=None), "X": dict(X=None), "b": dict(b=None), "ws": dict(ws=None),
        "small": dict(wsb=nb - 1), "misaligned": dict(ws=WS + 64), "mu<0": dict(mu=-1e-300),
        "nan": dict(mu=math.nan), "fused-": dict(fused=-1), "fused+": dict(fused=3),
    }
    for name, kw in cases.items():
        assert call(**kw) == 1, name
        assert _last_error(), name
    # the one-launch surface refuses the same way
    sums = ctypes.c_void_p(P)
    assert h.glx_certificate_step(_lib.GLX_F64, m, n, l, None, None, P, P, 0.01, 2, None, sums, WS, nb, None) == 1
    assert h.glx_certificate_step(_lib.GLX_F64, m, n, 129, None, None, P, P, 0.01, 0, None, sums, WS, nb, None) == 1
    assert h.glx_certificate_step(_lib.GLX_F64, m, n, l, None, None, P, P, 0.01, 1, None, sums, WS, nb, None) == 1
    # the fused form is refused where the plan takes none
    _, nb2 = _bytes(_lib.GLX_F64, m, n, 2)
    assert h.glx_certificate_step(_lib.GLX_F64, m, n, 2, P, P, P, P, 0.01, 1, None, sums, WS, nb2, None) == 1
    assert "fused" in _last_error()


def test_compose_matches_the_reference():
    from glx.certificate import compose
    for gmax, mu in ((0.5, 0.25), (0.2, 0.25), (0.25, 0.25), (3.0, 0.0)):
        rec = [2.0, -1.5, 4.0, gmax, 0.3, 0.25, 5.0, 1.0]
        c = compose(rec, mu)
        p, d, g, s = cref.compose(2.0, -1.5, 4.0, gmax, mu)
        assert (c["primal"], c["dual"], c["gap"], c["scale"]) == (p, d, g, s)
        assert c["kkt_fro"] == 0.5 and c["nonzero_rows"] == 5 and c["fused"] is True
        assert c["rel_gap"] == g / p
    assert math.isnan(compose([1, 1, 1, math.nan, 1, 1, math.nan, 0], 0.1)["gap"])
