"""CPU-only checks of the primal ADMM solver's host surface (no GPU is touched).

* ``tests/admm_primal_ref.py``, the NumPy statement of the restructured iteration (explicit
  inverse, direct and Woodbury forms, Gram-based spectral norms), reproduces the reference's
  recorded runs: ``k`` exactly, ``f_hist`` within 1e-8 relative (the project's fp64 bar; measured
  <= 6.4e-10 direct and <= 2.1e-9 Woodbury, recorded per case in ``admm_primal_index.json``);
* defaults, option merging, the struct layout, the refusals (the fp32 rule among them) and the
  automatic choice of form through ``glx_admm_primal_describe``.
"""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import admm_primal_ref

with open(os.path.join(GOLDEN, "admm_primal_index.json")) as _fh:
    INDEX = json.load(_fh)
CASES = sorted(INDEX)
WIDE = [c for c in CASES if INDEX[c]["m"] < INDEX[c]["n"]]   # the cases Woodbury serves


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
    got = sorted((INDEX[c]["m"], INDEX[c]["n"], INDEX[c]["l"], INDEX[c]["opts"].get("step_type", "fixed"))
                 for c in CASES)
    want = sorted([(256, 512, 2, "fixed"), (64, 128, 16, "fixed"), (128, 256, 32, "fixed"),
                   (100, 130, 3, "fixed"), (192, 128, 16, "fixed"), (96, 192, 1, "fixed"),
                   (64, 128, 16, "diminishing"), (64, 128, 16, "diminishing2")])
    assert got == want
    for c in CASES:   # "identical k" is a fair demand only away from a tie of the stop rule
        assert INDEX[c]["margin"] >= 5e-3
        dev = INDEX[c]["restated_deviation"]
        assert ("woodbury" in dev) == (c in WIDE)
        assert all(d["f_hist"] <= 1e-8 for d in dev.values())
    assert sorted(INDEX[c]["k"] for c in CASES if not INDEX[c]["opts"]) == sorted([63, 52, 58, 100, 36, 86])


@pytest.mark.parametrize("name,form", [(c, 1) for c in CASES] + [(c, 2) for c in WIDE])
def test_restated_iteration_reproduces_reference(name, form):
    meta, arrs, A, b, x0, mu = load_case(name)
    x, k, out = admm_primal_ref.gl_admm_primal(x0, A, b, mu, {**meta["opts"], "form": form})
    assert out["form"] == form
    assert k == int(arrs["k"])
    rel = lambda got, want: np.max(np.abs(np.asarray(got) - want) / np.abs(want))
    print("%s form %d: f_hist %.2e, x %.2e, r %.2e, s %.2e" % (
        name, form, rel(out["f_hist"], arrs["f_hist"]), np.max(np.abs(x - arrs["x"])) / np.max(np.abs(arrs["x"])),
        rel(out["r_norm"], arrs["r_norm"]), rel(out["s_norm"], arrs["s_norm"])))
    assert rel(out["f_hist"], arrs["f_hist"]) <= 1e-8
    assert rel(out["f_hist_best"], arrs["f_hist_best"]) <= 1e-8
    assert abs(out["fval"] - arrs["fval"]) <= 1e-8 * abs(arrs["fval"])
    assert np.max(np.abs(x - arrs["x"])) <= 1e-8 * np.max(np.abs(arrs["x"]))
    # the Gram-based norms of the restructured iteration against the reference's SVD-based ones:
    # three orders inside the 5e-3 margin every fixture keeps from thres
    assert rel(out["r_norm"], arrs["r_norm"]) <= 5e-6
    assert rel(out["s_norm"], arrs["s_norm"]) <= 5e-6


def test_restated_auto_form_is_the_byte_count_rule():
    assert admm_primal_ref.resolve_form(0, 8192, 16384) == 2
    assert admm_primal_ref.resolve_form(0, 100, 130) == 1
    assert admm_primal_ref.resolve_form(0, 192, 128) == 1
    assert admm_primal_ref.resolve_form(0, 128, 128) == 1
    assert admm_primal_ref.resolve_form(1, 64, 128) == 1 and admm_primal_ref.resolve_form(2, 100, 130) == 2


def test_default_opts_are_the_references():
    from glx import _lib
    o = _lib.admm_primal_default_opts()
    ref = admm_primal_ref.DEFAULT_OPTS   # gl_ADMM_primal.py:11-20
    assert (o.maxit, o.converge_len) == (ref["maxit"], ref["converge_len"]) == (100, 10)
    assert o.thres == ref["thres"] == 1e-3
    assert o.rho == ref["rho"] == 1e-2
    assert o.eta_0 == ref["eta_0"] == 100
    assert o.tau == ref["tau"] == (1 + 5 ** 0.5) * 0.5
    assert o.step_type == 1 and ref["step_type"] == "fixed"
    assert (o.form, o.max_total_iters) == (0, 0)


def test_option_merging():
    from glx import admm_primal
    given = {"maxit": 7, "rho": 0.5, "unknown_key": object(), "converge_thres": 1e-5, "form": 2,
             "step_type": "diminishing2"}
    before = dict(given)
    o = admm_primal.make_opts(given)
    assert given == before                       # the caller's dict is not mutated
    assert (o.maxit, o.rho, o.form, o.step_type) == (7, 0.5, 2, 3)
    assert (o.converge_len, o.thres, o.eta_0) == (10, 1e-3, 100.0)   # untouched defaults
    o = admm_primal.make_opts({"thres": 1e-4, "tau": 1.0, "converge_len": 3, "max_total_iters": 5,
                               "eta_0": 2, "step_type": "diminishing"})
    assert (o.thres, o.tau, o.converge_len, o.max_total_iters, o.eta_0, o.step_type) == (1e-4, 1.0, 3, 5, 2.0, 2)
    assert admm_primal.make_opts({"step_type": "fixed"}).step_type == 1
    with pytest.raises(ValueError):
        admm_primal.make_opts({"step_type": "line_search"})


def test_struct_layout_matches_c():
    from glx import _lib
    fields = [f for f, _ in _lib.GlxAdmmPrimalOpts._fields_]
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "glx.h"
int main(void) {
  printf("%zu", sizeof(glx_admm_primal_opts));
''' + "".join('  printf(" %%zu", offsetof(glx_admm_primal_opts, %s));\n' % f for f in fields) + r'''
  printf("\n");
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        exe = os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib.GlxAdmmPrimalOpts
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields]


def _describe(dtype, m, n, l, opts=None):
    from glx import _lib
    buf = ctypes.create_string_buffer(2048)
    rc = _lib.lib().glx_admm_primal_describe(dtype, m, n, l, ctypes.byref(opts) if opts is not None else None,
                                             buf, len(buf))
    return rc, (buf.value.decode() if rc == 0 else _lib.lib().glx_last_error().decode())


def _ws_bytes(dtype, m, n, l, opts=None):
    from glx import _lib
    nb = ctypes.c_size_t(0)
    rc = _lib.lib().glx_admm_primal_workspace_bytes(dtype, m, n, l, ctypes.byref(opts) if opts is not None else None,
                                                    ctypes.byref(nb))
    return rc, int(nb.value)


def test_auto_form_is_the_byte_count_rule():
    """Woodbury exactly when m^2 + m n < n^2 (m / n < 0.618)."""
    from glx import _lib
    F64 = _lib.GLX_F64
    for (m, n), want in (((8192, 16384), "Woodbury"), ((100, 130), "direct"), ((192, 128), "direct"),
                         ((128, 128), "direct")):
        rc, d = _describe(F64, m, n, 32 if m > 1000 else 3)
        assert rc == 0 and d.startswith("form=%s;" % want), (m, n, d)
        assert admm_primal_ref.resolve_form(0, m, n) == (2 if want == "Woodbury" else 1)
    # the boundary itself: 61^2 + 61 * 100 = 9821 < 10^4 <= 62^2 + 62 * 100 = 10044
    assert _describe(F64, 61, 100, 4)[1].startswith("form=Woodbury;")
    assert _describe(F64, 62, 100, 4)[1].startswith("form=direct;")
    # a given form overrides the rule, and each names its passes
    o = _lib.admm_primal_default_opts()
    o.form = 1
    d = _describe(F64, 8192, 16384, 32, o)[1]
    assert d.startswith("form=direct;") and "Kn w=" in d and "A x=" in d and "A^T" not in d
    o.form = 2
    d = _describe(F64, 100, 130, 3, o)[1]
    assert d.startswith("form=Woodbury;") and "K v=" in d and "A^T q=" in d and "A [x|z]=" in d
    assert "k_admm_primal" in d


def test_fp32_only_for_tall_direct():
    from glx import _lib, admm_primal
    F32 = _lib.GLX_F32
    rc, d = _describe(F32, 192, 128, 16)
    assert rc == 0 and d.startswith("form=direct;")
    assert _describe(F32, 128, 128, 16)[0] == 0
    assert _ws_bytes(F32, 192, 128, 16)[0] == 0
    o = _lib.admm_primal_default_opts()
    for form in (0, 1, 2):
        o.form = form
        for m, n, l in [(INDEX[c]["m"], INDEX[c]["n"], INDEX[c]["l"]) for c in WIDE]:
            rc, msg = _describe(F32, m, n, l, o)
            assert rc == 1 and "condition" in msg and "fp64" in msg, (m, n, l, form, msg)
            assert _ws_bytes(F32, m, n, l, o)[0] == 1
    o.form = 2
    rc, msg = _describe(F32, 192, 128, 16, o)   # Woodbury is refused in fp32 whatever the shape
    assert rc == 1 and "condition" in msg
    # the Python layer raises before it touches a device or spends the setup
    with pytest.raises(_lib.GlxError, match="condition"):
        admm_primal.solve(np.zeros((128, 16), np.float32), np.zeros((64, 128), np.float32),
                          np.zeros((64, 16), np.float32), 1e-2, {})


def test_workspace_grows_with_each_dimension():
    from glx import _lib
    rc, base = _ws_bytes(_lib.GLX_F64, 128, 256, 16)
    assert rc == 0 and base > 0
    for shape in ((256, 512, 16), (128, 512, 16), (128, 256, 32)):
        rc, nb = _ws_bytes(_lib.GLX_F64, *shape)
        assert rc == 0 and nb > base, shape
    assert _ws_bytes(_lib.GLX_F64, 256, 128, 16)[1] > _ws_bytes(_lib.GLX_F32, 256, 128, 16)[1]
    assert _ws_bytes(_lib.GLX_F64, 128, 256, 0)[0] == 1      # GLX_E_INVALID
    assert _ws_bytes(_lib.GLX_F64, 128, 256, 33)[0] == 1
    assert _ws_bytes(7, 128, 256, 16)[0] == 1


def _solve_rc(m=64, n=128, l=16, dtype=None, comm=None, A=0x10000, K=0x1000, ATb=0x2000, AATb=0x3000,
              ws=0x100000, ws_bytes=None, opts=None):
    """glx_admm_primal_solve on made-up (never dereferenced) device addresses: every refusal below
    is decided on the host before the first HIP call."""
    from glx import _lib
    dtype = _lib.GLX_F64 if dtype is None else dtype
    o = opts if opts is not None else _lib.admm_primal_default_opts()
    if ws_bytes is None:
        ws_bytes = _ws_bytes(_lib.GLX_F64, m, n, min(max(l, 1), 32))[1]
    p = _lib.GlxProblem(dtype=dtype, method=0, m=m, n=n, l=l, A=A, b=0x20000, x=0x30000, mu0=1e-2, comm=comm)
    res = _lib.GlxResult()
    rc = _lib.lib().glx_admm_primal_solve(ctypes.byref(p), K, ATb, AATb, ctypes.byref(o), ws, ws_bytes,
                                          ctypes.byref(res), None)
    return rc, _lib.lib().glx_last_error().decode()


def test_refusals_are_invalid():
    from glx import _lib
    rc, msg = _solve_rc(comm=0x4000)
    assert rc == 1 and "comm" in msg
    assert _solve_rc(l=0)[0] == 1
    rc, msg = _solve_rc(l=33)
    assert rc == 1 and "32" in msg
    rc, msg = _solve_rc(K=None)
    assert rc == 1 and "K" in msg
    rc, msg = _solve_rc(ATb=None)
    assert rc == 1 and "ATb" in msg
    rc, msg = _solve_rc(AATb=None)                 # (64, 128) resolves to Woodbury
    assert rc == 1 and "AATb" in msg
    rc, msg = _solve_rc(A=0x10008)
    assert rc == 1 and "aligned" in msg
    rc, msg = _solve_rc(ATb=0x2004)
    assert rc == 1 and "aligned" in msg
    rc, msg = _solve_rc(ws_bytes=4096)
    assert rc == 1 and "workspace" in msg
    rc, msg = _solve_rc(dtype=_lib.GLX_F32)
    assert rc == 1 and "condition" in msg
    for field, bad in (("rho", 0.0), ("rho", -1.0), ("eta_0", 0.0), ("step_type", 0), ("step_type", 4),
                       ("form", 3), ("form", -1), ("maxit", -1)):
        o = _lib.admm_primal_default_opts()
        setattr(o, field, bad)
        rc, msg = _solve_rc(opts=o)
        assert rc == 1, (field, bad)
        assert _describe(_lib.GLX_F64, 64, 128, 16, o)[0] == 1, (field, bad)


def test_driver_registry_is_unchanged():
    from glx import _lib
    assert "gl_ADMM_primal" not in _lib.METHODS and len(_lib.METHODS) == 5
    assert _lib.lib().glx_abi_version() == 2
