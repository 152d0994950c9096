"""Feature groups and weights without a device: the grouped rounding guard, the label helper and the
refusals. Reference: tests/group_ref.py.

The guard: group_ref.guard mirrors glx_group_screen_guard in float64 (checked on random records),
and at every instance's reference solution (group_ref.reference_solution, rel_gap <= 1e-12) the
guarded test, evaluated in longdouble on the float64 certificate's group norms, must screen no group
with x*_[g] != 0. The same must hold when the record's gap is forced to 0 and to -1e-9 of the primal
(sum_g w_g ||x_[g]|| is moved so that 1/2 (1 + s^2) rr + s rb + mu sx comes out there): the row
suite's tripwire for a computed gap that rounds to <= 0, which rho+ > 0 guards against.

The refusals: every bad description raises ValueError from the argument checks, before the library
touches a device (this suite runs on machines without one).
"""
import ctypes
import sys

import numpy as np
import pytest

import group_ref as gr


def _kernels():
    from glx import kernels
    return kernels


def test_guard_equals_reference_formulae():
    from glx import _lib
    k = _kernels()
    g = np.random.default_rng(11)
    for dtype, eps in ((_lib.GLX_F64, gr.EPS64), (_lib.GLX_F32, gr.EPS32)):
        for _ in range(50):
            m, n, l = int(g.integers(1, 5000)), int(g.integers(1, 20000)), int(g.integers(1, 129))
            max_run = int(g.integers(1, n + 1))
            rr = float(g.uniform(0.0, 10.0)) * float(g.choice([0.0, 1e-12, 1.0]))
            bn = float(g.uniform(0.0, 10.0))
            rb = float(g.uniform(-1.0, 1.0)) * np.sqrt(rr) * bn
            sx = float(g.uniform(0.0, 50.0))
            gmax = float(g.uniform(0.0, 2.0))
            mu = float(g.choice([0.0, 1e-3, 1.0, 5.0]))
            w_min = float(g.choice([0.01, 1.0, 7.5]))
            gcmax = float(g.uniform(0.1, 100.0))
            csq = gcmax * gcmax * float(g.uniform(1.0, n))
            rec = [rr, rb, sx, gmax, 0.0, 0.0, 0.0, 0.0]
            want = gr.guard(rec, mu, eps, m, n, l, max_run, w_min, gcmax, csq, bn)
            got = k.group_screen_guard(rec, mu, dtype, m, n, l, max_run, w_min, gcmax, csq, bn)
            for w, v in zip(want, got):
                assert (v == w) or abs(v - w) <= 8 * gr.EPS64 * abs(w), (dtype, m, n, l, max_run, rec, mu, want, got)
            assert 0.0 <= got[0] <= 1.0 and got[1] >= 0.0 and got[2] >= 0.0


def test_guard_with_single_rows_is_no_looser_than_the_row_guard():
    """Size-1 groups of weight 1: the grouped guard only adds roundings to the row guard's, so its s
    is no larger (gap+ and rho+ depend on s through s <r, b> and may move either way) and all three
    figures stay within the added roundings, a few gamma_{l+3} of the dtype, of the row guard's."""
    from glx import _lib
    k = _kernels()
    rec = [3.0, -1.2, 4.0, 0.9, 0.0, 0.0, 0.0, 0.0]
    for dtype, eps in ((_lib.GLX_F64, gr.EPS64), (_lib.GLX_F32, gr.EPS32)):
        row = k.screen_guard(rec, 0.5, dtype, 96, 512, 16, 11.0, 5e4, 30.0)
        grp = k.group_screen_guard(rec, 0.5, dtype, 96, 512, 16, 1, 1.0, 11.0, 5e4, 30.0)
        assert grp[0] <= row[0]
        for a, b in zip(grp, row):
            assert abs(a - b) <= 8 * gr.gamma(16 + 3, eps) * b


def test_guard_propagates_nan_and_refuses_bad_arguments():
    from glx import _lib
    k = _kernels()
    out = k.group_screen_guard([float("nan"), 0.0, 1.0, 1.0, 0, 0, 0, 0], 0.1, _lib.GLX_F64, 10, 10, 2, 3, 1.0, 1.0,
                               10.0, 1.0)
    assert all(np.isnan(v) for v in out[1:])
    out = k.group_screen_guard([1.0, 0.0, 1.0, float("nan"), 0, 0, 0, 0], 0.1, _lib.GLX_F64, 10, 10, 2, 3, 1.0, 1.0,
                               10.0, 1.0)
    assert all(np.isnan(v) for v in out)
    for bad in ((-1.0, _lib.GLX_F64, 2, 3, 1.0), (0.1, _lib.GLX_F64, 129, 3, 1.0), (0.1, 7, 2, 3, 1.0),
                (0.1, _lib.GLX_F64, 2, 0, 1.0), (0.1, _lib.GLX_F64, 2, 11, 1.0), (0.1, _lib.GLX_F64, 2, 3, 0.0),
                (0.1, _lib.GLX_F64, 2, 3, float("nan"))):
        mu, dtype, l, max_run, w_min = bad
        with pytest.raises(_lib.GlxError):
            k.group_screen_guard([1.0] * 8, mu, dtype, 10, 10, l, max_run, w_min, 1.0, 10.0, 1.0)


@pytest.fixture(scope="module", params=gr.CASES, ids=lambda c: "%dx%dx%d-%s@%g" % (c[0], c[1], c[2], c[3][1], c[4]))
def at_ref(request):
    m, n, l, pool, ratio = request.param
    ref = gr.reference_solution(m, n, l, pool, ratio)
    A, b, ptr, w, mu, x = (ref[k] for k in ("A", "b", "ptr", "w", "mu", "x"))
    c = gr.certificate(x, A, b, mu, ptr, w)
    gcn = np.asarray(gr.group_cnorms(A, ptr, w), dtype=np.float64)
    fig = (int(np.diff(ptr).max()), float(w.min()), float(gcn.max()), float(np.sum(A * A)),
           float(np.linalg.norm(b)))
    nz = gr.group_norms(x, ptr) != 0
    assert 0 < nz.sum() < nz.size
    return {"shape": (m, n, l), "mu": mu, "c": c, "gcn": gcn, "fig": fig, "nz": nz}


def _screened(case, rec, native):
    from glx import _lib
    m, n, l = case["shape"]
    if native:
        s, gap_p, rho = _kernels().group_screen_guard(rec, case["mu"], _lib.GLX_F64, m, n, l, *case["fig"])
    else:
        s, gap_p, rho = gr.guard(rec, case["mu"], gr.EPS64, m, n, l, *case["fig"])
    keep = gr.keep_mask(case["c"]["group_norms"], case["gcn"], s, rho, case["mu"])
    return s, gap_p, rho, ~keep


@pytest.mark.parametrize("native", [False, True], ids=["group_ref", "libglx"])
def test_guard_is_safe_at_the_reference_solution(at_ref, native):
    rec = gr.record(at_ref["c"])
    s, gap_p, rho, scr = _screened(at_ref, rec, native)
    assert rho > 0.0 and gap_p >= max(float(at_ref["c"]["gap"]), 0.0) and 0.0 < s <= 1.0
    assert not np.any(scr & at_ref["nz"])
    assert scr.sum() > 0                      # (the reference is accurate enough to screen something)


@pytest.mark.parametrize("native", [False, True], ids=["group_ref", "libglx"])
@pytest.mark.parametrize("forced", [0.0, -1e-9])
def test_guard_is_safe_when_the_gap_rounds_to_zero_or_below(at_ref, forced, native):
    c, mu = at_ref["c"], at_ref["mu"]
    rec = gr.record(c)
    s0 = _screened(at_ref, rec, native)[0]
    rr, rb = rec[0], rec[1]
    primal = 0.5 * rr + mu * rec[2]
    rec[2] = (forced * primal - (0.5 * (1.0 + s0 * s0) * rr + s0 * rb)) / mu
    gap = 0.5 * (1.0 + s0 * s0) * rr + s0 * rb + mu * rec[2]
    assert abs(gap - forced * primal) <= 1e-12 * primal
    s, gap_p, rho, scr = _screened(at_ref, rec, native)
    assert s == s0 and rho > 0.0 and gap_p > 0.0
    assert not np.any(scr & at_ref["nz"])


def test_the_model_of_the_issue_reaches_a_reduced_width():
    """The conditions the GPU tests assert of the screened arm (compactions >= 1, width < n) hold for
    the reference loop alone: every case reaches a padded kept width <= 0.9 n."""
    for m, n, l, pool, ratio in gr.CASES:
        A, b, ptr, w = gr.instance(gr.SEED, m, n, l, pool)
        _, info = gr.fista_screen(A, b, ratio * gr.mu_max(A, b, ptr, w), ptr, w, tol=1e-8)
        assert info["widths"] and min(info["widths"]) * 10 <= 9 * n, (pool, ratio, info["widths"])


def test_group_order_round_trips_a_shuffled_label_vector():
    import glx
    g = np.random.default_rng(5)
    ptr = gr.draw_groups(g, 200, gr.POOL_SMALL)
    names = g.permutation(1000)[: ptr.size - 1]            # arbitrary, distinct labels
    sorted_labels = np.repeat(np.sort(names), np.diff(ptr))
    shuffle = g.permutation(200)
    labels = sorted_labels[shuffle]
    perm, got_ptr = glx.group_order(labels)
    assert np.array_equal(labels[perm], sorted_labels) and np.array_equal(got_ptr, ptr)
    assert got_ptr.dtype == np.int32 and got_ptr[0] == 0 and got_ptr[-1] == 200
    # stable: rows of one label keep their order, so the permutation is unique
    for k in range(ptr.size - 1):
        assert np.all(np.diff(perm[ptr[k]:ptr[k + 1]]) > 0)
    # un-permuting puts a solution of the sorted problem back in the caller's order
    xs = g.standard_normal((200, 3))
    x = np.empty_like(xs)
    x[perm] = xs
    cols = g.standard_normal((4, 200))
    assert np.allclose(cols[:, perm] @ xs, cols @ x)
    assert np.array_equal(glx.group_order(["b", "a", "b"])[1], [0, 1, 3])
    with pytest.raises(ValueError):
        glx.group_order([])
    with pytest.raises(ValueError):
        glx.group_order(np.zeros((2, 2)))


BAD = [
    ("starts", dict(groups=[1, 3, 6])), ("ends", dict(groups=[0, 3, 5])), ("ends_past", dict(groups=[0, 3, 7])),
    ("repeats", dict(groups=[0, 3, 3, 6])), ("decreases", dict(groups=[0, 4, 3, 6])),
    ("floats", dict(groups=[0.0, 3.0, 6.0])), ("short", dict(groups=[0])), ("matrix", dict(groups=[[0, 6]])),
    ("zero_weight", dict(groups=[0, 3, 6], weights=[1.0, 0.0])),
    ("negative_weight", dict(groups=[0, 3, 6], weights=[1.0, -2.0])),
    ("nan_weight", dict(groups=[0, 3, 6], weights=[1.0, float("nan")])),
    ("inf_weight", dict(groups=[0, 3, 6], weights=[float("inf"), 1.0])),
    ("weights_length", dict(groups=[0, 3, 6], weights=[1.0, 1.0, 1.0])),
    ("row_weights_length", dict(weights=[1.0] * 5)), ("row_weights_zero", dict(weights=[1.0] * 5 + [0.0])),
]


@pytest.mark.parametrize("kw", [b[1] for b in BAD], ids=[b[0] for b in BAD])
def test_refusals_before_any_device_call(kw, monkeypatch):
    import glx
    cert_mod, screen_mod = sys.modules["glx.certificate"], sys.modules["glx.screen"]   # (glx.certificate is the function)

    def no_device(*a, **k):
        raise AssertionError("the library reached for a device before refusing")
    monkeypatch.setattr(cert_mod, "_inputs", no_device)
    monkeypatch.setattr(screen_mod, "_inputs", no_device)
    A, b, x = np.zeros((4, 6)), np.zeros((4, 2)), np.zeros((6, 2))
    with pytest.raises(ValueError):
        glx.certificate(x, A, b, 0.1, **kw)
    with pytest.raises(ValueError):
        glx.mu_max(A, b, **kw)
    with pytest.raises(ValueError):
        glx.solve_certified(A, b, 0.1, **kw)
    with pytest.raises(ValueError):
        glx.path(A, b, n_mus=2, **kw)


def test_refusals_of_width_and_communicator(monkeypatch):
    import glx
    cert_mod, screen_mod = sys.modules["glx.certificate"], sys.modules["glx.screen"]   # (glx.certificate is the function)

    def no_device(*a, **k):
        raise AssertionError("the library reached for a device before refusing")
    monkeypatch.setattr(cert_mod, "_inputs", no_device)
    monkeypatch.setattr(screen_mod, "_inputs", no_device)
    A, wide = np.zeros((4, 6)), np.zeros((4, 129))
    ok = dict(groups=[0, 3, 6], weights=[1.0, 2.0])
    with pytest.raises(ValueError, match="l <= 128"):
        glx.certificate(np.zeros((6, 129)), A, wide, 0.1, **ok)
    with pytest.raises(ValueError, match="l <= 128"):
        glx.solve_certified(A, wide, 0.1, **ok)
    with pytest.raises(ValueError, match="communicator"):
        glx.solve_certified(A, np.zeros((4, 2)), 0.1, comm=object(), **ok)
    with pytest.raises(ValueError, match="communicator"):
        glx.path(A, np.zeros((4, 2)), comm=object(), **ok)
    with pytest.raises(TypeError):
        glx.path(A, np.zeros((4, 2)), group=[0, 6])


def test_check_groups_defaults():
    from glx.certificate import check_groups
    assert check_groups(None, None, 6) is None
    ptr, w = check_groups([0, 2, 6], None, 6)
    assert ptr.dtype == np.int32 and np.array_equal(ptr, [0, 2, 6]) and np.array_equal(w, [1.0, 1.0])
    ptr, w = check_groups(None, [1, 2, 3], 3)
    assert np.array_equal(ptr, [0, 1, 2, 3]) and w.dtype == np.float64 and np.array_equal(w, [1.0, 2.0, 3.0])


def test_c_abi_refuses_on_the_host():
    """The C entries check the host description and the shapes before anything else: with no device
    these calls must come back GLX_E_INVALID (1), not a HIP error."""
    from glx import _lib
    h = _lib.lib()
    nb = ctypes.c_size_t(0)
    assert h.glx_group_certificate_workspace_bytes(_lib.GLX_F64, 96, 512, 16, 129, ctypes.byref(nb)) == 0
    base = ctypes.c_size_t(0)
    assert h.glx_certificate_workspace_bytes(_lib.GLX_F64, 96, 512, 16, ctypes.byref(base)) == 0
    assert nb.value > base.value
    assert h.glx_group_certificate_workspace_bytes(_lib.GLX_F64, 96, 512, 129, 10, ctypes.byref(nb)) == 1
    assert h.glx_group_certificate_workspace_bytes(_lib.GLX_F64, 96, 512, 16, 0, ctypes.byref(nb)) == 1
    assert h.glx_group_certificate_workspace_bytes(_lib.GLX_F64, 96, 512, 16, 513, ctypes.byref(nb)) == 1
    for screen in (0, 1):
        assert h.glx_group_certified_workspace_bytes(_lib.GLX_F64, 96, 512, 16, 129, screen, ctypes.byref(nb)) == 0
        row = ctypes.c_size_t(0)
        assert h.glx_certified_workspace_bytes(_lib.GLX_F64, 96, 512, 16, screen, ctypes.byref(row)) == 0
        assert nb.value > row.value
    assert "k_group_fista" in _lib.group_certified_describe(_lib.GLX_F64, 96, 512, 16, 8)
    assert "two sweeps" in _lib.group_certified_describe(_lib.GLX_F64, 96, 512, 16, 65)
    assert "k_group_cert" in _lib.group_certificate_describe(_lib.GLX_F32, 40, 130, 3, 5)
    ptr = np.array([0, 3, 6], dtype=np.int32)
    w = np.array([1.0, 2.0])
    rec = (ctypes.c_double * 8)()
    fake = 4096   # never dereferenced: every call below is refused first
    for p, ww in ((np.array([1, 3, 6], dtype=np.int32), w), (np.array([0, 3, 5], dtype=np.int32), w),
                  (np.array([0, 3, 3], dtype=np.int32), w), (ptr, np.array([1.0, 0.0])),
                  (ptr, np.array([1.0, float("nan")]))):
        rc = h.glx_group_certificate(_lib.GLX_F64, 4, 6, 2, fake, fake, fake, 0.1, 2, p.ctypes.data, ww.ctypes.data,
                                     None, None, rec, fake, 1 << 30, None)
        assert rc == 1 and b"groups:" in h.glx_last_error()
    rc = h.glx_group_certificate(_lib.GLX_F64, 4, 6, 2, fake, fake, fake, 0.1, 2, ptr.ctypes.data, w.ctypes.data,
                                 None, None, rec, fake, 16, None)
    assert rc == 1 and b"workspace" in h.glx_last_error()
