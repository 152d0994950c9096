"""The residual finalize at the head of k_atr_prox (kernels_atr.hip fin_head_run).

One launch at a time through glx.kernels.fin_atr_prox (glx_fin_atr_prox): the head launch against
k_finalize_residual followed by the plain k_atr_prox, on caller-supplied slabs. The head walks the
separate kernel's 256-thread blocks with the same element map, slab folds and in-block reduction,
so there is no tolerance: r0, r1, every partial, G, p, p_thr, z, the masks and the six trial sums
must agree in every bit, and a second launch of either form must repeat them.

Shapes (the smallest at which the head can go wrong): (8, 64, 16) one panel and fewer elements than
one block; (100, 128, 32) 12.5 blocks over 2 workgroups, a ragged last block and uneven shares;
(64, 1024, 32) 8 blocks over 16 workgroups, so workgroups without a share must still arrive;
(260, 192, 16). At each: chain 0, 1, 2; S in {1, 3, 8}; without the count, with it against *cmax,
and with it against pending trial partials.

Sessions: 30 iterations at (64, 1024, 32) and (100, 128, 32), at alpha0 and at 2.5 alpha0 (rejected
trials), with the A e gather and with A e fused into the dense pass: x and f_hist byte-identical
between GLX_FIN_HEAD=0, the default (the separate kernel: the head is opt-in) and GLX_FIN_HEAD=1,
and fin_form() names the form that ran.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

THRES = 1e-3
SHAPES = [(8, 64, 16), (100, 128, 32), (64, 1024, 32), (260, 192, 16)]
S0_OF = {1: 1, 3: 8, 8: 2}   # the A e slabs of a chained finalize: fewer, equal and more than S
OUT_KEYS = ("R0", "R1", "fin_parts", "G", "p", "pthr", "z", "sums", "zf")


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.int64) if a.dtype == np.float64 else a


@functools.lru_cache(maxsize=None)
def _inputs(m, n, l):
    """Shared by every case of a shape, never written: A, b, the iterate, the count's array and
    pending partials; the slabs for the largest S + S0."""
    rng = np.random.default_rng(100000 * m + 100 * n + l)
    A = rng.standard_normal((m, n))
    B = rng.standard_normal((m, l))
    slabs = rng.standard_normal((16, m, l))
    # entries of p = prox(x - t G) on both sides of THRES, some rows entirely small
    x = rng.standard_normal((n, l)) * 2.0 * THRES
    x[::5] *= 0.1
    cx = rng.standard_normal((n, l))
    cx[rng.random((n, l)) < 0.3] *= 1e-7   # below 1e-6 max |cx|
    cx[rng.random((n, l)) < 0.1] = 0.0
    parts = rng.standard_normal((300, 6))   # more slots than threads stride once
    parts[:, 3] = 0.1 * np.abs(parts[:, 3])   # below max |cx|, which slot 137 holds
    parts[137, 3] = float(np.max(np.abs(cx)))
    cmax = np.array([np.max(np.abs(cx))])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return {k: dev(v) for k, v in dict(A=A, B=B, slabs=slabs, x=x, cx=cx, parts=parts, cmax=cmax).items()}


def _launch(inp, m, n, l, chain, S, count, head):
    from glx import kernels
    S0 = S0_OF[S] if chain else 0
    nslab = S0 + S if chain else 2 * S
    P = inp["slabs"][:nslab].contiguous()
    kw = {}
    if count != "none":
        kw["cx"] = inp["cx"]
        kw["cmax" if count == "cmax" else "cmax_parts"] = inp["cmax"] if count == "cmax" else inp["parts"]
    out = kernels.fin_atr_prox(inp["A"], P, inp["B"], inp["x"], 1e-4 / np.sqrt(m), 0.1, S, S0=S0, chain=chain,
                               thres=THRES, emode=True, head=head, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("S", [1, 3, 8])
@pytest.mark.parametrize("chain", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_head_equals_finalize_then_trial(shape, chain, S):
    m, n, l = shape
    inp = _inputs(m, n, l)
    for count in ("none", "cmax", "parts"):
        ref = _launch(inp, m, n, l, chain, S, count, head=False)
        ref2 = _launch(inp, m, n, l, chain, S, count, head=False)
        got = _launch(inp, m, n, l, chain, S, count, head=True)
        got2 = _launch(inp, m, n, l, chain, S, count, head=True)
        nvb = ref["fin_parts"].shape[0]
        assert nvb == min(1024, -(-max(m * l, n * l if count != "none" else 0) // 256))
        assert got["fin_parts"].shape[0] == nvb
        # the reference is a real result: finite residuals and sums, a count where one is asked for,
        # flagged entries for the masks to show
        assert torch.isfinite(ref["R1"]).all() and torch.isfinite(ref["sums"]).all()
        assert torch.isfinite(ref["fin_parts"]).all()
        if count != "none":
            tot = float(ref["fin_parts"][:, 3].sum())
            want = float((inp["cx"].abs() > 1e-6 * inp["cmax"][0]).sum())
            assert tot == want, (tot, want)
        assert int((ref["zf"][:n] != 0).sum()) > 0
        for key in OUT_KEYS:
            if key == "R0" and chain == 0:
                assert torch.isfinite(ref["R0"]).all()
            a, b = _bits(ref[key]), _bits(got[key])
            diff = int((a != b).sum())
            print("%s %s chain %d S %d: %s differs in %d of %d" % (shape, count, chain, S, key, diff, a.size))
            assert np.array_equal(a, b), (key, count)
            assert np.array_equal(a, _bits(ref2[key])), (key, count, "finalize + trial, second launch")
            assert np.array_equal(b, _bits(got2[key])), (key, count, "head, second launch")


def _solve(monkeypatch, shape, scale, fused, head):
    from glx.solver import Session
    from oracle import numpy_ref
    m, n, l = shape
    monkeypatch.setenv("GLX_SPLIT_CAND", "1")
    if fused:
        monkeypatch.setenv("GLX_AX_VARIANT", "92278")
        monkeypatch.setenv("GLX_AE_HYB_ROWS", "1")
    else:
        monkeypatch.delenv("GLX_AX_VARIANT", raising=False)
        monkeypatch.setenv("GLX_AE_HYB_ROWS", "0")
    if head is None:
        monkeypatch.delenv("GLX_FIN_HEAD", raising=False)
    else:
        monkeypatch.setenv("GLX_FIN_HEAD", "1" if head else "0")
    A, b, u, x0, mu = numpy_ref.gen_data(m, n, l, 97006855)
    opts = {"alpha0": scale * numpy_ref.step_size_for(m, n), "maxit": 10}
    xd = torch.from_numpy(x0).cuda().clone()
    s = Session("gl_ProxGD_primal", xd, torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda(), float(mu),
                dict(opts))
    try:
        form = s.fin_form()
        plan = s.describe()
        s.run(0)
        res = s.finish()
        forms = s.ae_forms()
    finally:
        s.close()
    torch.cuda.synchronize()
    return form, plan, res, forms, xd.cpu().numpy()


@pytest.mark.parametrize("fused", [False, True], ids=["gather", "fused_ae"])
@pytest.mark.parametrize("scale", [1.0, 2.5], ids=["alpha0", "alpha0x2.5"])
@pytest.mark.parametrize("shape", [(64, 1024, 32), (100, 128, 32)], ids=lambda s: "%dx%dx%d" % s)
def test_session_identical_with_and_without_head(monkeypatch, shape, scale, fused):
    fk, pk, rk, ck, xk = _solve(monkeypatch, shape, scale, fused, head=False)
    fd, pd, rd, cd, xd = _solve(monkeypatch, shape, scale, fused, head=None)
    fh, ph, rh, ch, xh = _solve(monkeypatch, shape, scale, fused, head=True)
    # the default is the separate kernel (the head is opt-in: it measured level, not faster)
    assert fd == "fin=kernel" and pd == pk and cd == ck, fd
    assert [float(v).hex() for v in rd["f_hist"]] == [float(v).hex() for v in rk["f_hist"]]
    assert np.array_equal(xd.view(np.int64), xk.view(np.int64))
    print(ph, fh, "| iterations", rh["k"], "A@X passes", rh["ax_calls"], "A e forms", ch)
    assert fk == "fin=kernel", fk
    assert fh == "fin=head", fh
    assert pk == ph and "+trial (k_atr_prox)" in ph, ph
    assert rh["k"] == rk["k"] == 30
    if fused:
        assert ch["ae_fused_trials"] > 0, ch
    else:
        assert ch["ae_fused_trials"] == 0 and ch["ae_gather_trials"] > 0, ch
    if scale > 1.0:   # the step is too long: first trials are rejected, later trials keep the kernel
        assert rh["ax_calls"] > rh["k"] + 3, rh["ax_calls"]
    assert ck == ch
    assert [float(v).hex() for v in rk["f_hist"]] == [float(v).hex() for v in rh["f_hist"]]
    assert np.array_equal(xk.view(np.int64), xh.view(np.int64))
    for key in ("ax_calls", "atr_calls", "syncs", "ax_sources"):
        assert rk[key] == rh[key], key
