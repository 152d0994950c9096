"""The six glue kernels of the splitting solvers (dual ADMM, primal ADMM, dual ALM), one launch each.

Reached through glx_admm_rhs, glx_admm_fin, glx_admm_primal_rhs, glx_admm_primal_fin, glx_alm_j and
glx_alm_x (glx.kernels); nothing else is imported from glx, the references are the NumPy lines below.

Tier (a), every bit. libglx is built with -ffp-contract=off, so each element is a fixed chain of IEEE
operations in T that NumPy reproduces exactly: the slabs added in ascending order from slab 0
(slab_sum), then the expression of the kernel's header comment, scalars rounded to T first:
  k_admm_v           v = (Ax - rho Au) - b       (with Au = Ax, rho = 0: (Ax - 0 Ax) - b, which is +0
                                                   where Ax - b would be -0; asserted on such elements)
  k_admm_fin         Ax = sum of slabs 0 .. S-1, Au+ = sum of slabs S .. 2S-1, s = Au - Au+
  k_admm_primal_w    w = (ATb - z) + rho x
  k_admm_primal_fin  Ax, Az likewise, v = (AATb - Az) + rho Ax
  k_alm_j            J = rho (h - x / rho)
  k_alm_x            r = u + g, x+ = x - taurho r
The two sources' slabs differ in sign and slab k is scaled by k + 1, so a wrong offset, a dropped
slab or a swapped source cannot cancel.

Tier (b), the sums.
  sum (Ax - b)^2   the kernel rounds r = Ax - b and r * r to T and adds the squares as doubles. Ax is
       known to the bit (tier a), so the squares are formed here in T exactly as the kernel forms them
       and summed exactly (math.fsum); what is left is the fp64 accumulation, CSUM = 32 additions deep
       (a few per thread, 8 levels in the workgroup, 12 over the workgroup partials; the form and the
       constant of tests/test_gpu_admm.py), one more per further trip of a thread:
         |sum - ref| <= C (CSUM + trips - 1) eps64 sum r^2,   C = 2.
  sum_i ||x+_i||   (k_alm_x) test_gpu_admm.py's bar with dx = 0, x+ being known to the bit: per row the
       l squares, <= 6 additions and the root, (l / 2 + 2) eps ||x+_i||, plus the accumulation:
         |sum - ref| <= C ((l / 2 + 2) eps + (CSUM + trips - 1) eps64) sum_i ||x+_i||.
  max |x+|         exact: a maximum of values known to the bit.

Shapes. The elementwise and finalize kernels: S in 1, 2, 3, 8 (the finalize's second source starts
at P + S ml), both dtypes (k_alm_j: fp64, the solver's only type), 1, 255, 257 and 1025 elements, and
one ragged size past the grid cap each: (m, l) = (8201, 32) for the finalize kernels
(min(ceil(ml / 256), 1024) workgroups: one trip of 262144 elements, then 288 more) and (32771, 32) for
the rhs, w and J kernels (min(ceil(ml / 1024), 1024) workgroups: 1048576, then 96 more). At those the
elements on both sides of the trip boundary run again in a launch of their own, bit for bit.
k_alm_x: every (LPR, EPL) of launch_alm_x (l = 1, 2, 3, 5, 8, 16, 17, 32) by n in 1, 15, 64, 130, 257,
and the several-trip pairs of the other row modules, S in 1, 3, in place (the solver's call,
x_out == x) and out of place with identical bits.

Branches: s == NULL and AATb == NULL leave sentinel buffers untouched and change nothing else; one
NaN input element makes the sum NaN and that element's outputs NaN and leaves every other bit;
l = 33 and fp32 are refused by the ALM pair with a message before anything is written.

Measured on an MI355X, worst error / bound (the module prints this table when its tests are over,
pytest -s); tier (a) has no figure, every bit agreed:
  k_admm_fin sum (Ax - b)^2         f64 0.011   f32 0.000 (sums of a few thousand fp32 squares are exact in fp64)
  k_admm_primal_fin sum (Ax - b)^2  f64 0.012   f32 0.011
  k_alm_x sum_i ||x+_i||            0.014       max |x+| exact
None is above 1. Mutations this module catches are listed in tests/test_gpu_split_loops.py.
"""
import json
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C = 2.0
CSUM = 32
EPS64 = float(np.finfo(np.float64).eps)
RHO, TAU = 1e2, (1 + math.sqrt(5)) * 0.5
MEASURED = {}

DTS = [np.float64, np.float32]
DT_IDS = ["f64", "f32"]
SPLITS = [1, 2, 3, 8]
SMALL = [1, 255, 257, 1025]
FIN_BIG = 8201 * 32      # one trip of 1024 * 256 = 262144 elements, then 288
RHS_BIG = 32771 * 32     # one trip of 1024 * 1024 = 1048576 elements, then 96
FIN_TRIP, RHS_TRIP = 1024 * 256, 1024 * 1024


def _note(key, ratio):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MEASURED:
        print("\nworst error / bound:", json.dumps({k: round(v, 4) for k, v in sorted(MEASURED.items())}))


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert bad.size == 0, (what, int(bad.size), int(bad[0]), got[bad[0]], want[bad[0]])


def _tag(dt):
    return "f64" if dt == np.float64 else "f32"


# ---------------------------------------------------------------------------------------------
# the references, in T
# ---------------------------------------------------------------------------------------------
def slab_sum(P):
    """P[0] + P[1] + ... in that order, in P's type (slab_sum, glx_device.h)."""
    v = P[0].copy()
    for k in range(1, P.shape[0]):
        v = v + P[k]
    return v


def ref_admm_v(Ax, Au, b, rho):
    dt = b.dtype.type
    return (Ax - dt(rho) * Au) - b


def ref_admm_fin(P, S, b, Au):
    ax, au = slab_sum(P[:S]), slab_sum(P[S:])
    r = ax - b
    return {"Ax": ax, "Au": au, "s": Au - au, "sq": r * r}


def ref_primal_w(ATb, x, z, rho):
    dt = x.dtype.type
    return (ATb - z) + dt(rho) * x


def ref_primal_fin(P, S, b, AATb, rho):
    dt = b.dtype.type
    ax = slab_sum(P[:S])
    r = ax - b
    out = {"Ax": ax, "sq": r * r}
    if AATb is not None:
        az = slab_sum(P[S:])
        out["Az"] = az
        out["v"] = (AATb - az) + dt(rho) * ax
    return out


def ref_alm_j(h, x, rho):
    return np.float64(rho) * (slab_sum(h) - x / np.float64(rho))


def ref_alm_x(x, u, g, taurho):
    r = u + slab_sum(g)
    return {"r": r, "x": x - np.float64(taurho) * r}


def _sq_check(got_sum, sq, trips, key):
    """sum (Ax - b)^2 against the exact sum of the T-rounded squares, under the accumulation's bar."""
    ref = math.fsum(sq.astype(np.float64).tolist())
    bar = C * (CSUM + trips - 1) * EPS64 * ref
    err = abs(float(got_sum) - ref)
    if bar == 0.0:
        assert err == 0.0, key
        return
    _note(key, err / bar)
    assert err <= bar, (key, err, bar)


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def _vec(rng, count, dt, scale=1.0):
    return (rng.standard_normal(count) * scale).astype(dt)


def _two_sources(rng, count, S, dt):
    """2 S slabs: the first source positive, the second negative, slab k scaled by k + 1."""
    k = np.arange(1, S + 1, dtype=np.float64)[:, None]
    a = (0.25 + rng.random((S, count))) * k
    c = -(0.25 + rng.random((S, count))) * k
    return np.concatenate([a, c]).astype(dt)


def _trips(count, per_block):
    grid = min(-(-count // per_block), 1024)
    return -(-count // (grid * 256))


SIZES_FIN = SMALL + [FIN_BIG]
SIZES_RHS = SMALL + [RHS_BIG]


# ---------------------------------------------------------------------------------------------
# k_admm_v, k_admm_primal_w
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("ml", SIZES_RHS)
def test_admm_rhs(ml, dt):
    from glx import kernels
    rng = np.random.default_rng(ml)
    Ax, Au, b = _vec(rng, ml, dt), _vec(rng, ml, dt, 0.01), _vec(rng, ml, dt)
    got = _host(kernels.admm_rhs(_dev(Ax), _dev(Au), _dev(b), RHO))
    _same_bits(got, ref_admm_v(Ax, Au, b, RHO), "v")
    if ml >= RHS_TRIP:   # both sides of the trip boundary, in a launch of their own
        sl = slice(RHS_TRIP - 251, ml)
        part = _host(kernels.admm_rhs(_dev(Ax[sl]), _dev(Au[sl]), _dev(b[sl]), RHO))
        _same_bits(part, got[sl], "v at the trip boundary")
    # one NaN input: that element NaN, every other bit as before
    i = ml // 2
    b2 = b.copy()
    b2[i] = np.nan
    got2 = _host(kernels.admm_rhs(_dev(Ax), _dev(Au), _dev(b2), RHO))
    assert np.isnan(got2[i])
    keep = np.arange(ml) != i
    _same_bits(got2[keep], got[keep], "v beside the NaN")


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("ml", [257, RHS_BIG])
def test_admm_rhs_aliased_sources_rho_zero(ml, dt):
    """The dual ALM solver's call: one pointer for both sources, rho = 0. The kernel still evaluates
    (Ax - 0 * Ax) - b. At Ax = -0, b = +0 that is +0 (0 * -0 = -0, -0 - -0 = +0, +0 - +0 = +0) where
    Ax - b alone is -0: element 0 below. Everywhere else the two agree."""
    from glx import kernels
    rng = np.random.default_rng(ml + 5)
    Ax, b = _vec(rng, ml, dt), _vec(rng, ml, dt)
    Ax[:8] = [-0.0, -0.0, 0.0, 0.0, 1.5, -1.5, -0.0, 2.0]
    b[:8] = [0.0, -0.0, 0.0, -0.0, 1.5, -1.5, 3.0, 2.0]
    Axd, bd = _dev(Ax), _dev(b)
    got = _host(kernels.admm_rhs(Axd, Axd, bd, 0.0))   # the same tensor: the same pointer twice
    want = ref_admm_v(Ax, Ax, b, 0.0)
    _same_bits(got, want, "v")
    plain = Ax - b
    assert np.signbit(plain[0]) and not np.signbit(want[0]) and not np.signbit(got[0])
    assert np.array_equal(_bits(plain[1:]), _bits(want[1:]))
    _same_bits(got, _host(kernels.admm_rhs(Axd, Axd.clone(), bd, 0.0)), "aliased against a copy")
    _same_bits(_host(Axd), Ax, "the caller's Ax")


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("nl", SIZES_RHS)
def test_admm_primal_rhs(nl, dt):
    from glx import kernels
    rng = np.random.default_rng(nl + 1)
    ATb, x, z = _vec(rng, nl, dt, 30.0), _vec(rng, nl, dt), _vec(rng, nl, dt, 5.0)
    rho = 1e-2
    got = _host(kernels.admm_primal_rhs(_dev(ATb), _dev(x), _dev(z), rho))
    _same_bits(got, ref_primal_w(ATb, x, z, rho), "w")
    if nl >= RHS_TRIP:
        sl = slice(RHS_TRIP - 251, nl)
        part = _host(kernels.admm_primal_rhs(_dev(ATb[sl]), _dev(x[sl]), _dev(z[sl]), rho))
        _same_bits(part, got[sl], "w at the trip boundary")
    i = nl // 2
    x2 = x.copy()
    x2[i] = np.nan
    got2 = _host(kernels.admm_primal_rhs(_dev(ATb), _dev(x2), _dev(z), rho))
    assert np.isnan(got2[i])
    keep = np.arange(nl) != i
    _same_bits(got2[keep], got[keep], "w beside the NaN")


# ---------------------------------------------------------------------------------------------
# k_alm_j
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", SPLITS)
@pytest.mark.parametrize("nl", SIZES_RHS)
def test_alm_j(nl, S):
    from glx import kernels
    rng = np.random.default_rng(nl + 10 * S)
    h = _two_sources(rng, nl, S, np.float64)[:S] * np.where(rng.random(nl) < 0.5, -1.0, 1.0)
    x = _vec(rng, nl, np.float64)
    got = _host(kernels.alm_j(_dev(h), _dev(x), RHO))
    _same_bits(got, ref_alm_j(h, x, RHO), "J")
    if nl >= RHS_TRIP:
        sl = slice(RHS_TRIP - 251, nl)
        part = _host(kernels.alm_j(_dev(h[:, sl]), _dev(x[sl]), RHO))
        _same_bits(part, got[sl], "J at the trip boundary")
    i = nl // 2
    h2 = h.copy()
    h2[S - 1, i] = np.nan
    got2 = _host(kernels.alm_j(_dev(h2), _dev(x), RHO))
    assert np.isnan(got2[i])
    keep = np.arange(nl) != i
    _same_bits(got2[keep], got[keep], "J beside the NaN")


def test_alm_pair_refuses_fp32_and_l33():
    torch = _torch()
    from glx import _lib, kernels
    x = torch.ones((4, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.GlxError) as e:
        kernels.alm_j(x.reshape(-1).clone(), x.reshape(-1), RHO)
    assert e.value.code == 1 and "fp64" in str(e.value)
    with pytest.raises(_lib.GlxError) as e:
        kernels.alm_x(x, x.clone(), x.clone(), 1.0)
    assert e.value.code == 1 and "fp64" in str(e.value)
    # l = 33: refused with a message, nothing written
    x = torch.ones((5, 33), dtype=torch.float64, device="cuda")
    xo, ro = torch.full_like(x, 7.25), torch.full_like(x, -3.5)
    with pytest.raises(_lib.GlxError) as e:
        kernels.alm_x(x, x.clone(), x.clone(), 1.0, x_out=xo, r_out=ro)
    assert e.value.code == 1 and "l <= 32" in str(e.value)
    torch.cuda.synchronize()
    assert bool((xo == 7.25).all()) and bool((ro == -3.5).all()) and bool((x == 1.0).all())


# ---------------------------------------------------------------------------------------------
# k_admm_fin
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("S", SPLITS)
@pytest.mark.parametrize("ml", SIZES_FIN)
def test_admm_fin(ml, S, dt):
    torch = _torch()
    from glx import kernels
    rng = np.random.default_rng(ml + 100 * S)
    P = _two_sources(rng, ml, S, dt)
    b, Au = _vec(rng, ml, dt), _vec(rng, ml, dt)
    ref = ref_admm_fin(P, S, b, Au)
    trips = _trips(ml, 256)
    Pd, bd, Aud = _dev(P), _dev(b), _dev(Au)
    out = kernels.admm_fin(Pd, bd, Aud)
    got = {k: _host(out[k]) for k in ("Ax", "Au", "s")}
    for k in ("Ax", "Au", "s"):
        _same_bits(got[k], ref[k], k)
    _sq_check(_host(out["sums"])[0], ref["sq"], trips, "admm_fin sum " + _tag(dt))
    _same_bits(_host(Aud), Au, "the caller's Au")
    # s == NULL: Ax, Au and the sum as before (the kernel takes no other pointer to write through)
    o2 = kernels.admm_fin(Pd, bd, Aud, s=None)
    assert o2["s"] is None
    _same_bits(_host(o2["Ax"]), got["Ax"], "Ax without s")
    _same_bits(_host(o2["Au"]), got["Au"], "Au without s")
    _same_bits(_host(o2["sums"]), _host(out["sums"]), "sum without s")
    if ml >= FIN_TRIP:
        sl = slice(FIN_TRIP - 251, ml)
        part = kernels.admm_fin(_dev(P[:, sl]), _dev(b[sl]), _dev(Au[sl]))
        for k in ("Ax", "Au", "s"):
            _same_bits(_host(part[k]), got[k][sl], k + " at the trip boundary")
    # one NaN in the second source's last slab: Au+ and s of that element NaN, the sum untouched
    # (it reads Ax); one in the first source's: Ax of that element and the sum NaN
    i = ml // 2
    P2 = P.copy()
    P2[2 * S - 1, i] = np.nan
    o3 = kernels.admm_fin(_dev(P2), bd, Aud)
    assert np.isnan(_host(o3["Au"])[i]) and np.isnan(_host(o3["s"])[i])
    keep = np.arange(ml) != i
    for k in ("Au", "s"):
        _same_bits(_host(o3[k])[keep], got[k][keep], k + " beside the NaN")
    _same_bits(_host(o3["Ax"]), got["Ax"], "Ax with a NaN in the other source")
    _same_bits(_host(o3["sums"]), _host(out["sums"]), "sum with a NaN in the other source")
    P2 = P.copy()
    P2[S - 1, i] = np.nan
    o4 = kernels.admm_fin(_dev(P2), bd, Aud)
    assert np.isnan(_host(o4["Ax"])[i]) and np.isnan(_host(o4["sums"])[0])
    _same_bits(_host(o4["Ax"])[keep], got["Ax"][keep], "Ax beside the NaN")
    for k in ("Au", "s"):
        _same_bits(_host(o4[k]), got[k], k + " with a NaN in the other source")


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_admm_fin_null_s_leaves_a_sentinel(dt):
    """s == NULL beside a sentinel buffer placed where a stray store through s, Ax + ml or Au + ml
    would land: the three outputs sit in one allocation, [Ax | Au | sentinel]."""
    torch = _torch()
    from glx import kernels
    from glx._lib import check, lib
    ml, S = 1025, 3
    rng = np.random.default_rng(3)
    P, b, Au = _two_sources(rng, ml, S, dt), _vec(rng, ml, dt), _vec(rng, ml, dt)
    ref = ref_admm_fin(P, S, b, Au)
    pad = 1024 + (-ml) % 64
    buf = torch.full((3 * (ml + pad),), 12345.0, dtype=_dev(b).dtype, device="cuda")
    Ax, Aud, sent = buf[:ml], buf[ml + pad:2 * ml + pad], buf[2 * (ml + pad):]
    Aud.copy_(_dev(Au))
    Pd, bd = _dev(P), _dev(b)
    sums = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    ws = kernels._ws(kernels._dt(bd), 1, 1, 1, bd.device)
    check(lib().glx_admm_fin(kernels._dt(bd), ml, S, Pd.data_ptr(), bd.data_ptr(), Ax.data_ptr(), Aud.data_ptr(),
                             None, sums.data_ptr(), ws.data_ptr(), ws.numel(), kernels._stream(bd.device)))
    _same_bits(_host(Ax), ref["Ax"], "Ax")
    _same_bits(_host(Aud), ref["Au"], "Au")
    assert bool((sent == 12345.0).all()) and bool((buf[ml:ml + pad] == 12345.0).all())
    assert bool((buf[2 * ml + pad:2 * (ml + pad)] == 12345.0).all())
    _sq_check(_host(sums)[0], ref["sq"], 1, "admm_fin sum " + _tag(dt))


# ---------------------------------------------------------------------------------------------
# k_admm_primal_fin
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("S", SPLITS)
@pytest.mark.parametrize("ml", SIZES_FIN)
def test_admm_primal_fin(ml, S, dt):
    torch = _torch()
    from glx import kernels
    rng = np.random.default_rng(ml + 100 * S + 7)
    rho = 1e-2
    P = _two_sources(rng, ml, S, dt)
    b, AATb = _vec(rng, ml, dt), _vec(rng, ml, dt, 20.0)
    ref = ref_primal_fin(P, S, b, AATb, rho)
    trips = _trips(ml, 256)
    Pd, bd, Ad = _dev(P), _dev(b), _dev(AATb)
    out = kernels.admm_primal_fin(Pd, bd, rho, AATb=Ad)
    got = {k: _host(out[k]) for k in ("Ax", "Az", "v")}
    for k in ("Ax", "Az", "v"):
        _same_bits(got[k], ref[k], k)
    _sq_check(_host(out["sums"])[0], ref["sq"], trips, "primal_fin sum " + _tag(dt))
    # AATb == NULL (the direct form, S slabs): Az and v sentinels untouched, Ax and the sum as before
    Az, v = torch.full_like(bd, 777.0), torch.full_like(bd, -555.0)
    o2 = kernels.admm_primal_fin(_dev(P[:S]), bd, rho, AATb=None, Az=Az, v=v)
    torch.cuda.synchronize()
    assert bool((Az == 777.0).all()) and bool((v == -555.0).all())
    _same_bits(_host(o2["Ax"]), got["Ax"], "Ax, direct")
    _same_bits(_host(o2["sums"]), _host(out["sums"]), "sum, direct")
    if ml >= FIN_TRIP:
        sl = slice(FIN_TRIP - 251, ml)
        part = kernels.admm_primal_fin(_dev(P[:, sl]), _dev(b[sl]), rho, AATb=_dev(AATb[sl]))
        for k in ("Ax", "Az", "v"):
            _same_bits(_host(part[k]), got[k][sl], k + " at the trip boundary")
    i = ml // 2
    keep = np.arange(ml) != i
    P2 = P.copy()
    P2[0, i] = np.nan   # the first source: Ax, v and the sum
    o3 = kernels.admm_primal_fin(_dev(P2), bd, rho, AATb=Ad)
    assert np.isnan(_host(o3["Ax"])[i]) and np.isnan(_host(o3["v"])[i]) and np.isnan(_host(o3["sums"])[0])
    for k in ("Ax", "v"):
        _same_bits(_host(o3[k])[keep], got[k][keep], k + " beside the NaN")
    _same_bits(_host(o3["Az"]), got["Az"], "Az with a NaN in the other source")
    P2 = P.copy()
    P2[S, i] = np.nan   # the second source: Az and v, not the sum
    o4 = kernels.admm_primal_fin(_dev(P2), bd, rho, AATb=Ad)
    assert np.isnan(_host(o4["Az"])[i]) and np.isnan(_host(o4["v"])[i])
    for k in ("Az", "v"):
        _same_bits(_host(o4[k])[keep], got[k][keep], k + " beside the NaN")
    _same_bits(_host(o4["Ax"]), got["Ax"], "Ax with a NaN in the other source")
    _same_bits(_host(o4["sums"]), _host(out["sums"]), "sum with a NaN in the other source")


# ---------------------------------------------------------------------------------------------
# k_alm_x
# ---------------------------------------------------------------------------------------------
def _lpr(l):
    lpr = 1
    while lpr < min(l, 16):
        lpr *= 2
    return lpr


def _alm_x_case(n, l, S, seed):
    torch = _torch()
    from glx import kernels
    rng = np.random.default_rng(seed)
    taurho = TAU * RHO
    x = rng.standard_normal((n, l))
    u = rng.standard_normal((n, l)) * 0.01
    k = np.arange(1, S + 1, dtype=np.float64)[:, None, None]
    g = rng.standard_normal((S, n, l)) * 0.01 * k
    if n > 2:
        x[2], u[2], g[:, 2] = 0.0, 0.0, 0.0   # an all-zero row
    ref = ref_alm_x(x, u, g, taurho)
    per_trip = 512 * 256 // _lpr(l)
    trips = -(-n // per_trip)
    xd, ud, gd = _dev(x), _dev(u), _dev(g)
    out = kernels.alm_x(xd, ud, gd, taurho)
    got = {k_: _host(out[k_]) for k_ in ("x", "r")}
    _same_bits(got["x"], ref["x"], "x+")
    _same_bits(got["r"], ref["r"], "r")
    _same_bits(_host(xd), x, "the caller's x")
    sums = _host(out["sums"])
    xl = ref["x"].astype(np.longdouble)
    norms = np.sqrt(np.sum(xl * xl, axis=1))
    want = float(np.sum(norms))
    bar = C * ((l / 2 + 2) * EPS64 + (CSUM + trips - 1) * EPS64) * want
    _note("alm_x sum", abs(float(sums[0]) - want) / bar)
    assert abs(float(sums[0]) - want) <= bar
    assert float(sums[1]) == float(np.max(np.abs(ref["x"])))
    # in place (the solver's call): every bit of x+, r and both sums
    inp = kernels.alm_x(xd, ud, gd, taurho, in_place=True)
    _same_bits(_host(inp["x"]), got["x"], "x+ in place")
    _same_bits(_host(inp["r"]), got["r"], "r in place")
    _same_bits(_host(inp["sums"]), sums, "sums in place")
    # one NaN: its row's element NaN in r and x+, both sums NaN, every other bit as before
    i, j = n - 1, l // 2
    u2 = u.copy()
    u2[i, j] = np.nan
    o2 = kernels.alm_x(xd, _dev(u2), gd, taurho)
    keep = np.ones((n, l), dtype=bool)
    keep[i, j] = False
    for k_ in ("x", "r"):
        v = _host(o2[k_])
        assert np.isnan(v[i, j])
        _same_bits(v[keep], got[k_][keep], k_ + " beside the NaN")
    assert np.isnan(_host(o2["sums"])).all()
    return x, u, g, got, per_trip


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("l", [1, 2, 3, 5, 8, 16, 17, 32])
@pytest.mark.parametrize("n", [1, 15, 64, 130, 257])
def test_alm_x(n, l, S):
    _alm_x_case(n, l, S, seed=1000 * n + 10 * l + S)


SEVERAL_TRIPS = [(1, 131077), (2, 65541), (3, 32771), (8, 16389), (16, 8200), (17, 8200), (32, 8200)]


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("l,n", SEVERAL_TRIPS)
def test_alm_x_several_trips(l, n, S):
    """Past one trip of the 512-workgroup grid: two trips, the second ragged; the rows on both sides
    of the boundary again in a launch of their own, bit for bit."""
    from glx import kernels
    x, u, g, got, per_trip = _alm_x_case(n, l, S, seed=n + l + S)
    assert -(-n // per_trip) == 2 and 0 < n - per_trip < 256 // _lpr(l)
    rows = slice(per_trip - 251, n)
    part = kernels.alm_x(_dev(x[rows]), _dev(u[rows]), _dev(g[:, rows]), TAU * RHO)
    _same_bits(_host(part["x"]), got["x"][rows], "x+ at the trip boundary")
    _same_bits(_host(part["r"]), got["r"][rows], "r at the trip boundary")
