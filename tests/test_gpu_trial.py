"""The line-search trial kernels, one launch at a time, against a plain NumPy reference.

The trial is the half of an iteration that is not a dense product: prox, hard threshold, the
Armijo / backtracking sums, the row masks of e = p - thr(p) and the column bitmaps the A e gather
walks. It runs in k_prox_pgd, k_fista_trial, k_trial_split and k_fista_split (kernels_elem.hip),
in the fused epilogues k_atr_prox and k_atr_fista (kernels_atr.hip), and in prox_pgd_row,
fista_row, zf_store_panel and zf_store_group16 (glx_device.h). Reached here through
glx_trial_proxgd / glx_trial_fista (glx.kernels.trial_proxgd / trial_fista); no session, no solve.

Reference: the formulas as the reference project states them (ProxGD gl_ProxGD_primal.py:65-74,
89-92; FProxGD gl_FProxGD_primal.py:92-102, 136-145), written below in NumPy (nothing imported from
glx), computed in np.longdouble for f64 inputs and np.float64 for f32 inputs, with the scalars
rounded to the kernel's type first, as the kernel does (t, t*mu, thres, theta, a1 = 1 - theta',
b1 = theta', delta, delta^2).

Bars, with eps = the kernel type's machine epsilon (none is fitted to the kernel):
  p / xc       |got - ref| <= B = 16 eps (|x| + t |g|). The only cancellation is ||w|| - t mu; it
               enters as an absolute error ~ eps ||w|| on a factor <= 1.
  z            B_z = B + 4 eps (|x| + |p|): G_t = (x - p) / t carries (B + 2 eps |x - p|) / t, the
               product t G_t one more eps |x - p|, the last subtraction eps |z|, |z| ~ |p|.
  vnext        B_v = (B + 2 eps (|xc| + |thr(xk)|)) / theta + eps |vnext|.
  ynext        B_y = |a1| B + |b1| B_v + 2 eps (|a1 thr(xc)| + |b1 vnext|).
  G (form 1)   test_gradient_atr_codes' bar: max error <= 1e-13 (f64) or 2e-6 sqrt(m) (f32) times
               the largest accumulated magnitude max(|A|^T |R|).
  sums         term-by-term propagation of B: with B_G = (B + 2 eps |x - p|) / t + eps |G_t|,
               sum g G_t:  sum(|g| B_G + eps |g G_t|);  sum G_t^2: sum(2 |G_t| B_G + B_G^2 + eps G_t^2);
               sum ||p_i||: sum_i(||B_i||_2 + 8 eps ||p_i||) (triangle inequality, then the l
               squares, their <= 11 additions and the root); FISTA the same with xc - y for G_t
               (B_d = B + eps |xc - y|), FGD's smoothed norm with sqrt(||xc_i||^2 + delta^2) for
               ||p_i||. Each plus CSUM eps64 sum|term| for the fp64 accumulation (at most CSUM = 32
               additions deep at one trip: 8 per thread, 8 levels in the workgroup, 12 over the
               workgroup partials). A thread adds up to 8 more terms in every further trip of its
               workgroup, so the several-trip cases take CSUM + 8 (trips - 1): 40 at their two trips.
  max |p|      equal to the maximum of the returned p exactly; NaN when a NaN row is present.
Discrete outputs (pthr, e / ec, the row masks, every column-bitmap word including the padding
groups in [ceil16(n), npad), the two counts) are compared exactly outside an ambiguity set: the
elements where the reference's ||p| - thres| <= B or where w = x - t g could cancel to zero
(0 < |w| <= 2 eps (|x| + t |g|)), and the rows where | ||w|| - thres | or | ||w|| - t mu | is
within 16 eps ||w||. A case whose set holds more than 4 members fails; every case below has 0
(counted on the CPU from the reference alone and asserted again in each test). The counts may
differ from the reference by the set's members, either way.

Every case carries one all-zero row of x and g, one row holding -0.0 and one row holding a NaN. The
NaN would turn three of the sums into NaN, so each case runs twice: with a finite value in place of
the NaN (all the bars above), and with the NaN (every other row bit-identical to the first run,
the row itself NaN, the sums NaN, the counts exact).

The row kernels' cases by layout. A row of l values is held by LPR lanes with EPL values each
(dispatch_row: LPR = the power of two >= l up to 16, then EPL = ceil(l / 16) at LPR 16), so the l of
test_row_kernels select (LPR, EPL) =
  l = 1 (1, 1)   2 (2, 1)   3 (4, 1)   5, 8 (8, 1)   16 (16, 1)   17, 32 (16, 2)   40 (16, 3)
  64 (16, 4)   72 (16, 5)   88 (16, 6)   104 (16, 7)   128 (16, 8)
which is every instantiation; 3, 5, 17, 40, 72, 88 and 104 leave lanes or a row's last elements
without a value. test_replicated_halves_match_row_kernels runs k_trial_split at (4, 1) and at every
(16, EPL). All of those are one trip of at most 63 workgroups. test_row_kernels_several_trips runs
(l, n) = (1, 131077), (2, 65541), (3, 32771), (8, 16389), (16, 8200), (128, 8200): LPR 1, 2, 4, 8 and
LPR 16 at EPL 1 and 8, each 5 to 8 rows past the 512 * 256 / LPR rows that the capped grid of 512
workgroups takes in one trip, so two trips, the second ragged, and the rows on both sides of the
boundary bit-identical to a launch of their own (test_split_candidate_outputs makes the same two
trips at n = 8200 for the split outputs).

Measured on an MI355X, worst error / bound over all cases of this file (f64, f32); the module
prints the table and the ambiguity sets' sizes when its tests are over (pytest -s):
  p            0.131  0.130      xc           0.136  0.130      z            0.140  0.140
  vnext        0.432  0.427      ynext        0.301  0.296      G (form 1)   0.0044 0.0104
  sum g*Gt     0.0190 0.0283     sum Gt^2     0.0189 0.0271     sum |p_i|    0.0280 0.0176
  sum g*d      0.0286 0.0293     sum d^2      0.0239 0.0268     sum |xc_i|   0.0280 0.0168
  sum smooth   0.0182 0.0094
None is above 1 and none below 1e-3, so the constants stand as derived. Ambiguity sets: 0 members
in every case (largest set 0 over the 1248 references built; a several-trip case takes the first of
its seeds whose set, counted on the CPU from the reference alone, is empty).

What a one-line slip would trip (each tried on a NumPy model of the kernels' arithmetic put in
place of the library, never as device code):
  `pv[e] != T(0)` dropped from `ch` in prox_pgd_row   counts and masks: test_row_kernels[proxgd],
                                                      test_split_candidate_outputs, test_fused_epilogues
  `<=` for `<` in the threshold compare               test_threshold_edge_is_strict
  the tail group's store skipped in zf_store_group16  test_split_candidate_outputs (n % 16 != 0),
                                                      test_stale_words_row_kernels
  add for max in slot 3 of the ProxGD sums            `max |p|` in test_row_kernels,
                                                      test_split_candidate_outputs, test_fused_epilogues
  a1 and b1 swapped in fista_row                      ynext in test_row_kernels[fista, fgd],
                                                      test_split_candidate_outputs, test_fused_epilogues
  one sum off by 1e-10 relative                       the sums' bars in the same three tests
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda"
T_STEP, THRES = 0.37, 1e-3
MUS = (0.02, 2e-4)
THETA, THETA_NEXT, DELTA = 2.0 / 7.0, 2.0 / 8.0, 1e-4
CSUM = 32
EPS64 = float(np.finfo(np.float64).eps)
MAX_AMBIGUOUS = 4
# l -> (lanes per row, elements per lane) of dispatch_row: 1 (1, 1), 2 (2, 1), 3 (4, 1), 5 and 8
# (8, 1), 16 (16, 1), 17 and 32 (16, 2), 40 (16, 3), 64 (16, 4), 72 (16, 5), 88 (16, 6), 104 (16, 7),
# 128 (16, 8); 3, 5, 17, 40, 72, 88 and 104 leave lanes or tail elements of a row without a value
ROW_LS = [1, 2, 3, 5, 8, 16, 17, 32, 40, 64, 72, 88, 104, 128]
# one n past a single trip of 512 workgroups (512 * 256 / LPR rows) per lanes-per-row layout
MULTI_TRIP = [(1, 131077), (2, 65541), (3, 32771), (8, 16389), (16, 8200), (128, 8200)]

# worst error / bound per (output, dtype) and the ambiguity sets' sizes, printed when the module's
# tests are over (pytest -s)
RATIOS = {}
AMBIGUOUS = {"references": 0, "largest set": 0, "members in all": 0}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(RATIOS):
        print("ratio %-14s %s  %.3e" % (key[0], key[1], RATIOS[key]))
    print("ambiguity sets:", AMBIGUOUS)


def _k():
    from glx import kernels
    return kernels


def _types(dtype):
    return (np.float64, np.longdouble) if dtype == "f64" else (np.float32, np.float64)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(a, b, where=None):
    eq = _bits(a) == _bits(b)
    return bool(eq.all() if where is None else eq[where].all())


def _note(name, dtype, r):
    RATIOS[(name, dtype)] = max(RATIOS.get((name, dtype), 0.0), r)


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def _gen(n, l, dtype, seed):
    """The issue's generator: rows of x at four scales (a quarter all-zero), rows of g at four."""
    npdt = _types(dtype)[0]
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, l)) * rng.choice([0, 1e-3, 3e-2, 1.0], (n, 1), p=[.25, .25, .3, .2])
    g = rng.standard_normal((n, l)) * rng.choice([1e-4, 1e-2, 1.0, 30.0], (n, 1))
    xk = rng.standard_normal((n, l)) * rng.choice([0, 1e-3, 3e-2, 1.0], (n, 1), p=[.25, .25, .3, .2])
    return x.astype(npdt), g.astype(npdt), xk.astype(npdt)


def _special_rows(x, g=None):
    """Row n-3 all zero (x and g), row n-1 = -0.0 in x (and one -0.0 in g); returns where the NaN
    variant puts its NaN (row n-2)."""
    n, l = x.shape
    x[n - 3] = 0.0
    x[n - 1] = -0.0
    if g is not None:
        g[n - 3] = 0.0
        g[n - 1, 0] = -0.0
    return n - 2, l // 2


def _with_nan(x, pos):
    xn = x.copy()
    xn[pos] = np.nan
    return xn


# ---------------------------------------------------------------------------------------------
# the reference (plain NumPy, the compute type one step wider than the kernel's)
# ---------------------------------------------------------------------------------------------
def _prox_th(w, tmu, th):
    """gl_ProxGD_primal.py:65-71 (the same function at gl_FProxGD_primal.py:71-77)."""
    nrm = np.sqrt((w * w).sum(axis=1, keepdims=True))
    return w * np.clip(nrm - tmu, 0, None) / ((nrm < th) + nrm), nrm


def _ambiguous(p, w, nrm, mag, th, tmu, eps, prox=True):
    B = 16 * eps * mag
    amb_e = (np.abs(np.abs(p) - th) <= B) | ((w != 0) & (np.abs(w) <= 2 * eps * mag))
    amb_r = np.zeros(p.shape[0], dtype=bool)
    if prox:
        amb_r = ((np.abs(nrm - th) <= 16 * eps * nrm) | (np.abs(nrm - tmu) <= 16 * eps * nrm))[:, 0]
    return amb_e, amb_r


def ref_proxgd(x, g, t, mu, thres, csum=CSUM):
    npdt = x.dtype.type
    C = np.longdouble if npdt is np.float64 else np.float64
    eps = C(np.finfo(npdt).eps)
    tT, tmu, th = C(npdt(t)), C(npdt(t * mu)), C(npdt(thres))
    X, Gd = x.astype(C), g.astype(C)
    w = X - tT * Gd
    p, nrm = _prox_th(w, tmu, th)
    Gt = (X - p) / tT                      # gl_ProxGD_primal.py:73-74
    z = X - tT * Gt                        # :91
    small = np.abs(p) < th                 # :127 on the candidate
    ch = small & (p != 0)
    mag = np.abs(X) + tT * np.abs(Gd)
    B = 16 * eps * mag
    amb_e, amb_r = _ambiguous(p, w, nrm, mag, th, tmu, eps)
    BG = (B + 2 * eps * np.abs(X - p)) / tT + eps * np.abs(Gt)
    pn = np.sqrt((p * p).sum(axis=1))
    terms = [Gd * Gt, Gt * Gt, pn]
    bnds = [np.abs(Gd) * BG + eps * np.abs(Gd * Gt), 2 * np.abs(Gt) * BG + BG * BG + eps * Gt * Gt,
            np.sqrt((B * B).sum(axis=1)) + 8 * eps * pn]
    # a row on the ||w|| = thres step may take the other denominator: |dp| <= |w|
    slack = [np.abs(Gd) * np.abs(w) / tT, (2 * np.abs(Gt) + np.abs(w) / tT) * np.abs(w) / tT,
             np.sqrt((w * w).sum(axis=1))]
    sums, sbnd = [], []
    for k in range(3):
        sums.append(terms[k].sum())
        sbnd.append(bnds[k].sum() + csum * EPS64 * np.abs(terms[k]).sum() + slack[k][amb_r].sum())
    return dict(p=p, z=z, small=small, ch=ch, B=B, Bz=B + 4 * eps * (np.abs(X) + np.abs(p)),
                amb_e=amb_e, amb_r=amb_r, sums=sums, sbnd=sbnd, th=th, eps=eps)


def ref_fista(y, g, xk, t, mu, thres, theta, theta_next, delta, prox, csum=CSUM):
    npdt = y.dtype.type
    C = np.longdouble if npdt is np.float64 else np.float64
    eps = C(np.finfo(npdt).eps)
    tT, tmu, th = C(npdt(t)), C(npdt(t * mu)), C(npdt(thres))
    thT, a1, b1 = C(npdt(theta)), C(npdt(1.0 - theta_next)), C(npdt(theta_next))
    dd, dl_ = C(npdt(delta * delta)), C(npdt(delta))
    Y, Gd, XK = y.astype(C), g.astype(C), xk.astype(C)
    w = Y - tT * Gd
    if prox:
        xc, nrm = _prox_th(w, tmu, th)     # gl_FProxGD_primal.py:95 / :144
    else:
        xc, nrm = w, np.sqrt((w * w).sum(axis=1, keepdims=True))   # FGD: the identity prox
    d = xc - Y
    small = np.abs(xc) < th
    ch = small & (xc != 0)
    xo = np.where(np.abs(XK) < th, C(0), XK)           # :136
    vn = xo + (xc - xo) / thT                          # :145
    pt = np.where(small, C(0), xc)                     # :136 of the next step
    yn = a1 * pt + b1 * vn                             # :139 of the next step
    mag = np.abs(Y) + tT * np.abs(Gd)
    B = 16 * eps * mag
    amb_e, amb_r = _ambiguous(xc, w, nrm, mag, th, tmu, eps, prox)
    Bv = (B + 2 * eps * (np.abs(xc) + np.abs(xo))) / thT + eps * np.abs(vn)
    By = np.abs(a1) * B + np.abs(b1) * Bv + 2 * eps * (np.abs(a1 * pt) + np.abs(b1 * vn))
    Bd = B + eps * np.abs(d)
    ps = (xc * xc).sum(axis=1)
    Bn = np.sqrt((B * B).sum(axis=1))
    terms = [Gd * d, d * d]
    bnds = [np.abs(Gd) * Bd + eps * np.abs(Gd * d), 2 * np.abs(d) * Bd + Bd * Bd + eps * d * d]
    slack = [np.abs(Gd) * np.abs(w), (2 * np.abs(d) + np.abs(w)) * np.abs(w)]
    wn = np.sqrt((w * w).sum(axis=1))
    if not prox:
        sm = np.sqrt(ps + dd)
        terms.append(sm - dl_)
        bnds.append(Bn + 8 * eps * sm)
        slack.append(wn)
    terms.append(np.sqrt(ps))
    bnds.append(Bn + 8 * eps * np.sqrt(ps))
    slack.append(wn)
    sums, sbnd = [], []
    for k in range(len(terms)):
        sums.append(terms[k].sum())
        sbnd.append(bnds[k].sum() + csum * EPS64 * np.abs(terms[k]).sum() + slack[k][amb_r].sum())
    return dict(xc=xc, vn=vn, yn=yn, small=small, ch=ch, B=B, Bv=Bv, By=By, amb_e=amb_e, amb_r=amb_r,
                sums=sums, sbnd=sbnd, th=th, eps=eps)


def ref_zf(ch, n):
    """The zf buffer of a mask-writing trial on a zeroed buffer, as bits: rows[k][c] (npad x 32) and
    cols[c][k] (32 x npad), both = ch padded with zeros (glx.h: the row masks, then per column c the
    u16 words of npad / 16 row groups)."""
    npad = (n + 63) // 64 * 64
    rows = np.zeros((npad, 32), dtype=bool)
    rows[:n, :ch.shape[1]] = ch
    return rows, rows.T.copy()


def unpack_zf(zf, n):
    npad = (n + 63) // 64 * 64
    words = np.ascontiguousarray(zf).view(np.uint32)
    assert words.size == 2 * npad
    rows = ((words[:npad, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool)
    bm = words[npad:].view(np.uint16).reshape(32, npad // 16)
    cols = ((bm[:, :, None] >> np.arange(16, dtype=np.uint16)) & 1).astype(bool).reshape(32, npad)
    return rows, cols


# ---------------------------------------------------------------------------------------------
# checks (NumPy arrays in, so they run without a device)
# ---------------------------------------------------------------------------------------------
def _check_close(name, dtype, got, ref, bound, skip_rows):
    assert np.array_equal(np.isnan(got), np.isnan(ref)), name
    v = ~np.isnan(ref) & ~skip_rows[:, None]
    err = np.abs(got.astype(ref.dtype) - ref)
    assert not (err[v & (bound == 0)] != 0).any(), name
    nz = v & (bound > 0)
    r = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    _note(name, dtype, r)
    assert r <= 1.0, (name, dtype, r)


def _amb_count(ref):
    c = int(ref["amb_e"].sum()) + int(ref["amb_r"].sum())
    AMBIGUOUS["references"] += 1
    AMBIGUOUS["largest set"] = max(AMBIGUOUS["largest set"], c)
    AMBIGUOUS["members in all"] += c
    assert c <= MAX_AMBIGUOUS, "ambiguity set holds %d members" % c
    return c


def _check_discrete(ref, p_got, pthr, e, zf, n, counts=None):
    """pthr / e / masks / bitmaps / counts from the reference's decisions and the returned p."""
    amb = ref["amb_e"] | ref["amb_r"][:, None]
    ok = ~amb
    zero = np.zeros_like(p_got)
    small, ch = ref["small"], ref["ch"]
    assert _same_bits(pthr, np.where(small, zero, p_got), ok), "pthr"
    if e is not None:
        assert _same_bits(e, np.where(small, p_got, zero), ok), "e"
    if zf is not None:
        rows, cols = unpack_zf(zf, n)
        erows, ecols = ref_zf(ch, n)
        okp = np.ones_like(erows)
        okp[:n, :ch.shape[1]] = ok
        assert np.array_equal(rows[okp], erows[okp]), "row masks"
        assert np.array_equal(cols[okp.T], ecols[okp.T]), "column bitmaps"
    if counts is not None:
        lo4 = int((ch & ok).sum())
        assert lo4 <= counts[0] <= lo4 + int(amb.sum()), ("acc[4]", counts[0], lo4)
        sure = (ch & ok).any(axis=1)
        lo5 = int(sure.sum())
        assert lo5 <= counts[1] <= lo5 + int((amb.any(axis=1) & ~sure).sum()), ("acc[5]", counts[1], lo5)


def _check_sums(names, dtype, got, ref):
    for k, name in enumerate(names):
        err = abs(np.longdouble(got[k]) - np.longdouble(ref["sums"][k]))
        bound = np.longdouble(ref["sbnd"][k])
        r = float(err / bound) if bound > 0 else (0.0 if err == 0 else np.inf)
        _note(name, dtype, r)
        assert r <= 1.0, (name, dtype, r, float(got[k]), float(ref["sums"][k]))


def check_proxgd(dtype, out, ref, n, emode):
    """out: NumPy arrays of one trial_proxgd call (p, pthr, z, sums, zf) on NaN-free inputs."""
    _amb_count(ref)
    _check_close("p", dtype, out["p"], ref["p"], ref["B"], ref["amb_r"])
    if not emode:
        _check_close("z", dtype, out["z"], ref["z"], ref["Bz"], ref["amb_r"])
    s = out["sums"]
    _check_discrete(ref, out["p"], out["pthr"], out["z"] if emode else None, out["zf"] if emode else None,
                    n, counts=(s[4], s[5]))
    _check_sums(("sum g*Gt", "sum Gt^2", "sum |p_i|"), dtype, s, ref)
    assert s[3] == np.abs(out["p"]).max(), "max |p|"


def check_fista(dtype, out, ref, n, prox, split):
    _amb_count(ref)
    skip = ref["amb_r"]
    _check_close("xc", dtype, out["xc"], ref["xc"], ref["B"], skip)
    _check_close("vnext", dtype, out["vnext"], ref["vn"], ref["Bv"], skip)
    amb = ref["amb_e"] | skip[:, None]            # thr(xc) inside y_next is a discrete decision
    _check_close("ynext", dtype, np.where(amb, np.nan, out["ynext"]).astype(out["ynext"].dtype),
                 np.where(amb, np.nan, ref["yn"]), ref["By"], skip)
    if split:
        zero = np.zeros_like(out["xc"])
        _check_discrete(ref, out["xc"], np.where(ref["small"], zero, out["xc"]), out["ec"], out["zf"], n)
    s = out["sums"]
    names = ("sum g*d", "sum d^2", "sum |xc_i|") if prox else ("sum g*d", "sum d^2", "sum smooth", "sum |xc_i|")
    _check_sums(names, dtype, s, ref)
    assert s[-1] == np.abs(out["xc"]).max(), "max |xc|"


def check_nan_variant(clean, nan, nanrow, value_keys, zero_keys, nsum, ref_ch=None):
    """The same call with a NaN in one row: every other row keeps its bits, the row itself is NaN
    (e / ec: 0, its mask 0), the sums NaN, the max NaN, the counts those of the other rows."""
    rows = np.arange(clean[value_keys[0]].shape[0]) != nanrow
    for key in value_keys + zero_keys:
        assert _same_bits(clean[key][rows], nan[key][rows]), key
    for key in value_keys:
        assert np.isnan(nan[key][nanrow]).all(), key
    for key in zero_keys:
        assert _same_bits(nan[key][nanrow], np.zeros_like(nan[key][nanrow])), key
    assert np.isnan(nan["sums"][:nsum]).all()
    if nan.get("zf") is not None:
        n = rows.size
        r0, c0 = unpack_zf(clean["zf"], n)
        r1, c1 = unpack_zf(nan["zf"], n)
        r0[nanrow] = False
        c0[:, nanrow] = False
        assert np.array_equal(r0, r1) and np.array_equal(c0, c1)
    if ref_ch is not None:   # ProxGD's counts (acc[4], acc[5]); callers pass it only with an empty set
        other = ref_ch[rows]
        assert nan["sums"][4] == other.sum() and nan["sums"][5] == other.any(axis=1).sum()


def _out_np(o):
    return {k: _np(v) for k, v in o.items()}


def run_proxgd(x, g, mu, **kw):
    return _out_np(_k().trial_proxgd(_dev(x), _dev(g), T_STEP, mu, THRES, **kw))


def run_fista(y, g, xk, mu, **kw):
    return _out_np(_k().trial_fista(_dev(y), _dev(g), _dev(xk), T_STEP, mu, THETA, THETA_NEXT, THRES, DELTA, **kw))


def proxgd_case(dtype, x, g, mu, n, emode, nanpos, ref=None, **kw):
    """Both variants of one ProxGD case with all its checks; returns the clean run's outputs.
    ref: the reference of (x, g), where the caller has built it already."""
    out = run_proxgd(x, g, mu, emode=emode, **kw)
    if ref is None:
        ref = ref_proxgd(x, out["G"] if kw.get("form") == 1 else g, T_STEP, mu, THRES)
    check_proxgd(dtype, out, ref, n, emode)
    nan = run_proxgd(_with_nan(x, nanpos), g, mu, emode=emode, **kw)
    exact = _amb_count(ref) == 0
    check_nan_variant(out, nan, nanpos[0], ["p", "pthr"] + ([] if emode else ["z"]), ["z"] if emode else [], 4,
                      ref["ch"] if exact else None)
    return out, ref


def fista_case(dtype, y, g, xk, mu, n, prox, split, nanpos, ref=None, **kw):
    out = run_fista(y, g, xk, mu, prox=prox, split=split, **kw)
    if ref is None:
        ref = ref_fista(y, out["G"] if kw.get("form") == 1 else g, xk, T_STEP, mu, THRES, THETA, THETA_NEXT, DELTA,
                        prox)
    check_fista(dtype, out, ref, n, prox, split)
    nan = run_fista(_with_nan(y, nanpos), g, xk, mu, prox=prox, split=split, **kw)
    nsum = 4 if prox else 5
    if not prox:   # FGD has no row norm in xc: only the NaN element itself is NaN
        assert np.isnan(nan["xc"][nanpos]) and np.isnan(nan["sums"]).all()
        keep = np.ones(out["xc"].shape, dtype=bool)
        keep[nanpos] = False
        for key in ("xc", "vnext", "ynext"):
            assert _same_bits(out[key], nan[key], keep), key
        return out, ref
    check_nan_variant(out, nan, nanpos[0], ["xc", "vnext", "ynext"], ["ec"] if split else [], nsum)
    return out, ref


# ---------------------------------------------------------------------------------------------
# row kernels: every lanes-per-row / elements-per-lane instantiation, one and several workgroups
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu", MUS)
@pytest.mark.parametrize("n", [17, 1000])
@pytest.mark.parametrize("l", ROW_LS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["proxgd", "fista", "fgd"])
def test_row_kernels(kind, dtype, l, n, mu):
    x, g, xk = _gen(n, l, dtype, seed=1000 * l + n)
    nanpos = _special_rows(x, g)
    if kind == "proxgd":
        proxgd_case(dtype, x, g, mu, n, False, nanpos)
    else:
        fista_case(dtype, x, g, xk, mu, n, kind == "fista", False, nanpos)


def _lpr(l):
    lpr = 1
    while lpr < min(l, 16):
        lpr *= 2
    return lpr


def _several_trip_inputs(kind, dtype, l, n, mu, csum):
    """The case's inputs and reference: the first of the seeds 1000 l + n, + 100003, ... whose
    ambiguity set, counted from the reference alone, is empty (with f32 and 10^5 .. 10^6 elements a
    seed may leave an element within B of thres)."""
    for k in range(16):
        x, g, xk = _gen(n, l, dtype, seed=1000 * l + n + 100003 * k)
        nanpos = _special_rows(x, g)
        if kind == "proxgd":
            ref = ref_proxgd(x, g, T_STEP, mu, THRES, csum=csum)
        else:
            ref = ref_fista(x, g, xk, T_STEP, mu, THRES, THETA, THETA_NEXT, DELTA, kind == "fista", csum=csum)
        if not (ref["amb_e"].any() or ref["amb_r"].any()):
            return x, g, xk, nanpos, ref
    raise AssertionError("no seed with an empty ambiguity set")


@pytest.mark.parametrize("l,n", MULTI_TRIP)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["proxgd", "fista", "fgd"])
def test_row_kernels_several_trips(kind, dtype, l, n):
    """One n past a single trip of the 512-workgroup grid per lanes-per-row layout: the last
    workgroups make a second, ragged trip (5 to 8 rows). The sums' bars take CSUM + 8 per further
    trip (a thread adds up to 8 more terms in each). Then the rows on both sides of the trip
    boundary run again as a case of their own, in one trip: a row's outputs depend on neither n nor
    the trip, so they come back bit for bit."""
    per_trip = 512 * 256 // _lpr(l)
    trips = -(-n // per_trip)
    assert trips == 2 and 0 < n - per_trip < 256 // _lpr(l)
    mu = MUS[(l + len(kind)) % 2]
    x, g, xk, nanpos, ref = _several_trip_inputs(kind, dtype, l, n, mu, CSUM + 8 * (trips - 1))
    rows = slice(per_trip - 251, n)
    if kind == "proxgd":
        out, _ = proxgd_case(dtype, x, g, mu, n, False, nanpos, ref=ref)
        part = run_proxgd(x[rows].copy(), g[rows].copy(), mu, emode=False)
        same = ("p", "pthr", "z")
    else:
        out, _ = fista_case(dtype, x, g, xk, mu, n, kind == "fista", False, nanpos, ref=ref)
        part = run_fista(x[rows].copy(), g[rows].copy(), xk[rows].copy(), mu, prox=kind == "fista")
        same = ("xc", "vnext", "ynext")
    for key in same:
        assert _same_bits(out[key][rows], part[key]), key


# ---------------------------------------------------------------------------------------------
# split-candidate outputs: e / ec, the row masks and the column bitmaps at every ragged tail
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu", MUS)
# (8200: past the 512-workgroup cap of the row kernels, so a workgroup makes a second trip whose
# 16-row groups lie partly in the padding below npad and partly beyond it, where nothing is stored)
@pytest.mark.parametrize("n", [16, 17, 63, 64, 65, 1000, 2063, 8200])
@pytest.mark.parametrize("l", [16, 32])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["proxgd", "fista"])
def test_split_candidate_outputs(kind, dtype, l, n, mu):
    x, g, xk = _gen(n, l, dtype, seed=77 * l + n)
    nanpos = _special_rows(x, g)
    if kind == "proxgd":
        out, ref = proxgd_case(dtype, x, g, mu, n, True, nanpos)
    else:
        out, ref = fista_case(dtype, x, g, xk, mu, n, True, True, nanpos)
    assert n < 1000 or ref["ch"].any(axis=1).sum() > n // 8     # the large cases flag many rows


@pytest.mark.parametrize("l", [1, 16])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_threshold_edge_is_strict(dtype, l):
    """|p| == thres exactly is kept: the compare is np.abs(x) < thres (gl_ProxGD_primal.py:127).
    Rows with one nonzero entry x0 within 8 ulps of +-thres, g = 0 and mu = 0: then ||w|| = |x0|
    exactly (the root of a correctly rounded square) and p = fl(fl(x0 |x0|) / d) with
    d = (|x0| < thres) + |x0|: IEEE operations NumPy repeats in the kernel's type, so the
    expectation is exact. Some rows land on thres itself; the rows below it take the other
    denominator and are zeroed."""
    npdt = _types(dtype)[0]
    th = npdt(THRES)
    x0 = [th]
    for _ in range(8):
        x0 = [np.nextafter(x0[0], npdt(0))] + x0 + [np.nextafter(x0[-1], npdt(1))]
    x0 = np.array(x0 + [-v for v in x0], dtype=npdt)
    n = x0.size
    x = np.zeros((n, l), dtype=npdt)
    x[:, l // 2] = x0
    g = np.zeros_like(x)
    p = np.zeros_like(x)
    p[:, l // 2] = (x0 * np.abs(x0)) / ((np.abs(x0) < th).astype(npdt) + np.abs(x0))
    small = np.abs(p) < th
    assert (np.abs(p) == th).any() and small.any() and (~small[:, l // 2]).any()
    ch = small & (p != 0)
    zero = np.zeros_like(p)
    o = run_proxgd(x, g, 0.0, emode=False)
    assert _same_bits(o["p"], p) and _same_bits(o["pthr"], np.where(small, zero, p))
    assert o["sums"][4] == ch.sum() and o["sums"][5] == ch.any(axis=1).sum()
    f = run_fista(x, g, x, 0.0)
    a1, b1, theta = npdt(1.0 - THETA_NEXT), npdt(THETA_NEXT), npdt(THETA)
    xo = np.where(np.abs(x) < th, npdt(0), x)
    vn = xo + (p - xo) / theta
    assert _same_bits(f["xc"], p) and _same_bits(f["vnext"], vn)
    assert _same_bits(f["ynext"], a1 * np.where(small, npdt(0), p) + b1 * vn)
    if l == 16:
        oe = run_proxgd(x, g, 0.0, emode=True)
        assert _same_bits(oe["z"], np.where(small, p, zero))
        _assert_zf(oe["zf"], ch, n)
        fe = run_fista(x, g, x, 0.0, split=True)
        assert _same_bits(fe["ec"], np.where(small, p, zero))
        _assert_zf(fe["zf"], ch, n)


# ---------------------------------------------------------------------------------------------
# fused epilogues of A^T R (form 1)
# ---------------------------------------------------------------------------------------------
FUSED_SHAPES = [(8, 64, 16), (100, 128, 32), (256, 2048, 32), (2052, 2048, 16)]
# (tile, dtypes its `fused` field names, K splits it takes with a fused trial)
FUSED_TILES = [(8, ("f64",), (1, 2, 3, 8)), (1008, ("f64", "f32"), (1, 2, 3, 8)),
               (1028, ("f64", "f32"), (1, 2, 3, 8)), (38, ("f64",), (1,)), (1038, ("f64",), (1,))]
FUSED_CASES = [(tile, dt, S) for tile, dts, Ss in FUSED_TILES for dt in dts for S in Ss]
_atr_cache = {}


def _atr_inputs(shape, dtype):
    """A, R with G = A^T R on the generator's row scales (column i of A carries row i's), x, xk;
    made once per (shape, dtype) and left unchanged."""
    key = (shape, dtype)
    if key not in _atr_cache:
        m, n, l = shape
        npdt = _types(dtype)[0]
        x, _, xk = _gen(n, l, dtype, seed=m + 3 * n + l)
        rng = np.random.default_rng(m * n + l)
        sg = rng.choice([1e-4, 1e-2, 1.0, 30.0], n)
        A = (rng.standard_normal((m, n)) * (sg / np.sqrt(m))).astype(npdt)
        R = rng.standard_normal((m, l)).astype(npdt)
        A[:, n - 3] = 0.0
        nanpos = _special_rows(x)
        Ad, Rd = _dev(A), _dev(R)
        gref = Ad.double().T @ Rd.double()
        gmag = float((Ad.double().abs().T @ Rd.double().abs()).max())
        _atr_cache[key] = (x, xk, Ad, Rd, gref, gmag, nanpos)
    return _atr_cache[key]


def _check_G(dtype, m, G, gref, gmag):
    rel = float((torch.from_numpy(G).to(gref.device).double() - gref).abs().max()) / gmag
    tol = 1e-13 if dtype == "f64" else 2e-6 * (m ** 0.5)
    _note("G (form 1)", dtype, rel / tol)
    assert rel < tol, (rel, tol)


@pytest.mark.parametrize("shape", FUSED_SHAPES)
@pytest.mark.parametrize("tile,dtype,S", FUSED_CASES)
@pytest.mark.parametrize("kind", ["proxgd", "fista"])
def test_fused_epilogues(monkeypatch, kind, tile, dtype, S, shape):
    monkeypatch.setenv("GLX_ATR_VARIANT", str(tile))
    monkeypatch.setenv("GLX_ATR_S", str(S))
    monkeypatch.delenv("GLX_ATR_FUSE_SPLIT", raising=False)
    m, n, l = shape
    x, xk, A, R, gref, gmag, nanpos = _atr_inputs(shape, dtype)
    mu = MUS[(tile + S) % 2]
    for zf in (False, True):
        kw = dict(form=1, A=A, R=R)
        if kind == "proxgd":
            o1, _ = proxgd_case(dtype, x, None, mu, n, zf, nanpos, **kw)
            o0 = run_proxgd(x, o1["G"], mu, emode=zf)
            o2 = run_proxgd(x, None, mu, emode=zf, **kw)
            same = ("p", "pthr", "z")
        else:
            o1, _ = fista_case(dtype, x, None, xk, mu, n, True, zf, nanpos, **kw)
            o0 = run_fista(x, o1["G"], xk, mu, split=zf)
            o2 = run_fista(x, None, xk, mu, split=zf, **kw)
            same = ("xc", "vnext", "ynext") + (("ec",) if zf else ())
        _check_G(dtype, m, o1["G"], gref, gmag)
        for key in same:            # the epilogue computes the row kernel's bits from its own G
            assert _same_bits(o1[key], o0[key]), (key, zf)
        if zf:
            assert np.array_equal(o1["zf"], o0["zf"])
        for key in same + ("G", "sums"):   # and the same bits again on a second call
            assert _same_bits(o1[key], o2[key]), (key, zf)


def test_fused_epilogue_refuses_inadmissible_plan():
    from glx import _lib
    x, g, xk = _gen(96, 8, "f64", seed=5)
    A = _dev(np.ones((16, 96)))
    R = _dev(np.ones((16, 8)))
    with pytest.raises(_lib.GlxError) as ei:
        _k().trial_proxgd(_dev(x), None, T_STEP, MUS[0], THRES, form=1, A=A, R=R)
    assert ei.value.code == 1      # GLX_E_INVALID
    with pytest.raises(_lib.GlxError) as ei:
        _k().trial_fista(_dev(x), None, _dev(xk), T_STEP, MUS[0], THETA, THETA_NEXT, THRES, form=1, A=A, R=R)
    assert ei.value.code == 1


# ---------------------------------------------------------------------------------------------
# replicated halves of the row-sharded schedules (form 2)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [17, 1000])
@pytest.mark.parametrize("l", [3, 16, 17, 32, 40, 64, 72, 88, 104, 128])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_replicated_halves_match_row_kernels(dtype, l, n):
    x, g, xk = _gen(n, l, dtype, seed=31 * l + n)
    _special_rows(x, g)
    k = _k()
    mu = MUS[1]
    masks = l in (16, 32)
    oz = run_proxgd(x, g, mu, emode=False)
    zf0 = torch.zeros(k.trial_mask_words(n), dtype=torch.int32, device=DEV) if masks else None
    sz = _out_np(k.trial_proxgd(_dev(x), None, T_STEP, mu, THRES, form=2, emode=False, p=_dev(oz["p"]), zf=zf0))
    assert _same_bits(sz["pthr"], oz["pthr"]) and _same_bits(sz["z"], oz["z"])
    if masks:
        oe = run_proxgd(x, g, mu, emode=True)
        se = _out_np(k.trial_proxgd(_dev(x), None, T_STEP, mu, THRES, form=2, emode=True, p=_dev(oe["p"])))
        assert _same_bits(oe["p"], oz["p"])
        assert _same_bits(se["pthr"], oe["pthr"]) and _same_bits(se["z"], oe["z"])
        assert np.array_equal(se["zf"], oe["zf"]) and np.array_equal(sz["zf"], oe["zf"])
    of = run_fista(x, g, xk, mu)
    sf = _out_np(k.trial_fista(None, None, _dev(xk), T_STEP, mu, THETA, THETA_NEXT, THRES, form=2,
                               xc=_dev(of["xc"])))
    assert _same_bits(sf["vnext"], of["vnext"]) and _same_bits(sf["ynext"], of["ynext"])


def _hand_values(npdt):
    th = npdt(THRES)
    tiny = np.nextafter(npdt(0), npdt(1))
    vals = [th, -th, np.nextafter(th, npdt(0)), np.nextafter(th, npdt(np.inf)), npdt(0.0), npdt(-0.0), tiny,
            npdt(np.inf), npdt(np.nan), -np.nextafter(th, npdt(0)), -np.nextafter(th, npdt(np.inf)), -tiny,
            npdt(-np.inf), npdt(0.5)]
    return np.array(vals, dtype=npdt)


@pytest.mark.parametrize("l", [16, 32])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_replicated_halves_hand_built(dtype, l):
    """p made of the threshold's edge values: +-thres and its two neighbours, +-0, the smallest
    subnormal, inf, NaN. The kernel's type does all the arithmetic here, so NumPy in that type is
    the exact expectation: thr keeps |v| >= thres, inf and NaN; a mask bit is a zeroed NONZERO
    entry (a subnormal counts, a signed zero does not)."""
    npdt = _types(dtype)[0]
    k = _k()
    vals = _hand_values(npdt)
    n = 33
    p = vals[(np.arange(n)[:, None] * 5 + np.arange(l)[None, :] * 3) % vals.size]
    xt = vals[(np.arange(n)[:, None] * 3 + np.arange(l)[None, :] * 7 + 4) % vals.size]
    th, t = npdt(THRES), npdt(T_STEP)
    small = np.abs(p) < th
    zero = np.zeros_like(p)
    ch = small & (p != 0)
    erows, ecols = ref_zf(ch, n)
    for emode in (True, False):
        zf0 = torch.zeros(k.trial_mask_words(n), dtype=torch.int32, device=DEV)
        s = _out_np(k.trial_proxgd(_dev(xt), None, T_STEP, MUS[0], THRES, form=2, emode=emode, p=_dev(p), zf=zf0))
        assert _same_bits(s["pthr"], np.where(small, zero, p))
        rows, cols = unpack_zf(s["zf"], n)
        assert np.array_equal(rows, erows) and np.array_equal(cols, ecols)
        if emode:
            assert _same_bits(s["z"], np.where(small, p, zero))
        else:
            with np.errstate(all="ignore"):
                z = xt - t * ((xt - p) / t)
            assert np.array_equal(np.isnan(s["z"]), np.isnan(z))
            assert _same_bits(s["z"], z, ~np.isnan(z))
    theta, a1, b1 = npdt(THETA), npdt(1.0 - THETA_NEXT), npdt(THETA_NEXT)
    with np.errstate(all="ignore"):
        xo = np.where(np.abs(xt) < th, npdt(0), xt)
        vn = xo + (p - xo) / theta
        yn = a1 * np.where(small, npdt(0), p) + b1 * vn
    f = _out_np(k.trial_fista(None, None, _dev(xt), T_STEP, MUS[0], THETA, THETA_NEXT, THRES, form=2, xc=_dev(p)))
    for got, want in ((f["vnext"], vn), (f["ynext"], yn)):
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert _same_bits(got, want, ~np.isnan(want))


# ---------------------------------------------------------------------------------------------
# stale words: a trial rewrites every word of the groups it visits, also with nothing to flag
# ---------------------------------------------------------------------------------------------
def _flagging_inputs(n, l, dtype, seed):
    """Inputs whose trial at a tiny mu zeroes a nonzero entry in nearly every row (|p| ~ 3e-4) and
    at a huge mu gives p = 0 everywhere."""
    npdt = _types(dtype)[0]
    rng = np.random.default_rng(seed)
    x = (3e-4 * rng.standard_normal((n, l))).astype(npdt)
    g = (1e-5 * rng.standard_normal((n, l))).astype(npdt)
    return x, g


MU_FLAG_ALL, MU_FLAG_NONE = 1e-6, 1e3


def _assert_zf(zf, ch, n):
    rows, cols = unpack_zf(zf, n)
    erows, ecols = ref_zf(ch, n)
    assert np.array_equal(rows, erows) and np.array_equal(cols, ecols)


@pytest.mark.parametrize("n", [17, 65, 2063])
@pytest.mark.parametrize("l", [16, 32])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_stale_words_row_kernels(dtype, l, n):
    k = _k()
    x, g = _flagging_inputs(n, l, dtype, seed=n + l)
    ref1 = ref_proxgd(x, g, T_STEP, MU_FLAG_ALL, THRES)
    ref2 = ref_proxgd(x, g, T_STEP, MU_FLAG_NONE, THRES)
    assert _amb_count(ref1) == 0 and _amb_count(ref2) == 0
    assert ref1["ch"].any(axis=1).sum() > n // 2 and not ref2["ch"].any()
    xd, gd = _dev(x), _dev(g)
    for form in ("proxgd", "fista", "split"):
        zf = torch.zeros(k.trial_mask_words(n), dtype=torch.int32, device=DEV)
        if form == "proxgd":
            k.trial_proxgd(xd, gd, T_STEP, MU_FLAG_ALL, THRES, emode=True, zf=zf)
            _assert_zf(_np(zf), ref1["ch"], n)
            k.trial_proxgd(xd, gd, T_STEP, MU_FLAG_NONE, THRES, emode=True, zf=zf)
        elif form == "fista":   # y = x and the same prox: the same p, so the same flags
            k.trial_fista(xd, gd, xd, T_STEP, MU_FLAG_ALL, THETA, THETA_NEXT, THRES, split=True, zf=zf)
            _assert_zf(_np(zf), ref1["ch"], n)
            k.trial_fista(xd, gd, xd, T_STEP, MU_FLAG_NONE, THETA, THETA_NEXT, THRES, split=True, zf=zf)
        else:
            p1 = k.trial_proxgd(xd, gd, T_STEP, MU_FLAG_ALL, THRES)["p"]
            p2 = k.trial_proxgd(xd, gd, T_STEP, MU_FLAG_NONE, THRES)["p"]
            k.trial_proxgd(xd, None, T_STEP, MU_FLAG_ALL, THRES, form=2, emode=True, p=p1, zf=zf)
            _assert_zf(_np(zf), ref1["ch"], n)
            k.trial_proxgd(xd, None, T_STEP, MU_FLAG_NONE, THRES, form=2, emode=True, p=p2, zf=zf)
        _assert_zf(_np(zf), ref2["ch"], n)


@pytest.mark.parametrize("tile", [8, 38])
@pytest.mark.parametrize("kind", ["proxgd", "fista"])
def test_stale_words_fused(monkeypatch, kind, tile):
    monkeypatch.setenv("GLX_ATR_VARIANT", str(tile))
    monkeypatch.setenv("GLX_ATR_S", "1")
    k = _k()
    m, n, l = 64, 2048, 32
    x, _ = _flagging_inputs(n, l, "f64", seed=tile)
    rng = np.random.default_rng(tile + 1)
    A = _dev(1e-5 * rng.standard_normal((m, n)) / 8.0)
    R = _dev(rng.standard_normal((m, l)))
    xd = _dev(x)
    zf = torch.zeros(k.trial_mask_words(n), dtype=torch.int32, device=DEV)
    for mu, most in ((MU_FLAG_ALL, True), (MU_FLAG_NONE, False)):
        if kind == "proxgd":
            o = k.trial_proxgd(xd, None, T_STEP, mu, THRES, form=1, emode=True, A=A, R=R, zf=zf)
        else:
            o = k.trial_fista(xd, None, xd, T_STEP, mu, THETA, THETA_NEXT, THRES, form=1, split=True, A=A, R=R,
                              zf=zf)
        ref = ref_proxgd(x, _np(o["G"]), T_STEP, mu, THRES)
        assert _amb_count(ref) == 0
        assert (ref["ch"].any(axis=1).sum() > n // 2) if most else not ref["ch"].any()
        _assert_zf(_np(zf), ref["ch"], n)


# ---------------------------------------------------------------------------------------------
# chain: the masks and e of a trial drive the A e gathers
# ---------------------------------------------------------------------------------------------
def test_trial_masks_drive_the_gather():
    k = _k()
    m, n, l = 192, 1000, 32
    x, g, _ = _gen(n, l, "f64", seed=4242)
    _special_rows(x, g)
    o = k.trial_proxgd(_dev(x), _dev(g), T_STEP, MUS[1], THRES, emode=True)
    e = o["z"]
    assert int((e != 0).any(dim=1).sum()) > n // 8
    At = torch.randn(n, m, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).to(DEV)
    ref = At.T @ e
    scale = float((At.abs().T @ e.abs()).max())
    for form in (1, 2):
        Y = k.flagged_rows_product(At, e, o["zf"], form=form)
        err = float((Y - ref).abs().max())
        assert err <= 1e-13 * max(1.0, scale), (form, err)
