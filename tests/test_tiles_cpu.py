"""The case table of test_gpu_tiles.py, checked on the host (no GPU).

glx_plan_describe reads the same GLX_* variables as the launchers, so what a case says it runs
can be asserted without launching anything: every case's plan string, that the table names every
tile of csrc/glx_tiles.h and no other, and that every admitted (tile, dtype, right-hand sides)
has a case. A tile added to glx_tiles.h without a case fails here.
"""
import os
import re

import pytest

import tile_cases
from conftest import PKG

TILES_H = os.path.join(PKG, "csrc", "glx_tiles.h")
DTYPE_BITS = {"kF32": ("f32",), "kF64": ("f64",), "kAnyType": ("f32", "f64"), "0u": ()}


def _table(text, name):
    """The {code, Fam::..., ...} rows of `inline constexpr <Tile> <name>[] = { ... };`."""
    body = re.search(r"%s\[\]\s*=\s*\{(.*?)\n\};" % name, text, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    rows = []
    for code, fam, rest in re.findall(r"\{\s*(\d+)\s*,\s*Fam::(\w+)\s*,([^{}]*)\}", body):
        rows.append((int(code), fam, [f.strip() for f in rest.split(",")]))
    assert rows, name
    return rows


def _int(field):
    return {"true": 1, "false": 0}[field] if field in ("true", "false") else int(field)


def tiles():
    """{("ax", code): record} and {("atr", code): record} with the fields the plan string shows
    and the admitted (dtype, nsrc) set."""
    with open(TILES_H) as fh:
        text = fh.read()
    out = {}
    for code, fam, f in _table(text, "kAxTiles"):
        mt, pf, vpl, waves, slots, kc, ntl = (_int(x) for x in f[:7])
        planned, built = DTYPE_BITS[f[9]], DTYPE_BITS[f[10]]
        nmin, nmax, shown = int(f[11]), int(f[12]), int(f[13])
        if fam == "Valu":
            name = "k_ax_valu<"
        elif fam == "Mfma":
            name = "k_ax_mfma<kind1,MT%d,PF%d,NTL%d,VPL%d> S=" % (mt, pf, ntl, vpl)
        elif fam == "Lds":
            name = "k_ax_lds<MT%d,PF%d,VPL%d,W%d> S=" % (mt, pf, vpl, waves)
        else:
            name = "k_ax_dma<MT%d,NS%d,KC%d,NTL%d,HOIST%d(2:PIPE),W%d> S=" % (mt, slots, kc, ntl, shown, waves)
        admitted = {(dt, ns) for dt in built if dt in planned for ns in range(nmin, nmax + 1)}
        out[("ax", code)] = {"name": name, "admitted": admitted, "tail": ""}
    for code, fam, f in _table(text, "kAtrTiles"):
        wl, pf, ntl, panel = (_int(x) for x in f[:4])
        name = "k_atr_valu<" if fam == "Valu" else "k_atr_mfma<WL%d,PF%d,NTL%d> S=" % (wl, pf, ntl)
        out[("atr", code)] = {"name": name, "admitted": {(dt, 1) for dt in DTYPE_BITS[f[5]]},
                              "tail": " (32-column panels)" if panel == 32 else ""}
    return out


def uncovered(rows):
    """The admitted (product, tile, dtype, nsrc) that no case of `rows` runs."""
    have = {(c.product, c.code, c.dtype, c.nsrc) for c in tile_cases.cases(rows)}
    want = {(p, code, dt, ns) for (p, code), t in tiles().items() for dt, ns in t["admitted"]}
    return sorted(want - have), sorted(have - want)


CASES = tile_cases.cases()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_plans_what_it_names(case, monkeypatch):
    from glx import _lib
    tile_cases.apply_env(monkeypatch, case.env)
    plan = _lib.plan_describe(_lib.GLX_F64 if case.dtype == "f64" else _lib.GLX_F32, case.m, case.n, case.l)
    assert case.plan in plan.split("; "), (case.id, plan)   # a whole entry: S=1 is not S=12
    # and the string is the one the claimed tile's record prints: the code is not just a label
    tile = tiles()[(case.product, case.code)]
    shown = case.plan.split("=", 1)[1]
    assert shown.startswith(tile["name"]) and shown.endswith(tile["tail"]), (case.id, tile["name"])
    assert tile["tail"] or "panels" not in shown


def test_table_names_exactly_the_tiles_of_glx_tiles_h():
    claimed = {(c.product, c.code) for c in CASES}
    assert claimed == set(tiles()), (sorted(set(tiles()) - claimed), sorted(claimed - set(tiles())))


def test_every_admitted_combination_has_a_case():
    missing, extra = uncovered(tile_cases.ROWS)
    assert not missing, "no case runs (product, tile, dtype, nsrc): %s" % missing
    assert not extra, "cases for combinations glx_tiles.h does not admit: %s" % extra


def test_built_but_unplanned_dtypes_cannot_be_requested(monkeypatch):
    """Admitted above means built and planned (AxTile::built and ::dtypes). A tile compiled for a
    dtype its record does not plan (the f64 LDS-DMA tiles in f32) is out of reach of both variant
    knobs, so there is nothing to run: asked for, the plan shows another kernel."""
    from glx import _lib
    with open(TILES_H) as fh:
        rows = _table(fh.read(), "kAxTiles")
    checked = 0
    for code, fam, f in rows:
        for dt in set(DTYPE_BITS[f[10]]) - set(DTYPE_BITS[f[9]]):
            name = tiles()[("ax", code)]["name"]
            kc = max(int(f[5]), 16)
            for knob in ("GLX_AX_VARIANT", "GLX_AXB_VARIANT"):
                for m, n, l in ((17, kc, 16), (17, 4 * kc, 32), (257, 25 * kc, 16), (8192, 16384, 32)):
                    tile_cases.apply_env(monkeypatch, {knob: str(code)})
                    plan = _lib.plan_describe(_lib.GLX_F64 if dt == "f64" else _lib.GLX_F32, m, n, l)
                    assert name not in plan, (code, dt, knob, plan)
                    checked += 1
    assert checked   # glx_tiles.h has such tiles today; drop this test's reason with them


def test_every_row_is_needed():
    """Each row is the only cover of its (tile, dtype, nsrc): without it the check above fails and
    names the combination."""
    keys = [r[:4] for r in tile_cases.ROWS]
    assert len(set(keys)) == len(keys)
    for i, row in enumerate(tile_cases.ROWS):
        missing, _ = uncovered(tile_cases.ROWS[:i] + tile_cases.ROWS[i + 1:])
        assert missing == [row[:4]], (row[:4], missing)


def test_forced_splits_leave_no_split_empty():
    """A forced S must leave every split a chunk (A @ X) or a row step (A^T R): an LDS tile's block
    without chunks returns before it writes its slab."""
    for c in CASES:
        S = int(re.search(r"S=(\d+)", c.plan).group(1))
        if c.product == "atr":
            steps = c.m // 4 if "mfma" in c.plan else c.m
            assert steps >= S, c.id
        else:
            m = re.search(r"KC(\d+)", c.plan)
            es = 8 if c.dtype == "f64" else 4
            vpl = re.search(r"VPL(\d)", c.plan)
            chunk = int(m.group(1)) if m else (4 * (16 // es) * int(vpl.group(1)) if vpl else 1)
            assert c.n // chunk >= S, c.id
