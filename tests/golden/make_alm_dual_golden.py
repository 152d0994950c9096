"""Generate the dual ALM fixtures in tests/golden/ by running the REFERENCE solver.

Run in the build container only (the reference tree does not exist on the GPU box):

    python tests/golden/make_alm_dual_golden.py

It imports ``gl_ALM_dual`` from ``/root/reference/code`` (read-only tree, so byte-code writing is
disabled), feeds it instances drawn by the repo's own generator (``glx.driver.gen_data``, a
restatement of ``main.py:37-51``) and stores only data: the seed, the shape, the options, input
hashes, ``b`` itself (the host BLAS's ``A @ u`` is not portable bit for bit; A and x0 are redrawn),
the reference's ``x, k, fval, f_hist, f_hist_best`` and the spectral norms ``||r||_2``, ``||s||_2``
of every iteration. The norms are recorded by watching the reference's own ``LA.norm(., ord=2)``
calls on 2-D arguments without an axis (``gl_ALM_dual.py:140-141``; the row norms of its prox pass
``axis=1``). No reference source is copied.

A case whose norms come within 5e-3 relative of ``thres`` at any iteration is refused: the GPU
takes those norms from Gram matrices of a restructured iteration, and "identical k" is a fair
demand only away from a tie.

For the record, the index also holds what ``tests/alm_dual_ref.py`` (the restructured iteration in
NumPy float64) measured against each run on the machine that wrote it: the largest relative
deviation of ``f_hist``, of x (relative to max |x|) and of the two norms.

Writes ``alm_dual_<case>.npz`` and the index ``alm_dual_index.json``.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/code"
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "convex-optimization_amd"))
sys.path.insert(0, REF)

from glx.driver import SEED, gen_data  # noqa: E402

import alm_dual_ref  # noqa: E402
import gl_ALM_dual as _ref  # noqa: E402

MU = 1e-2
THRES = 1e-3          # the reference's default (gl_ALM_dual.py:69)
MIN_MARGIN = 5e-3     # relative distance every norm must keep from THRES
# (m, n, l, opts): the dual ADMM solver's six shapes with default options, and one with t rho != 1
CASES = [(256, 512, 2, {}), (64, 128, 16, {}), (128, 256, 32, {}), (100, 130, 3, {}), (192, 128, 16, {}),
         (96, 192, 1, {}), (64, 128, 16, {"rho": 50.0})]


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


class _NormWatch:
    """Stands in for the reference module's ``LA``: records the matrix 2-norms it takes."""

    def __init__(self, la):
        self._la = la
        self.seen = []

    def __getattr__(self, name):
        return getattr(self._la, name)

    def norm(self, x, *args, **kw):
        v = self._la.norm(x, *args, **kw)
        if kw.get("ord") == 2 and "axis" not in kw and np.ndim(x) == 2:
            self.seen.append(float(v))
        return v


def deviations(arrays, x0, A, b, mu, opts):
    x, k, out = alm_dual_ref.gl_alm_dual(x0, A, b, mu, opts)
    if k != int(arrays["k"]):
        raise SystemExit("the restated iteration gives k = %d, the reference %d" % (k, int(arrays["k"])))
    rel = lambda got, want: float(np.max(np.abs(np.asarray(got) - want) / np.abs(want)))
    return {"f_hist": rel(out["f_hist"], arrays["f_hist"]),
            "x": float(np.max(np.abs(x - arrays["x"])) / np.max(np.abs(arrays["x"]))),
            "r_norm": rel(out["r_norm"], arrays["r_norm"]), "s_norm": rel(out["s_norm"], arrays["s_norm"])}


def run_case(m, n, l, opts):
    _, _, _, mu, A, b, _u, x0, *_ = gen_data(SEED, m, n, l, MU)
    watch = _NormWatch(np.linalg)
    _ref.LA = watch
    try:
        x, k, out = _ref.gl_Alm_dual(x0, A, b, mu, dict(opts))
    finally:
        _ref.LA = np.linalg
    norms = np.asarray(watch.seen, dtype=np.float64).reshape(-1, 2)   # (r, s) per iteration
    assert norms.shape[0] == k, (norms.shape, k)
    margin = float(np.min(np.abs(norms - THRES) / THRES))
    if margin < MIN_MARGIN:
        raise SystemExit("case %s: a norm comes within %.1e of thres; refusing to write it" % ((m, n, l, opts), margin))
    arrays = {"b": b, "x": x, "k": np.int64(k), "fval": np.float64(out["fval"]),
              "f_hist": np.asarray(out["f_hist"], dtype=np.float64),
              "f_hist_best": np.asarray(out["f_hist_best"], dtype=np.float64),
              "r_norm": norms[:, 0], "s_norm": norms[:, 1]}
    meta = {"m": m, "n": n, "l": l, "seed": SEED, "mu": mu, "dtype": "f64", "k": int(k), "opts": dict(opts),
            "margin": margin, "restated_deviation": deviations(arrays, x0, A, b, mu, opts),
            "sha256": {"A": sha(A), "b": sha(b), "x0": sha(x0)}}
    return meta, arrays


def main():
    index = {}
    for m, n, l, opts in CASES:
        name = "alm_dual_%dx%dx%d" % (m, n, l)
        if opts:
            name += "_" + "_".join("%s%g" % (key, v) for key, v in opts.items())
        meta, arrays = run_case(m, n, l, opts)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **arrays)
        index[name] = meta
        print("%s: k=%d fval=%.12e margin=%.2e dev=%s" % (name, meta["k"], float(arrays["fval"]), meta["margin"],
                                                         json.dumps(meta["restated_deviation"])), flush=True)
    with open(os.path.join(HERE, "alm_dual_index.json"), "w") as fh:
        json.dump(index, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
