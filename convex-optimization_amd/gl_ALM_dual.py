"""Drop-in replacement for the reference's ``code/gl_ALM_dual.py`` (def at line 66).

Same module name, function name, signature and return contract — main.py (or any
caller) imports it unchanged with this directory on sys.path. The computation runs on
the GPU through libglx (glx/alm.py); there is no CPU fallback.
"""
from glx.alm import solve as _solve


def gl_Alm_dual(x0, A, b, mu, opts: dict):
    return _solve(x0, A, b, mu, opts)
