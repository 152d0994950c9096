"""Drop-in replacement for the reference's ``code/gl_ADMM_dual.py`` (def at line 10).

Same module name, function name, signature and return contract — main.py (or any
caller) imports it unchanged with this directory on sys.path. The computation runs on
the GPU through libglx (glx/admm.py); there is no CPU fallback.
"""
from glx.admm import solve as _solve


def gl_Admm_dual(x0, A, b, mu, opts: dict):
    return _solve(x0, A, b, mu, opts)
