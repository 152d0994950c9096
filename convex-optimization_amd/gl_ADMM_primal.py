"""Drop-in replacement for the reference's ``code/gl_ADMM_primal.py`` (def at line 10).

Same module name, function name, signature and return contract — main.py (or any
caller) imports it unchanged with this directory on sys.path. The computation runs on
the GPU through libglx (glx/admm_primal.py); there is no CPU fallback.
"""
from glx.admm_primal import solve as _solve


def gl_Admm_primal(x0, A, b, mu, opts: dict):
    return _solve(x0, A, b, mu, opts)
