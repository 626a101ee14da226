"""TEST INFRASTRUCTURE: the numpy statement of the Runge-Kutta stage bracket (include/amt_advance_mu_t.h section 15, DESIGN.md
section 7.8): small_step_prep and small_step_finish as whole-array operations on the ranges, one numpy operation per rounding
in the arrays' dtype, no library calls.

Arrays are laid out as everywhere in the tests: 3-D (jdim, kdim, idim), 2-D (jdim, idim), Fortran index x at x - xms; with
``members`` > 1 one more leading axis.  ``bounds`` needs ids ide jds jde kde ims ime jms jme kms kme its ite jts jte kts kte.
Both functions work IN PLACE on the dict they are given and return it: every array of the call, outputs and inputs.
"""
from __future__ import annotations

import numpy as np

PREP_3D = ("t", "t_1", "t_old", "ww", "ww_1")
PREP_2D = ("mu", "mu_old", "mu_save", "muts", "mudf", "mut", "mub")
PREP = PREP_3D + PREP_2D                                           # the argument order of amt_stage_prep_device_*
FINISH_3D = ("t", "t_1", "ww", "ww_1")
FINISH_2D = ("mu", "mu_save", "muts", "mut")
FINISH = FINISH_3D + FINISH_2D                                     # of amt_stage_finish_device_*, h_diabatic apart
EXTRAS = ("t_old", "mu_old", "mu_save", "mub")                     # what amt_*_stage_ptr numbers 0..3


def prep_outputs(rk_step):
    """The arrays prep writes at this step; every other array of the call is an input."""
    return ("t", "t_1", "ww_1", "mu", "mu_save", "muts") + (("t_old", "mu_old", "mudf") if rk_step == 1 else ())


FINISH_OUTPUTS = ("t", "ww", "mu")


def columns(b):
    """(slice j, slice i) of the columns its..min(ite, ide-1), jts..min(jte, jde-1); empty slices where there are none."""
    ihi, jhi = min(b.ite, b.ide - 1), min(b.jte, b.jde - 1)
    return slice(b.jts - b.jms, max(jhi, b.jts - 1) - b.jms + 1), slice(b.its - b.ims, max(ihi, b.its - 1) - b.ims + 1)


def column_mask(b):
    m = np.zeros((b.jme - b.jms + 1, b.ime - b.ims + 1), bool)
    m[columns(b)] = True
    return m


def cell_mask(b, levels):
    """Boolean (jdim, kdim, idim): the columns over kts..kte-1 (levels = "t") or kts..kte (levels = "ww")."""
    m = np.zeros((b.jme - b.jms + 1, b.kme - b.kms + 1, b.ime - b.ims + 1), bool)
    sj, si = columns(b)
    m[sj, b.kts - b.kms:b.kte - b.kms + (1 if levels == "ww" else 0), si] = True
    return m


def _boxes(b):
    sj, si = columns(b)
    kt = slice(b.kts - b.kms, b.kte - b.kms)                       # kts..kte-1
    kw = slice(b.kts - b.kms, b.kte - b.kms + 1)                   # kts..kte
    return (Ellipsis, sj, si), (Ellipsis, sj, kt, si), (Ellipsis, sj, kw, si), (Ellipsis, sj, None, si)


def prep(a, b, rk_step):
    """small_step_prep of Runge-Kutta step ``rk_step`` on ``a``: name -> array for PREP (``mudf`` may be None at rk_step > 1)."""
    if rk_step < 1:
        raise ValueError("rk_step >= 1")
    col, cell_t, cell_w, lift = _boxes(b)
    with np.errstate(all="ignore"):
        m = a["mu"][col].copy()                                    # mu as it was before the call
        x = a["t"][cell_t].copy()                                  # t as it was before the call
        if rk_step == 1:
            a["mu_old"][col] = m
            a["muts"][col] = a["mub"][col] + m
            a["mu_save"][col] = m
            a["mu"][col] = m - m
            a["mudf"][col] = 0
            a["t_old"][cell_t] = x
        else:
            a["muts"][col] = a["mub"][col] + a["mu_old"][col]
            a["mu_save"][col] = m
            a["mu"][col] = a["mu_old"][col] - m
        s = a["muts"][lift]                                        # the NEW muts, one value per column
        a["t_1"][cell_t] = x
        left = s * a["t_old"][cell_t]
        right = a["mut"][lift] * x
        a["t"][cell_t] = left - right
        a["ww_1"][cell_w] = a["ww"][cell_w]
    return a


def finish(a, b, n, dts, h_diabatic=None):
    """small_step_finish behind ``n`` sub-steps on ``a``: name -> array for FINISH; ``h_diabatic`` an array of t's shape or None.
    ``dts`` is rounded to the arrays' dtype first."""
    if n < 1:
        raise ValueError("n >= 1")
    col, cell_t, cell_w, lift = _boxes(b)
    T = a["t"].dtype.type
    with np.errstate(all="ignore"):
        mut, muts = a["mut"][lift], a["muts"][lift]
        acc = a["t"][cell_t]
        if h_diabatic is not None:
            c = T(dts) * T(n)
            cm = c * mut
            heat = cm * np.asarray(h_diabatic)[cell_t]
            acc = acc - heat
        back = a["t_1"][cell_t] * mut
        total = acc + back
        a["t"][cell_t] = total / muts
        a["ww"][cell_w] = a["ww"][cell_w] + a["ww_1"][cell_w]
        a["mu"][col] = a["mu"][col] + a["mu_save"][col]
    return a


def as_bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)
