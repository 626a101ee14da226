"""TEST INFRASTRUCTURE: the numpy statement of the acoustic loop's pressure diagnosis calc_p_rho (include/amt_advance_mu_t.h
section 16): one numpy operation per rounding in the arrays' dtype, no library calls.

Arrays are laid out as everywhere in the tests: 3-D (jdim, kdim, idim), 2-D (jdim, idim), 1-D (kdim,), Fortran index x at
x - xms; with ``members`` > 1 the 3-D and 2-D arrays have one more leading axis, the 1-D arrays are shared.  ``bounds`` needs
ids ide jds jde kde ims ime jms jme kms kme its ite jts jte kts kte.  ``p_rho`` works IN PLACE on the dict it is given and
returns it: every array of the call, outputs and inputs.  Inputs may be one array under two names; an output is its own.
"""
from __future__ import annotations

import numpy as np

from stage_ref import as_bits, cell_mask, column_mask, columns  # noqa: F401  -- the ranges are the stage bracket's

OUT_3D = ("al", "p", "ph", "pm1")                                  # ph: an input in mode 1, an output above kts in mode 2
IN_3D = ("alt", "c2a", "t", "t_old")
IN_2D = ("mu", "muts")
IN_1D = ("rdnw", "znu", "dnw")
NAMES = OUT_3D + IN_3D + IN_2D + IN_1D                             # the argument order of amt_p_rho_device_*
SETTING = ("al", "p", "ph", "pm1", "alt", "c2a", "znu", "dnw")     # what amt_*_p_rho_ptr numbers 0..7
NONHYDROSTATIC, HYDROSTATIC = 1, 2


def shape(b, name, members=1):
    if name in IN_1D:
        return (b.kdim,)
    one = (b.jdim, b.idim) if name in IN_2D else (b.jdim, b.kdim, b.idim)
    return ((members,) + one) if members > 1 else one


def level_mask(b):
    """Boolean (kdim,): the levels kts..kte-1 of a 1-D array."""
    m = np.zeros(b.kdim, bool)
    m[b.kts - b.kms:b.kte - b.kms] = True
    return m


def written_mask(b, name, mode):
    """The cells of ``name`` a call may change; None: not one."""
    if name in ("al", "p", "pm1"):
        return cell_mask(b, "t")
    if name == "ph" and mode == HYDROSTATIC:                       # kts+1..kte
        m = cell_mask(b, "ww")
        m[:, b.kts - b.kms, :] = False
        return m
    return None


def read_mask(b, name, mode, step):
    """The cells of ``name`` a call reads before it has written them; None: not one."""
    if name in IN_3D:
        return cell_mask(b, "t")
    if name in IN_2D:
        return column_mask(b)
    if name == "ph":
        m = cell_mask(b, "ww")                                     # mode 1: kts..kte
        if mode == HYDROSTATIC:                                    # mode 2: level kts alone
            m[:, b.kts - b.kms + 1:, :] = False
        return m
    if name == "pm1":
        return cell_mask(b, "t") if step != 0 else None
    if name == "rdnw":
        return level_mask(b) if mode == NONHYDROSTATIC else None
    if name in ("znu", "dnw"):
        return level_mask(b) if mode == HYDROSTATIC else None
    return None                                                    # al, p


def p_rho(a, b, mode, step, t0, smdiv):
    """One diagnosis behind sub-step ``step`` (0: behind small_step_prep) on ``a``: name -> array for NAMES.  ``t0`` and
    ``smdiv`` are rounded to the arrays' dtype first."""
    if mode not in (NONHYDROSTATIC, HYDROSTATIC):
        raise ValueError("mode 1 or 2")
    if step < 0:
        raise ValueError("step >= 0")
    T = a["t"].dtype.type
    t0, smdiv = T(t0), T(smdiv)
    sj, si = columns(b)
    col = (Ellipsis, sj, si)
    with np.errstate(all="ignore"):
        mu, muts = a["mu"][col], a["muts"][col]
        if mode == NONHYDROSTATIC:
            minus_over_muts = T(-1) / muts
        for k in range(b.kts, b.kte):                              # cells kts..kte-1, ascending: mode 2 is a recurrence
            kk = k - b.kms
            here, above = (Ellipsis, sj, kk, si), (Ellipsis, sj, kk + 1, si)
            alt, c2a, told = a["alt"][here], a["c2a"][here], a["t_old"][here]
            mt = mu * told
            dt = a["t"][here] - mt
            num = alt * dt
            tsum = t0 + told
            den = muts * tsum
            q = num / den
            if mode == NONHYDROSTATIC:
                am = alt * mu
                dph = a["ph"][above] - a["ph"][here]
                rd = a["rdnw"][kk] * dph
                s = am + rd
                al = minus_over_muts * s
                e = q - al
                x = c2a * e
            else:
                x = mu * a["znu"][kk]
                r = x / c2a
                al = q - r
                ma = muts * al
                mb = mu * alt
                s = ma + mb
                d = a["dnw"][kk] * s
                a["ph"][above] = a["ph"][here] - d
            a["al"][here] = al
            if step == 0:
                a["p"][here] = x
            else:
                dx = x - a["pm1"][here]
                sd = smdiv * dx
                a["p"][here] = x + sd
            a["pm1"][here] = x
    return a
