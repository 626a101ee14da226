"""TEST INFRASTRUCTURE: the numpy statement of the flux-average contract (include/amt_advance_mu_t.h section 14, DESIGN.md
section 7.7).  Explicit loops over the ranges, one dtype-exact scalar operation per rounding, no library calls.

Arrays are laid out as everywhere in the tests: 3-D (jdim, kdim, idim), 2-D (jdim, idim), Fortran index x at x - xms; with
``members`` > 1 one more leading axis.  ``bounds`` needs ids ide jds jde kde ims ime jms jme kms kme its ite jts jte kts kte.
"""
from __future__ import annotations

import numpy as np

ACCUMULATORS = ("ru_m", "rv_m", "ww_m")
INPUTS = ("u", "v", "ww", "u_1", "v_1", "ww_1", "muu", "muv", "msfuy", "msfvx_inv")
INPUTS_3D = INPUTS[:6]
# accumulator -> (the field it adds, the field of the linearisation state, the two 2-D factors)
ROLE = {"ru_m": ("u", "u_1", "muu", "msfuy"), "rv_m": ("v", "v_1", "muv", "msfvx_inv"), "ww_m": ("ww", "ww_1", None, None)}


def ranges(b, name):
    """Fortran-inclusive (i0, i1, k0, k1, j0, j1) in which accumulator ``name`` accumulates; a range may be empty (x1 < x0)."""
    imass, jmass = min(b.ite, b.ide - 1), min(b.jte, b.jde - 1)
    return {"ru_m": (b.its, b.ite, b.kts, b.kte - 1, b.jts, jmass),
            "rv_m": (b.its, imass, b.kts, b.kte - 1, b.jts, b.jte),
            "ww_m": (b.its, imass, b.kts, b.kte, b.jts, jmass)}[name]


def range_mask(b, name):
    """Boolean (jdim, kdim, idim): the cells of the accumulator's range."""
    i0, i1, k0, k1, j0, j1 = ranges(b, name)
    m = np.zeros((b.jme - b.jms + 1, b.kme - b.kms + 1, b.ime - b.ims + 1), bool)
    if i1 >= i0 and k1 >= k0 and j1 >= j0:
        m[j0 - b.jms:j1 - b.jms + 1, k0 - b.kms:k1 - b.kms + 1, i0 - b.ims:i1 - b.ims + 1] = True
    return m


def tile_mask(b):
    """Boolean (jdim, kdim, idim): the tile box its..ite, kts..kte, jts..jte."""
    m = np.zeros((b.jme - b.jms + 1, b.kme - b.kms + 1, b.ime - b.ims + 1), bool)
    if b.ite >= b.its and b.kte >= b.kts and b.jte >= b.jts:
        m[b.jts - b.jms:b.jte - b.jms + 1, b.kts - b.kms:b.kte - b.kms + 1, b.its - b.ims:b.ite - b.ims + 1] = True
    return m


def _stacked(a, members, ndim):
    a = np.asarray(a)
    return a.reshape((members,) + a.shape[-ndim:]) if a.ndim == ndim + 1 or members == 1 else a


def sumflux(acc, inp, b, iteration, n, members=1):
    """One accumulation IN PLACE on ``acc`` (name -> array for ACCUMULATORS); ``inp``: name -> array for INPUTS (never
    written; entries may be one array).  Returns ``acc``."""
    if not (n >= 1 and 1 <= iteration <= n and members >= 1):
        raise ValueError("n >= 1, 1 <= iteration <= n, members >= 1")
    first, last = iteration == 1, iteration == n
    with np.errstate(all="ignore"):
        for name in ACCUMULATORS:
            xn, x1n, fan, fbn = ROLE[name]
            a = _stacked(acc[name], members, 3)
            T = a.dtype.type
            zero, nT = T(0), T(n)
            x, x1 = _stacked(inp[xn], members, 3), _stacked(inp[x1n], members, 3)
            fa = _stacked(inp[fan], members, 2) if fan else None
            fb = _stacked(inp[fbn], members, 2) if fbn else None
            assert a.shape[0] == members and x.dtype == a.dtype and x1.dtype == a.dtype and np.shares_memory(a, acc[name])
            i0, i1, k0, k1, j0, j1 = ranges(b, name)
            for m in range(members):
                for j in range(b.jts, b.jte + 1):
                    for k in range(b.kts, b.kte + 1):
                        for i in range(b.its, b.ite + 1):
                            at = (m, j - b.jms, k - b.kms, i - b.ims)
                            if not (i0 <= i <= i1 and k0 <= k <= k1 and j0 <= j <= j1):
                                if first:
                                    a[at] = zero                  # WRF zeroes the whole tile
                                continue
                            s = zero + x[at] if first else a[at] + x[at]
                            if last:
                                q = s / nT
                                at2 = (m, j - b.jms, i - b.ims)
                                if name == "ru_m":
                                    s = q + (fa[at2] * x1[at]) / fb[at2]
                                elif name == "rv_m":
                                    s = q + (fa[at2] * x1[at]) * fb[at2]
                                else:
                                    s = q + x1[at]
                            a[at] = s
    return acc


def as_bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)
