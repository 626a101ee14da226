"""TEST INFRASTRUCTURE: the numpy statement of the acoustic loop's momentum update advance_uv (include/amt_advance_mu_t.h
section 17): one numpy operation per rounding in the arrays' dtype, no library calls.

Arrays are laid out as everywhere in the tests: 3-D (jdim, kdim, idim), 2-D (jdim, idim), 1-D (kdim,), Fortran index x at
x - xms; with ``members`` > 1 the 3-D and 2-D arrays have one more leading axis, the 1-D arrays are shared.  ``bounds`` needs
ids ide jds jde kde ims ime jms jme kms kme its ite jts jte kts kte.  ``advance_uv`` works IN PLACE on the dict it is given and
returns it: every array of the call, outputs and inputs.  Inputs may be one array under two names; u and v are their own.
"""
from __future__ import annotations

import numpy as np

OUT_3D = ("u", "v")
IN_3D = ("ru_tend", "rv_tend", "p", "pb", "ph", "php", "alt", "al")
IN_2D = ("mu", "muu", "muv", "mudf")
CQ_3D = ("cqu", "cqv")
MSF_2D = ("msfux", "msfuy", "msfvx", "msfvx_inv", "msfvy")
IN_1D = ("fnm", "fnp", "rdnw")
NAMES = OUT_3D + IN_3D + IN_2D + CQ_3D + MSF_2D + IN_1D            # the argument order of amt_advance_uv_device_*
RANK = {**{n: 3 for n in OUT_3D + IN_3D + CQ_3D}, **{n: 2 for n in IN_2D + MSF_2D}, **{n: 1 for n in IN_1D}}
# what each part reads beside its own output: 3-D and 2-D arrays at the cell and at its neighbour (i-1 for u, j-1 for v) ...
BOTH = ("p", "pb", "ph", "php", "alt", "al", "mu", "mudf")
# ... and at the cell alone
OWN = {"u": ("u", "ru_tend", "cqu", "muu", "msfux", "msfuy"), "v": ("v", "rv_tend", "cqv", "muv", "msfvx", "msfvy", "msfvx_inv")}


def shape(b, name, members=1):
    if RANK[name] == 1:
        return (b.kdim,)
    one = (b.jdim, b.idim) if RANK[name] == 2 else (b.jdim, b.kdim, b.idim)
    return ((members,) + one) if members > 1 else one


def ranges(b, periodic_x=False, specified=False, nested=False):
    """(i_start, i_end, i_endu, j_start, j_end, j_endv), Fortran-inclusive and global."""
    clip = bool(specified or nested)
    if clip and not periodic_x:
        i_start, i_end, i_endu = max(b.its, b.ids + 1), min(b.ite, b.ide - 2), min(b.ite, b.ide - 1)
    else:
        i_start, i_end, i_endu = b.its, min(b.ite, b.ide - 1), b.ite
    if clip:
        j_start, j_end, j_endv = max(b.jts, b.jds + 1), min(b.jte, b.jde - 2), min(b.jte, b.jde - 1)
    else:
        j_start, j_end, j_endv = b.jts, min(b.jte, b.jde - 1), b.jte
    return i_start, i_end, i_endu, j_start, j_end, j_endv


def part_ranges(b, part, **flags):
    """(i_lo, i_hi, j_lo, j_hi) of the u or the v part; a part without a cell has hi < lo on one axis."""
    i_start, i_end, i_endu, j_start, j_end, j_endv = ranges(b, **flags)
    return (i_start, i_endu, j_start, j_end) if part == "u" else (i_start, i_end, j_start, j_endv)


def empty(b, **flags):
    """Nothing to do: the empty tile, kte == kts, or both parts without a cell."""
    if b.ite < b.its or b.jte < b.jts or b.kte <= b.kts:
        return True
    return all(r[1] < r[0] or r[3] < r[2] for r in (part_ranges(b, "u", **flags), part_ranges(b, "v", **flags)))


def _part_slices(b, part, **flags):
    i_lo, i_hi, j_lo, j_hi = part_ranges(b, part, **flags)
    if b.ite < b.its or b.jte < b.jts or i_hi < i_lo or j_hi < j_lo:
        return None
    di, dj = (1, 0) if part == "u" else (0, 1)
    sj, si = slice(j_lo - b.jms, j_hi - b.jms + 1), slice(i_lo - b.ims, i_hi - b.ims + 1)
    nj, ni = slice(j_lo - dj - b.jms, j_hi - dj - b.jms + 1), slice(i_lo - di - b.ims, i_hi - di - b.ims + 1)
    return sj, si, nj, ni


def cell_mask(b, name, **flags):
    """Boolean, one member's shape of u or v: the cells a call may change."""
    m = np.zeros(shape(b, name), bool)
    s = _part_slices(b, name, **flags)
    if s is not None and b.kte > b.kts:
        m[s[0], b.kts - b.kms:b.kte - b.kms, s[1]] = True
    return m


def read_mask(b, name, non_hydrostatic, **flags):
    """Boolean, one member's shape of ``name``: the cells a call reads."""
    m = np.zeros(shape(b, name), bool)
    if b.kte <= b.kts:
        return m
    nh = bool(non_hydrostatic)
    k0, k1 = b.kts - b.kms, b.kte - b.kms                          # cells k0..k1-1; w levels k0..k1
    for part in ("u", "v"):
        s = _part_slices(b, part, **flags)
        if s is None:
            continue
        sj, si, nj, ni = s
        spots = [(sj, si)] if name in OWN[part] else [(sj, si), (nj, ni)] if name in BOTH else []
        if name in ("php", "mu") and not nh:
            spots = []
        for (aj, ai) in spots:
            if RANK[name] == 2:
                m[aj, ai] = True
            else:
                m[aj, k0:k1 + (1 if name == "ph" else 0), ai] = True
        if name == "rdnw" and nh:
            m[k0:k1] = True
        if name in ("fnm", "fnp") and nh:
            m[k0 + 1:k1] = True                                    # dpn(kts+1..kte-1)
    return m


def advance_uv(a, b, non_hydrostatic, rdx, rdy, dts, cf1, cf2, cf3, emdiv, periodic_x=False, specified=False, nested=False):
    """One momentum update on ``a``: name -> array for NAMES.  The scalars are rounded to the arrays' dtype first."""
    T = a["u"].dtype.type
    rdx, rdy, dts, cf1, cf2, cf3, emdiv = (T(x) for x in (rdx, rdy, dts, cf1, cf2, cf3, emdiv))
    half, zero = T(0.5), T(0)
    flags = dict(periodic_x=periodic_x, specified=specified, nested=nested)
    if b.kte <= b.kts:
        return a
    if non_hydrostatic and b.kde < 4:
        raise ValueError("non_hydrostatic needs kde >= 4")
    with np.errstate(all="ignore"):
        dx, dy = T(1) / rdx, T(1) / rdy
        new = {}
        for part in ("u", "v"):
            s = _part_slices(b, part, **flags)
            if s is None:
                continue
            sj, si, nj, ni = s
            own2, nb2 = (Ellipsis, sj, si), (Ellipsis, nj, ni)
            own = lambda name, k: a[name][(Ellipsis, sj, k - b.kms, si)]
            nb = lambda name, k: a[name][(Ellipsis, nj, k - b.kms, ni)]
            if part == "u":
                mr = a["msfux"][own2] / a["msfuy"][own2]
                rd, dd, mass, cq, tend = rdx, dx, a["muu"][own2], "cqu", "ru_tend"
            else:
                mr = a["msfvy"][own2] / a["msfvx"][own2]
                rd, dd, mass, cq, tend = rdy, dy, a["muv"][own2], "cqv", "rv_tend"
            c = mr * half
            c = c * rd
            c = c * mass
            md = (-emdiv) * dd
            md = md * (a["mudf"][own2] - a["mudf"][nb2])
            md = md / a["msfuy"][own2] if part == "u" else md * a["msfvx_inv"][own2]
            if non_hydrostatic:
                mrd = mr * rd
                hm = half * (a["mu"][nb2] + a["mu"][own2])
                sk = {k: own("p", k) + nb("p", k) for k in range(b.kts, b.kte)}
                dpn = {}
                t1, t2, t3 = cf1 * sk[b.kts], cf2 * sk[b.kts + 1], cf3 * sk[b.kts + 2]
                dpn[b.kts] = half * ((t1 + t2) + t3)
                for k in range(b.kts + 1, b.kte):
                    kk = k - b.kms
                    dpn[k] = half * ((a["fnm"][kk] * sk[k]) + (a["fnp"][kk] * sk[k - 1]))
                dpn[b.kte] = np.zeros_like(dpn[b.kts])
            out = []
            for k in range(b.kts, b.kte):
                g = (own("ph", k + 1) - nb("ph", k + 1)) + (own("ph", k) - nb("ph", k))
                g = g + ((own("alt", k) + nb("alt", k)) * (own("p", k) - nb("p", k)))
                g = g + ((own("al", k) + nb("al", k)) * (own("pb", k) - nb("pb", k)))
                dpxy = c * g
                if non_hydrostatic:
                    w = mrd * (own("php", k) - nb("php", k))
                    e = a["rdnw"][k - b.kms] * (dpn[k + 1] - dpn[k])
                    e = e - hm
                    dpxy = dpxy + (w * e)
                x = own(part, k) + (dts * own(tend, k))
                x = x - ((dts * own(cq, k)) * dpxy)
                out.append(x + md)
            new[part] = (sj, si, out)
        for part, (sj, si, out) in new.items():                    # u and v overlap no input: the order does not matter
            for n, k in enumerate(range(b.kts, b.kte)):
                a[part][(Ellipsis, sj, k - b.kms, si)] = out[n]
    return a


def nan_patterns(shape, dtype, tag):
    """Quiet NaNs whose payload names array ``tag`` and the cell."""
    u = np.uint64 if np.dtype(dtype).itemsize == 8 else np.uint32
    quiet = u(0x7FF8000000000000) if np.dtype(dtype).itemsize == 8 else u(0x7FC00000)
    n = int(np.prod(shape))
    assert n < (1 << 17) and tag < 31
    return (quiet | (np.arange(1, n + 1, dtype=u) + u((tag + 1) << 17))).reshape(shape).view(dtype)


def make_state(b, dtype, seed, non_hydrostatic, members=1, poison=True, **flags):
    """The 24 arrays of a call: finite values where the contract reads or writes (map factors and masses in 0.5..1.5, the
    rest in -2..2), and with ``poison`` a NaN with a payload of its own in every other cell."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, name in enumerate(NAMES):
        shp = shape(b, name, members)
        keep = read_mask(b, name, non_hydrostatic, **flags)
        if name in OUT_3D:
            keep = keep | cell_mask(b, name, **flags)
        keep = np.broadcast_to(keep, shp)
        lo, hi = (0.5, 1.5) if name in MSF_2D + ("muu", "muv") else (-2.0, 2.0)
        a = rng.uniform(lo, hi, shp).astype(dtype)
        if poison:
            a[~keep] = nan_patterns(shp, dtype, k)[~keep]
        out[name] = a
    return out
