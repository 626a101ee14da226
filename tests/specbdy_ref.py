"""TEST INFRASTRUCTURE: numpy statement of the boundary-zone update of specified / nested lateral boundaries, written from its
definition and independent of the library (include/amt_advance_mu_t.h section 12).

Fortran indices are global.  i_start..i_end, j_start..j_end is the compute window of module_small_step_em.f90:91-106, restated
here so that nothing of the library is involved.  With ihi = min(ite, ide-1), jhi = min(jte, jde-1) the BOUNDARY ZONE of a tile
is every cell (i, j), its <= i <= ihi, jts <= j <= jhi, that is not in the window.  The update, each zone cell once:

    t(i,k,j)  = t(i,k,j)  + dts * ft(i,k,j)        k = kts .. kte-1
    mu(i,j)   = mu(i,j)   + dts * mu_tend(i,j)
    muts(i,j) = muts(i,j) + dts * mu_tend(i,j)

two roundings in the arrays' dtype (product, then sum); for fp32 dts is rounded to float first.  Everything else keeps its
bits.  The zone is a MASK here -- tile mass points minus window --, not a list of strips.

Arrays are (jdim, kdim, idim) / (jdim, idim) as everywhere in the tests, or member-stacked with one more leading axis; the
update then happens in every member.
"""
import numpy as np

MAY_CHANGE = ("t", "mu", "muts")


def window(flags, b):
    """(i_start, i_end, j_start, j_end); flags = (periodic_x, specified, nested)."""
    periodic_x, specified, nested = (bool(x) for x in flags)
    i_start, i_end = b.its, min(b.ite, b.ide - 1)
    j_start, j_end = b.jts, min(b.jte, b.jde - 1)
    if (specified or nested) and not periodic_x:
        i_start, i_end = max(b.its, b.ids + 1), min(b.ite, b.ide - 2)
    if specified or nested:
        j_start, j_end = max(b.jts, b.jds + 1), min(b.jte, b.jde - 2)
    return i_start, i_end, j_start, j_end


def _box(b, i0, i1, j0, j1):
    """Boolean (jdim, idim) mask of the memory cells i0..i1, j0..j1 (empty ranges give an empty box)."""
    m = np.zeros((b.jme - b.jms + 1, b.ime - b.ims + 1), bool)
    if i1 >= i0 and j1 >= j0:
        m[j0 - b.jms: j1 - b.jms + 1, i0 - b.ims: i1 - b.ims + 1] = True
    return m


def tile_mask(b):
    """The tile's mass points its..min(ite, ide-1), jts..min(jte, jde-1)."""
    return _box(b, b.its, min(b.ite, b.ide - 1), b.jts, min(b.jte, b.jde - 1))


def window_mask(flags, b):
    i0, i1, j0, j1 = window(flags, b)
    return _box(b, i0, i1, j0, j1) if (i1 >= i0 and j1 >= j0) else _box(b, 0, -1, 0, -1)


def zone_mask(flags, b):
    """(jdim, idim) mask of the boundary zone: the tile's mass points that are not in the compute window."""
    return tile_mask(b) & ~window_mask(flags, b)


def spec_bdy_update(arrays, bounds, flags, dts):
    """Advance the zone's cells of ``arrays`` (name -> numpy array; t, ft, mu, muts, mu_tend are used) in place and return
    ``arrays``."""
    b = bounds
    zone = zone_mask(flags, b)
    dt = arrays["t"].dtype
    s = dt.type(dts)                                             # fp32: dts rounded to float first
    k0, k1 = b.kts - b.kms, b.kte - 1 - b.kms                    # memory levels of kts .. kte-1
    jj, ii = np.nonzero(zone)
    if k1 >= k0:
        t, ft = arrays["t"], arrays["ft"]
        step = s * ft[..., jj, k0:k1 + 1, ii]                    # one rounding
        t[..., jj, k0:k1 + 1, ii] = t[..., jj, k0:k1 + 1, ii] + step     # and another
        assert step.dtype == dt
    tend = s * arrays["mu_tend"][..., jj, ii]
    assert tend.dtype == dt
    for name in ("mu", "muts"):
        a = arrays[name]
        a[..., jj, ii] = a[..., jj, ii] + tend
    return arrays


def as_bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)
