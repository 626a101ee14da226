"""TEST INFRASTRUCTURE: numpy statement of the cyclic (periodic) lateral boundary refresh, written from its definition and
independent of the library (include/amt_advance_mu_t.h section 9).

Fortran indices are global.  i_start..i_end, j_start..j_end is the compute window of module_small_step_em.f90:91-106,
restated here so that nothing of the library is involved.

* cyclic x, period ide - ids: column ide receives column ids of u, u_1, t_1, muu, msfuy; column ids-1 receives column ide-1
  of t_1.  Rows j_start..j_end, every memory level.
* cyclic y, period jde - jds: row jde receives row jds of v, v_1, t_1, muv, msfvx_inv; row jds-1 receives row jde-1 of t_1.
  Columns i_start..i_end, every memory level.

Corner cells are not written.  Arrays are (jdim, kdim, idim) / (jdim, idim) as everywhere in the tests, or member-stacked with
one more leading axis; the copy then happens in every member.
"""
import numpy as np

CYCLIC_X, CYCLIC_Y = 1, 2
COLS_FROM_RIGHT = ("u", "u_1", "t_1", "muu", "msfuy")
COLS_FROM_LEFT = ("t_1",)
ROWS_FROM_ABOVE = ("v", "v_1", "t_1", "muv", "msfvx_inv")
ROWS_FROM_BELOW = ("t_1",)
RANK3 = ("u", "u_1", "v", "v_1", "t_1")                      # (.., j, k, i); the others are (.., j, i)
MAY_CHANGE = ("u", "u_1", "v", "v_1", "t_1", "muu", "muv", "msfuy", "msfvx_inv")


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


def cyclic_fill(arrays, bounds, axes, flags=(0, 0, 0)):
    """Refresh the wrap cells of ``arrays`` (name -> numpy array) in place and return ``arrays``."""
    b = bounds
    i0, i1, j0, j1 = window(flags, b)
    J = slice(j0 - b.jms, j1 - b.jms + 1)
    I = slice(i0 - b.ims, i1 - b.ims + 1)
    col = lambda i: i - b.ims
    row = lambda j: j - b.jms
    if axes & CYCLIC_X:
        for n in COLS_FROM_RIGHT:
            a = arrays[n]
            if n in RANK3:
                a[..., J, :, col(b.ide)] = a[..., J, :, col(b.ids)]
            else:
                a[..., J, col(b.ide)] = a[..., J, col(b.ids)]
        for n in COLS_FROM_LEFT:
            a = arrays[n]
            a[..., J, :, col(b.ids - 1)] = a[..., J, :, col(b.ide - 1)]
    if axes & CYCLIC_Y:
        for n in ROWS_FROM_ABOVE:
            a = arrays[n]
            if n in RANK3:
                a[..., row(b.jde), :, I] = a[..., row(b.jds), :, I]
            else:
                a[..., row(b.jde), I] = a[..., row(b.jds), I]
        for n in ROWS_FROM_BELOW:
            a = arrays[n]
            a[..., row(b.jds - 1), :, I] = a[..., row(b.jde - 1), :, I]
    return arrays


def as_bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)
