"""numpy statement of include/amt_advance_mu_t.h section 13: ensemble mean, sample variance and envelope over the members of a
member-stacked field.  ``a`` has shape (members, jdim, kdim, idim) for a rank-3 field and (members, jdim, idim) for a rank-2
one; ``extents = (ims, ime, jms, jme, kms, kme)`` and ``box = (i0, i1, k0, k1, j0, j1)`` as in diag_ref (rank 2 ignores k).
``moments`` returns the four arrays OVER THE BOX (shape of ``a[0][box_index]``), in ``a``'s dtype.

It loops over the members, as the contract does, and works elementwise on float64 arrays: every operation is one IEEE
operation per cell, so the bits are defined and there is nothing to tolerate."""
import numpy as np

from diag_ref import box_index, default_extents

NAMES = ("mean", "var", "lo", "hi")


def member_index(a, extents=None, box=None):
    """Index of the box in ONE member's array."""
    one = a[0]
    extents = default_extents(one) if extents is None else extents
    if box is None:
        ims, ime, jms, jme, kms, kme = extents
        box = (ims, ime, kms, kme, jms, jme)
    return box_index(one, extents, box)


def moments(a, extents=None, box=None) -> dict:
    idx = member_index(a, extents, box)
    dtype = a.dtype
    members = a.shape[0]
    x = [np.array(a[m][idx]) for m in range(members)]                  # copies: cells outside the box are never looked at
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        s = x[0].astype(np.float64)
        for m in range(1, members):
            s = s + x[m].astype(np.float64)
        mean_d = s / np.float64(members)
        q = np.zeros_like(mean_d)
        for m in range(members):
            d = x[m].astype(np.float64) - mean_d
            q = q + d * d
        var_d = q / np.float64(max(members - 1, 1))
        lo, hi = x[0].copy(), x[0].copy()
        nan = np.isnan(x[0])
        for m in range(1, members):
            lo = np.where(x[m] < lo, x[m], lo)
            hi = np.where(x[m] > hi, x[m], hi)
            nan = nan | np.isnan(x[m])
        lo = np.where(nan, dtype.type(np.nan), lo)
        hi = np.where(nan, dtype.type(np.nan), hi)
        return dict(mean=mean_d.astype(dtype), var=var_d.astype(dtype), lo=lo.astype(dtype), hi=hi.astype(dtype))


def expected(before, ref, idx):
    """One member-shaped output array after a call: ``before`` with the box replaced by ``ref``."""
    out = before.copy()
    out[idx] = ref
    return out
