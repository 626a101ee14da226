"""numpy restatement of the two records of include/amt_advance_mu_t.h section 10 (amt_field_stats, amt_field_diff) for ONE
member: ``a`` is that member's array in the package's layout -- (jdim, kdim, idim) for a rank-3 field, (jdim, idim) for a
rank-2 one -- ``extents = (ims, ime, jms, jme, kms, kme)`` its Fortran memory extents and ``box = (i0, i1, k0, k1, j0, j1)``
Fortran-inclusive (rank 2 ignores the k entries).  Offsets count elements from the member's base."""
import math

import numpy as np


def box_index(a, extents, box):
    ims, _ime, jms, _jme, kms, _kme = extents
    i0, i1, k0, k1, j0, j1 = box
    if a.ndim == 3:
        return (slice(j0 - jms, j1 - jms + 1), slice(k0 - kms, k1 - kms + 1), slice(i0 - ims, i1 - ims + 1))
    return (slice(j0 - jms, j1 - jms + 1), slice(i0 - ims, i1 - ims + 1))


def default_extents(a):
    if a.ndim == 3:
        return (0, a.shape[2] - 1, 0, a.shape[0] - 1, 0, a.shape[1] - 1)
    return (0, a.shape[1] - 1, 0, a.shape[0] - 1, 0, 0)


def _box(a, extents, box):
    extents = default_extents(a) if extents is None else extents
    if box is None:
        ims, ime, jms, jme, kms, kme = extents
        box = (ims, ime, kms, kme, jms, jme)
    idx = box_index(a, extents, box)
    offsets = np.arange(a.size, dtype=np.int64).reshape(a.shape)[idx].ravel()
    return idx, offsets


def stats(a, extents=None, box=None) -> dict:
    idx, offsets = _box(a, extents, box)
    x = a[idx].ravel()
    nan = np.isnan(x)
    inf = np.isinf(x)
    bad = nan | inf
    fin = x[~bad].astype(np.float64)                    # exact for float32
    return dict(count=int(x.size), n_nan=int(nan.sum()), n_inf=int(inf.sum()),
                first_nonfinite=int(offsets[bad].min()) if bad.any() else -1,
                min=float(fin.min()) if fin.size else math.inf,
                max=float(fin.max()) if fin.size else -math.inf,
                max_abs=float(np.abs(fin).max()) if fin.size else 0.0,
                sum=math.fsum(fin.tolist()),
                abs_sum=math.fsum(np.abs(fin).tolist()))     # not part of the record: the scale of the sum's error bound


def sum_bound(count: int, abs_sum: float) -> float:
    """|computed - exact| of ANY order of n - 1 double additions of n doubles: gamma_{n-1} * sum |x|, gamma_k = k u / (1 - k u),
    u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2)."""
    u = 2.0 ** -53
    k = max(count - 1, 0)
    return k * u / (1.0 - k * u) * abs_sum


def diff(a, b, extents=None, box=None) -> dict:
    assert a.shape == b.shape and a.dtype == b.dtype
    idx, offsets = _box(a, extents, box)
    x, y = a[idx].ravel(), b[idx].ravel()
    u = np.uint64 if a.dtype.itemsize == 8 else np.uint32
    differ = x.view(u) != y.view(u)
    both = np.isfinite(x) & np.isfinite(y)
    with np.errstate(over="ignore", invalid="ignore"):
        d = np.abs(x[both].astype(np.float64) - y[both].astype(np.float64))
    return dict(count=int(x.size), n_diff=int(differ.sum()),
                first_diff=int(offsets[differ].min()) if differ.any() else -1,
                max_abs_diff=float(d.max()) if d.size else 0.0)
