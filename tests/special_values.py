"""Special values layered over a patch in the tests only (pure numpy): exact and negative zeros, subnormals, overflow to
Inf and Inf - Inf, planted NaN / Inf / zero divisors, and NaN in every cell the routine does not read.

Every other test feeds the kernels one benign band of values (include/amt_synth.h: t near 300, u near 10, mut near 9e4, map
factors in [0.9, 1.1], ww near 0 but never 0).  On that band an accumulator seeded with its first term instead of 0, a flushed
denormal, a divide that is not correctly rounded on a subnormal quotient, or a read of a cell the Fortran never reads (times
zero, or staged and dropped) all give the Fortran's bits.  Here they do not.

* ``apply(patch, regime, seed)``: overlay the named, seeded regime on a host patch (numpy, in place) and return it; device
  patches go through ``to_host`` / ``to_device``.  Regimes: ``rest``, ``signed_zeros``, ``denormal``, ``overflow``,
  ``planted_composite``, ``unread_poison``.
* ``planted(patch, field, value, where)``: one cell of one input set to a quiet NaN, +Inf, -Inf or 0.0.
* ``read_mask(patch)``: per array, the cells the Fortran reads; tests/test_special_values_cpu.py
  holds it against the oracle: NaN everywhere else changes no output bit.
* ``same_up_to_nan_payload(a, b)``: NaN at the same cells (sign and payload not compared: x86 generates the negative default
  NaN, gfx950 the positive one, and operand order decides the payload that propagates), every other cell equal as bits.
"""
from __future__ import annotations

import numpy as np

# the state a WRF run started at rest holds as exact zeros
ELEVEN = ("u", "v", "u_1", "v_1", "ww", "ww_1", "ft", "mu_tend", "mu", "t", "t_1")
RANK3 = ("ww", "ww_1", "u", "u_1", "v", "v_1", "t", "t_1", "t_ave", "ft")
RANK1 = ("dnw", "fnm", "fnp", "rdnw")
OUTPUTS = ("ww", "t", "t_ave", "mu", "muave", "muts", "mudf")
INTENT_OUT = ("t_ave", "muave", "muts", "mudf")                  # written before they are read, if they are read at all
REGIMES = ("rest", "signed_zeros", "denormal", "overflow", "planted_composite", "unread_poison")

# `denormal`: the eleven fields times 2**DENORMAL_SCALE[itemsize]; t (about 2**8) then lies a few bits below the smallest
# normal number, ww and the products dnw * dvdxi deeper in the subnormal range (tests/test_special_values_cpu.py asserts
# the share of subnormal cells on the oracle)
DENORMAL_SCALE = {4: -137, 8: -1033}
# `overflow`: about 2 % of the cells of u, v, ww_1, t_1 times 2**OVERFLOW_SCALE[itemsize][field], of either sign
OVERFLOW_SCALE = {4: dict(u=116, v=116, ww_1=122, t_1=112), 8: dict(u=1012, v=1012, ww_1=1018, t_1=1008)}
OVERFLOW_SHARE = 0.02


def rank(name: str) -> int:
    return 3 if name in RANK3 else 1 if name in RANK1 else 2


def window(patch):
    """(i_start, i_end, j_start, j_end, k_start, k_end) of module_small_step_em.f90:91-106 (amt_compute_window)."""
    b, c = patch.bounds, patch.config
    i0, i1, j0, j1 = b.its, min(b.ite, b.ide - 1), b.jts, min(b.jte, b.jde - 1)
    if not c.periodic_x and (c.specified or c.nested):
        i0, i1 = max(b.its, b.ids + 1), min(b.ite, b.ide - 2)
    if c.specified or c.nested:
        j0, j1 = max(b.jts, b.jds + 1), min(b.jte, b.jde - 2)
    return i0, i1, j0, j1, b.kts, b.kte - 1


def _box(patch, name, i0, i1, j0, j1, k0=None, k1=None):
    """Index of the Fortran-inclusive box in the memory of array ``name``."""
    b = patch.bounds
    js, is_ = slice(j0 - b.jms, j1 - b.jms + 1), slice(i0 - b.ims, i1 - b.ims + 1)
    if rank(name) == 3:
        return (js, slice(k0 - b.kms, k1 - b.kms + 1), is_)
    return (js, is_)


def window_index(patch, name):
    """Index of the compute window in array ``name`` (rank 3: levels 1..k_end; rank 2)."""
    i0, i1, j0, j1, _k0, k1 = window(patch)
    return _box(patch, name, i0, i1, j0, j1, 1, k1)


def read_mask(patch) -> dict:
    """name -> bool array: True where the Fortran reads the cell as an INPUT.  ww is read at level 1 only (levels 2..k_end
    are written first, :159-163), the INTENT(OUT) arrays nowhere; dnw, rdnw at 1..k_end, fnm, fnp at 2..k_end."""
    i0, i1, j0, j1, _k0, k1 = window(patch)
    b = patch.bounds
    m = {n: np.zeros(a.shape, bool) for n, a in patch.arrays.items()}
    for n in ("msftx", "msfty", "mu", "mut", "mu_tend"):
        m[n][_box(patch, n, i0, i1, j0, j1)] = True
    for n in ("t", "ft", "ww_1"):
        m[n][_box(patch, n, i0, i1, j0, j1, 1, k1)] = True
    m["ww"][_box(patch, "ww", i0, i1, j0, j1, 1, 1)] = True
    for n in ("v", "v_1", "muv", "msfvx_inv"):                   # row j + 1 (:143, :241)
        m[n][_box(patch, n, i0, i1, j0, j1 + 1, 1, k1)] = True
    for n in ("u", "u_1", "muu", "msfuy"):                       # column i + 1 (:145, :244)
        m[n][_box(patch, n, i0, i1 + 1, j0, j1, 1, k1)] = True
    m["t_1"][_box(patch, "t_1", i0, i1, j0 - 1, j1 + 1, 1, k1)] = True      # a cross: no corners
    m["t_1"][_box(patch, "t_1", i0 - 1, i1 + 1, j0, j1, 1, k1)] = True
    for n in ("dnw", "rdnw"):
        m[n][1 - b.kms:k1 - b.kms + 1] = True
    for n in ("fnm", "fnp"):
        m[n][2 - b.kms:k1 - b.kms + 1] = True
    return m


def _uint(dt):
    return np.uint64 if np.dtype(dt).itemsize == 8 else np.uint32


def quiet_nan(dt, negative=False):
    u = _uint(dt)
    bits = (0x7FF8000000000000 if u is np.uint64 else 0x7FC00000) | ((1 << (8 * np.dtype(dt).itemsize - 1)) if negative else 0)
    return np.array([bits], dtype=u).view(dt)[0]


def _rng(regime, seed, patch):
    b = patch.bounds
    return np.random.default_rng([REGIMES.index(regime), int(seed), b.idim, b.kdim, b.jdim, patch.arrays["t"].dtype.itemsize])


# ---------------------------------------------------------------------------------------------
# regimes
# ---------------------------------------------------------------------------------------------
def _rest(patch, seed):
    for n in ELEVEN:
        patch.arrays[n][...] = 0.0


def _signed_zeros(patch, seed):
    """A third of the cells of the eleven fields +0.0, a third -0.0; on top, whole window rows and whole columns of -0.0 in
    u, v, u_1, v_1, mu_tend, ww and ww_1 together, so that dmdt there is a sum of negative-zero terms only.  dts changes its
    sign: dmdt starts from +0.0 and a sum is -0.0 only if every term is, so dmdt + mu_tend is never -0.0, and with dts > 0
    mu = mu + dts * (dmdt + mu_tend) could not be -0.0 at all; with dts < 0 it is wherever mu was -0.0 and the bracket +0.0,
    and a dmdt seeded with its first term (-0.0) turns that cell into +0.0."""
    patch.dts = -abs(patch.dts)
    rng = _rng("signed_zeros", seed, patch)
    a = patch.arrays
    t_1 = a["t_1"].copy()
    for n in ELEVEN:
        r = rng.random(a[n].shape)
        a[n][r < 1 / 3] = 0.0
        a[n][(r >= 1 / 3) & (r < 2 / 3)] = -0.0
    i0, i1, j0, j1, _k0, k1 = window(patch)
    b = patch.bounds
    rows = sorted({j0, j1, int(rng.integers(j0, j1 + 1))})
    cols = sorted({i0, i1, int(rng.integers(i0, i1 + 1))})
    for n in ("u", "v", "u_1", "v_1", "mu_tend", "ww", "ww_1"):
        for j in rows:                                           # rows j and j + 1 of the v family, every column
            a[n][j - b.jms:j - b.jms + 2] = -0.0
        for i in cols:                                           # columns i and i + 1 of the u family, every row
            a[n][..., i - b.ims:i - b.ims + 2] = -0.0
    # One cell whose t must come out -0.0: t = (-0 + msfty*dts*ft) - dts*msfty*X is -0.0 only if ft = +0.0 and X = -0.0, and X
    # only if both flux differences are (-0) - (+0) over positive t_1 sums.  In the middle forced column (ww there is zero):
    i, j = cols[len(cols) // 2], (j0 + j1) // 2
    k = (1 + k1) // 2
    J, K, I = j - b.jms, k - b.kms, i - b.ims
    a["u"][J, K, I], a["u"][J, K, I + 1], a["v"][J, K, I], a["v"][J + 1, K, I] = 0.0, -0.0, 0.0, -0.0
    a["u_1"][J, K, I:I + 2] = -0.0
    a["v_1"][J:J + 2, K, I] = -0.0
    a["t"][J, K, I], a["ft"][J, K, I] = -0.0, 0.0
    for dj, dk, di in ((0, 0, 0), (0, 0, -1), (0, 0, 1), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0)):
        if 0 <= K + dk < b.kdim:
            a["t_1"][J + dj, K + dk, I + di] = t_1[J + dj, K + dk, I + di]


def _denormal(patch, seed):
    s = np.ldexp(patch.arrays["t"].dtype.type(1), DENORMAL_SCALE[patch.arrays["t"].dtype.itemsize])
    for n in ELEVEN:
        patch.arrays[n] *= s


def _overflow(patch, seed):
    rng = _rng("overflow", seed, patch)
    dt = patch.arrays["t"].dtype
    for n, e in OVERFLOW_SCALE[dt.itemsize].items():
        a = patch.arrays[n]
        hit = rng.random(a.shape) < OVERFLOW_SHARE
        sign = np.where(rng.random(a.shape) < 0.5, -1.0, 1.0).astype(dt)
        with np.errstate(over="raise"):
            a[hit] = (np.abs(a[hit]) + dt.type(1)) * sign[hit] * np.ldexp(dt.type(1), e)


# (field, value) of the composite's plants, in the order they are placed
_COMPOSITE = (("u", "nan"), ("t_1", "+inf"), ("v_1", "-inf"), ("msfty", "zero"), ("ft", "nan"), ("muu", "+inf"),
              ("ww_1", "-inf"), ("mu_tend", "nan"), ("t", "+inf"), ("msfuy", "zero"), ("ww", "nan"), ("muv", "-inf"))


def composite_sites(patch, seed, columns=()):
    """[(field, value, (i, k, j))]: plants at least four columns and two rows apart.  ``columns``: window columns that
    must carry a plant (a tile's last column, the next tile's first, ...); further ones are drawn.  Column i_end + 1
    (the halo column of the u family and t_1) is always among them, with a field that is read there."""
    rng = _rng("planted_composite", seed, patch)
    i0, i1, j0, j1, _k0, k1 = window(patch)
    want = [int(c) for c in columns if i0 <= c <= i1 + 1] + [i1 + 1]
    free = list(rng.permutation(np.arange(i0, i1 + 1)))
    sites, used = [], []

    def far(i, j):
        return all(abs(i - ui) >= 4 or abs(j - uj) >= 2 for ui, uj in used)

    rows = list(range(j0, j1 + 1))
    for n, (field, value) in enumerate(_COMPOSITE * 2):
        if want:
            i = want.pop(0)
        elif free:
            i = int(free.pop(0))
        else:
            break
        if i == i1 + 1:
            field = ("u", "t_1", "u_1", "muu", "msfuy")[n % 5]
            value = "nan" if field != "msfuy" else "zero"
        j = next((int(r) for r in rng.permutation(rows) if far(i, r)), None)
        if j is None:
            continue
        used.append((i, j))
        sites.append((field, value, (i, int(rng.integers(1, k1 + 1)), j)))
        if len(sites) >= 12 and not want:
            break
    return sites


def _planted_composite(patch, seed, columns=()):
    for field, value, (i, k, j) in composite_sites(patch, seed, columns):
        plant_at(patch, field, value, i, k, j)


def _unread_poison(patch, seed):
    nan = (quiet_nan(patch.arrays["t"].dtype), quiet_nan(patch.arrays["t"].dtype, negative=True))
    for n, read in read_mask(patch).items():
        a = patch.arrays[n]
        flat = np.flatnonzero(~read.ravel())
        a.ravel()[flat[0::2]] = nan[0]
        a.ravel()[flat[1::2]] = nan[1]


_APPLY = {"rest": _rest, "signed_zeros": _signed_zeros, "denormal": _denormal, "overflow": _overflow,
          "planted_composite": _planted_composite, "unread_poison": _unread_poison}


def apply(patch, regime: str, seed: int = 0, **kw):
    """Overlay ``regime`` on the host patch ``patch`` in place; returns it."""
    if any(hasattr(a, "is_cuda") for a in patch.arrays.values()):
        raise TypeError("apply works on host patches: use to_host() / to_device()")
    _APPLY[regime](patch, seed, **kw)
    return patch


# ---------------------------------------------------------------------------------------------
# single plants
# ---------------------------------------------------------------------------------------------
VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "zero": 0.0}
PLANT_FIELDS = ("u", "u_1", "v", "v_1", "ww", "ww_1", "t", "t_1", "ft", "mu", "mut", "muu", "muv", "mu_tend",
                "msfuy", "msfvx_inv", "msftx", "msfty")
ZERO_DIVISORS = ("msfty", "msfuy", "msftx", "mut")
WHERE = ("interior", "first_column", "last_column", "first_row", "last_row")
# the halo cells the stencil does read
HALO_WHERE = {"halo_right": ("u", "u_1", "muu", "msfuy", "t_1"), "halo_above": ("v", "v_1", "muv", "msfvx_inv", "t_1"),
              "halo_left": ("t_1",), "halo_below": ("t_1",)}


def site(patch, field, where):
    """(i, k, j) of ``where`` for ``field``: k is the middle level of 1..k_end, but level 1 for ww (the only level of ww the
    routine reads)."""
    i0, i1, j0, j1, _k0, k1 = window(patch)
    im, jm = (i0 + i1) // 2, (j0 + j1) // 2
    k = 1 if field == "ww" else (1 + k1) // 2 if k1 > 1 else 1
    i, j = {"interior": (im, jm), "first_column": (i0, jm), "last_column": (i1, jm), "first_row": (im, j0),
            "last_row": (im, j1), "halo_right": (i1 + 1, jm), "halo_above": (im, j1 + 1), "halo_left": (i0 - 1, jm),
            "halo_below": (im, j0 - 1)}[where]
    return i, k, j


def plant_at(patch, field, value, i, k, j):
    b = patch.bounds
    a = patch.arrays[field]
    v = a.dtype.type(VALUES[value])
    if rank(field) == 3:
        a[j - b.jms, k - b.kms, i - b.ims] = v
    else:
        a[j - b.jms, i - b.ims] = v
    return patch


def planted(patch, field, value, where):
    """One cell of input ``field`` of the host patch set to ``value`` ("nan", "+inf", "-inf", "zero") at ``where``."""
    if where in HALO_WHERE and field not in HALO_WHERE[where]:
        raise ValueError(f"{field} is not read at {where}")
    return plant_at(patch, field, value, *site(patch, field, where))


def single_plants():
    """[(field, value, where)]: every input field x {NaN, +Inf, -Inf} (and 0.0 for the divisors) x the five window places and
    the halo places at which the field is read."""
    out = []
    for f in PLANT_FIELDS:
        wheres = list(WHERE) + [w for w, fields in HALO_WHERE.items() if f in fields]
        for v in ("nan", "+inf", "-inf") + (("zero",) if f in ZERO_DIVISORS else ()):
            out += [(f, v, w) for w in wheres]
    return out


# ---------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------
def canonical_nan(a):
    """A copy of ``a`` with every NaN replaced by the positive quiet NaN without payload."""
    out = np.ascontiguousarray(a).copy()
    out[np.isnan(out)] = quiet_nan(out.dtype)
    return out


def same_up_to_nan_payload(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    u = _uint(a.dtype)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def outside_window_bits_equal(patch, name, got, before) -> bool:
    """Every cell of ``got`` outside the compute window has the bits of ``before``: untouched cells keep NaN payloads, -0.0."""
    u = _uint(got.dtype)
    out = np.ones(got.shape, bool)
    out[window_index(patch, name)] = False
    return bool(np.array_equal(np.ascontiguousarray(got).view(u)[out], np.ascontiguousarray(before).view(u)[out]))


def first_difference(a, b):
    """(index, a value, b value) of the first cell that differs under same_up_to_nan_payload, for messages; None if none."""
    na, nb = np.isnan(a), np.isnan(b)
    u = _uint(a.dtype)
    bad = (na != nb) | (~na & ~nb & (a.view(u) != b.view(u)))
    if not bad.any():
        return None
    idx = tuple(int(x) for x in np.argwhere(bad)[0])
    return idx, a[idx], b[idx], int(bad.sum())


# ---------------------------------------------------------------------------------------------
# Reference-anchored cases (tests/golden/special_values_digests.json, written by tests/golden/make_golden.py)
# ---------------------------------------------------------------------------------------------
SHAPES = ("16x8x16", "37x5x11_ragged", "48x41x20_tile")
PLANT_SHAPE = "37x5x11_ragged"
SEED = 2029


def base_case(pkg, shape, flag, dtype):
    """The patch the regimes are laid over: hard_inputs.hard_case with the rk3 scalars (dts = 20/3)."""
    import hard_inputs
    return hard_inputs.hard_case(pkg, shape, flag, dtype, "rk3_dx12km")


def special_case(pkg, key):
    """'<shape>/<flags>/<dtype>/<regime>' or '<shape>/<flags>/<dtype>/plant:<field>:<value>:<where>' -> host patch."""
    shape, flag, dtname, what = key.split("/")
    p = base_case(pkg, shape, flag, np.dtype(dtname))
    if what.startswith("plant:"):
        _, field, value, where = what.split(":")
        return planted(p, field, value, where)
    return apply(p, what, SEED)


def regime_keys():
    import cases
    return [f"{s}/{f}/{np.dtype(dt).name}/{r}" for s in SHAPES for f in cases.FLAG_COMBOS for dt in (np.float32, np.float64)
            for r in REGIMES]


def plant_keys():
    return [f"{PLANT_SHAPE}/none/{np.dtype(dt).name}/plant:{f}:{v}:{w}" for dt in (np.float32, np.float64)
            for f, v, w in single_plants()]

