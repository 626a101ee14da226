"""tests/uv_ref.py, the numpy statement of advance_uv (include/amt_advance_mu_t.h section 17), held to a three-loop scalar
transcription of the contract and to physical identities.  No device, no library call."""
import numpy as np
import pytest

import uv_ref as R

F64, F32 = np.float64, np.float32
SC = dict(rdx=1.0e-3, rdy=1.25e-3, dts=2.0, cf1=1.5, cf2=-0.75, cf3=0.25, emdiv=0.01)
FLAGS = [(0, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 0)]


def _flags(f):
    return dict(periodic_x=bool(f[0]), specified=bool(f[1]), nested=bool(f[2]))


def _whole(pkg, ni=6, nk=5, nj=5):
    return pkg.synth.Bounds(ids=1, ide=ni, jds=1, jde=nj, kde=nk, ims=0, ime=ni + 1, jms=0, jme=nj + 1, kms=0, kme=nk + 1,
                            its=1, ite=ni, jts=1, jte=nj, kts=1, kte=nk)


def _interior(pkg, ni=6, nk=5, nj=5):
    return pkg.synth.Bounds(ids=1, ide=ni + 20, jds=1, jde=nj + 12, kde=nk, ims=3, ime=ni + 7, jms=2, jme=nj + 5, kms=-1, kme=nk + 1,
                            its=5, ite=ni + 4, jts=4, jte=nj + 3, kts=1, kte=nk)


def _scalar(a, b, nh, flags, sc):
    """The contract, cell by cell, in Python scalars of the arrays' type: three loops per part."""
    T = a["u"].dtype.type
    rdx, rdy, dts, cf1, cf2, cf3, emdiv = (T(sc[k]) for k in ("rdx", "rdy", "dts", "cf1", "cf2", "cf3", "emdiv"))
    half = T(0.5)
    dx, dy = T(1) / rdx, T(1) / rdy
    at3 = lambda n, i, k, j: a[n][j - b.jms, k - b.kms, i - b.ims]
    at2 = lambda n, i, j: a[n][j - b.jms, i - b.ims]
    lev = lambda n, k: a[n][k - b.kms]
    new = {}
    with np.errstate(all="ignore"):
        for part in ("u", "v"):
            i_lo, i_hi, j_lo, j_hi = R.part_ranges(b, part, **flags)
            di, dj = (1, 0) if part == "u" else (0, 1)
            for j in range(j_lo, j_hi + 1):
                for i in range(i_lo, i_hi + 1):
                    ii, jj = i - di, j - dj
                    if part == "u":
                        mr = at2("msfux", i, j) / at2("msfuy", i, j)
                        rd, dd, mass, cq, tend = rdx, dx, at2("muu", i, j), "cqu", "ru_tend"
                    else:
                        mr = at2("msfvy", i, j) / at2("msfvx", i, j)
                        rd, dd, mass, cq, tend = rdy, dy, at2("muv", i, j), "cqv", "rv_tend"
                    c = ((mr * half) * rd) * mass
                    md = ((-emdiv) * dd) * (at2("mudf", i, j) - at2("mudf", ii, jj))
                    md = md / at2("msfuy", i, j) if part == "u" else md * at2("msfvx_inv", i, j)
                    if nh:
                        s = {k: at3("p", i, k, j) + at3("p", ii, k, jj) for k in range(b.kts, b.kte)}
                        dpn = {b.kts: half * (((cf1 * s[1]) + (cf2 * s[2])) + (cf3 * s[3])), b.kte: T(0)}
                        for k in range(b.kts + 1, b.kte):
                            dpn[k] = half * ((lev("fnm", k) * s[k]) + (lev("fnp", k) * s[k - 1]))
                    for k in range(b.kts, b.kte):
                        g = (((at3("ph", i, k + 1, j) - at3("ph", ii, k + 1, jj)) + (at3("ph", i, k, j) - at3("ph", ii, k, jj)))
                             + ((at3("alt", i, k, j) + at3("alt", ii, k, jj)) * (at3("p", i, k, j) - at3("p", ii, k, jj)))) \
                            + ((at3("al", i, k, j) + at3("al", ii, k, jj)) * (at3("pb", i, k, j) - at3("pb", ii, k, jj)))
                        dpxy = c * g
                        if nh:
                            dpxy = dpxy + (((mr * rd) * (at3("php", i, k, j) - at3("php", ii, k, jj)))
                                           * ((lev("rdnw", k) * (dpn[k + 1] - dpn[k])) - (half * (at2("mu", ii, jj) + at2("mu", i, j)))))
                        new[(part, i, k, j)] = ((at3(part, i, k, j) + (dts * at3(tend, i, k, j))) - ((dts * at3(cq, i, k, j)) * dpxy)) + md
    for (part, i, k, j), x in new.items():
        a[part][j - b.jms, k - b.kms, i - b.ims] = x
    return a


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "p%ds%dn%d" % f)
@pytest.mark.parametrize("nh", [0, 1])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_numpy_statement_equals_the_scalar_transcription(pkg, dtype, nh, flags):
    for b in (_whole(pkg), _interior(pkg), _whole(pkg, 2, 4, 2), _interior(pkg, 1, 4, 1)):
        f = _flags(flags)
        a = R.make_state(b, dtype, 3, nh, **f)
        want = _scalar({n: x.copy() for n, x in a.items()}, b, nh, f, SC)
        got = R.advance_uv({n: x.copy() for n, x in a.items()}, b, nh, **SC, **f)
        for n in R.NAMES:
            assert got[n].tobytes() == want[n].tobytes(), (n, b.as_tuple())
        for n in R.OUT_3D:
            m = R.cell_mask(b, n, **f)
            assert np.isfinite(got[n][m]).all() and np.isnan(got[n][~m]).all()
            if not R.empty(b, **f) and m.any():
                assert (got[n][m] != a[n][m]).any()


@pytest.mark.parametrize("nh", [0, 1])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_a_horizontally_uniform_state_is_balanced(pkg, dtype, nh):
    """Every horizontal difference is an exact zero: dpxy == 0 and mdx == 0 exactly, u becomes u + dts * ru_tend as bits."""
    b = _interior(pkg)
    a = R.make_state(b, dtype, 5, nh, poison=False)
    for n in ("p", "pb", "ph", "php", "alt", "al"):
        a[n][:] = a[n][:1, :, :1]
    for n in ("mu", "mudf"):
        a[n][:] = a[n][0, 0]
    before = {n: x.copy() for n, x in a.items()}
    R.advance_uv(a, b, nh, **SC)
    T = dtype
    for part, tend in (("u", "ru_tend"), ("v", "rv_tend")):
        m = R.cell_mask(b, part)
        want = before[part] + T(SC["dts"]) * before[tend]                     # x - 0 + 0 == x as bits for x != 0
        assert (want[m] != 0).all() and a[part][m].tobytes() == want[m].tobytes()


@pytest.mark.parametrize("nh", [0, 1])
def test_a_cyclic_shift_of_the_inputs_shifts_the_outputs(pkg, nh):
    """Interior tile, every array filled over the whole memory: rolling all of them by (1, 2) columns and rows and moving the
    tile along gives the rolled outputs."""
    b = _interior(pkg)
    a = R.make_state(b, F64, 8, nh, poison=False)
    moved = {n: (np.roll(x, (2, 1), axis=(0, -1)) if R.RANK[n] > 1 else x.copy()) for n, x in a.items()}
    b2 = b.replace(its=b.its + 1, ite=b.ite + 1, jts=b.jts + 2, jte=b.jte + 2)
    R.advance_uv(a, b, nh, **SC)
    R.advance_uv(moved, b2, nh, **SC)
    for n in R.OUT_3D:
        m = R.cell_mask(b, n)
        assert np.roll(a[n], (2, 1), axis=(0, -1))[R.cell_mask(b2, n)].tobytes() == moved[n][R.cell_mask(b2, n)].tobytes()
        assert m.sum() == R.cell_mask(b2, n).sum()


@pytest.mark.parametrize("nh", [0, 1])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_the_u_part_on_transposed_inputs_is_the_v_part(pkg, dtype, nh):
    """emdiv = 0 (the damping divides in one part and multiplies in the other), rdx == rdy: the u part on the transposed
    inputs, map factors swapped, equals the v part as bits."""
    n = 6
    b = pkg.synth.Bounds(ids=-9, ide=40, jds=-9, jde=40, kde=5, ims=0, ime=n + 1, jms=0, jme=n + 1, kms=1, kme=5,
                         its=1, ite=n, jts=1, jte=n, kts=1, kte=5)
    sc = dict(SC, emdiv=0.0, rdy=SC["rdx"])
    a = R.make_state(b, dtype, 9, nh, poison=False)
    tr = lambda x: np.ascontiguousarray(np.swapaxes(x, 0, -1)) if x.ndim > 1 else x.copy()
    swap = {"u": "v", "v": "u", "ru_tend": "rv_tend", "rv_tend": "ru_tend", "cqu": "cqv", "cqv": "cqu", "muu": "muv", "muv": "muu",
            "msfux": "msfvy", "msfvy": "msfux", "msfuy": "msfvx", "msfvx": "msfuy"}
    t = {swap.get(name, name): tr(x) for name, x in a.items()}
    R.advance_uv(a, b, nh, **sc)
    R.advance_uv(t, b, nh, **sc)
    m = R.cell_mask(b, "v")
    assert tr(t["u"])[m].tobytes() == a["v"][m].tobytes() and m.sum() == n * n * 4


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "p%ds%dn%d" % f)
@pytest.mark.parametrize("nh", [0, 1])
def test_nan_outside_the_read_mask_changes_no_output_bit(pkg, nh, flags):
    f = _flags(flags)
    for b in (_whole(pkg), _interior(pkg)):
        clean = R.advance_uv(R.make_state(b, F64, 4, nh, poison=False, **f), b, nh, **SC, **f)
        dirty = R.advance_uv(R.make_state(b, F64, 4, nh, poison=True, **f), b, nh, **SC, **f)
        for n in R.OUT_3D:
            m = R.cell_mask(b, n, **f)
            assert clean[n][m].tobytes() == dirty[n][m].tobytes() and np.isfinite(dirty[n][m]).all()
