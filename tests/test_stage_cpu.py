"""The Runge-Kutta stage bracket (include/amt_advance_mu_t.h section 15) without a GPU: tests/stage_ref.py against a plain
three-loop scalar transcription of small_step_prep and small_step_finish, the clauses the contract spells out (what stays
bit-unchanged, what is never read, mu = m - m), and every refusal of the library -- pointer level and handles --, which must
come back before any device call with the arrays untouched."""
import ctypes

import numpy as np
import pytest

import stage_ref as R
from conftest import bits_equal

DIMS = (7, 4, 5)                       # NI x NK x NJ mass cells
DTS = 1.7
F32, F64 = np.float32, np.float64


def _bounds(pkg, tile="whole"):
    b = pkg.synth.domain_bounds(*DIMS)
    b = b.replace(kms=0, kme=b.kte + 1)                           # a memory level below kts and one above kte
    if tile == "interior":
        b = b.replace(its=2, ite=5, jts=2, jte=4)
    elif tile == "east":
        b = b.replace(its=4, ite=b.ide, jts=2, jte=4)
    return b


def _nan_patterns(shape, dtype, tag):
    u = np.uint64 if np.dtype(dtype).itemsize == 8 else np.uint32
    quiet = u(0x7FF8000000000000) if np.dtype(dtype).itemsize == 8 else u(0x7FC00000)
    n = int(np.prod(shape))
    return (quiet | (np.arange(1, n + 1, dtype=u) + u(4096 * tag))).reshape(shape).view(dtype)


def _arrays(b, dtype, seed):
    """Every array of both calls plus h_diabatic, random and finite everywhere."""
    rng = np.random.default_rng(seed)
    s3, s2 = (b.jdim, b.kdim, b.idim), (b.jdim, b.idim)
    a = {n: rng.uniform(-2.0, 2.0, s3).astype(dtype) for n in R.PREP_3D + ("h_diabatic",)}
    a.update({n: rng.uniform(0.5, 1.5, s2).astype(dtype) for n in R.PREP_2D})
    return a


def _prep_loops(a, b, rk_step):
    """small_step_prep, three loops per statement, Fortran indices, scalar arithmetic in the arrays' type."""
    J, K, I = (lambda j: j - b.jms), (lambda k: k - b.kms), (lambda i: i - b.ims)
    ihi, jhi = min(b.ite, b.ide - 1), min(b.jte, b.jde - 1)
    m_before = a["mu"].copy()
    for j in range(b.jts, jhi + 1):
        for i in range(b.its, ihi + 1):
            m = m_before[J(j), I(i)]
            if rk_step == 1:
                a["mu_old"][J(j), I(i)] = m
                a["muts"][J(j), I(i)] = a["mub"][J(j), I(i)] + m
                a["mu_save"][J(j), I(i)] = m
                a["mu"][J(j), I(i)] = m - m
                a["mudf"][J(j), I(i)] = 0.0
            else:
                a["muts"][J(j), I(i)] = a["mub"][J(j), I(i)] + a["mu_old"][J(j), I(i)]
                a["mu_save"][J(j), I(i)] = m
                a["mu"][J(j), I(i)] = a["mu_old"][J(j), I(i)] - m
    for j in range(b.jts, jhi + 1):
        for k in range(b.kts, b.kte):
            for i in range(b.its, ihi + 1):
                at = (J(j), K(k), I(i))
                x = a["t"][at]
                if rk_step == 1:
                    a["t_old"][at] = x
                a["t_1"][at] = x
                left = a["muts"][J(j), I(i)] * a["t_old"][at]
                right = a["mut"][J(j), I(i)] * x
                a["t"][at] = left - right
    for j in range(b.jts, jhi + 1):
        for k in range(b.kts, b.kte + 1):
            for i in range(b.its, ihi + 1):
                a["ww_1"][J(j), K(k), I(i)] = a["ww"][J(j), K(k), I(i)]
    return a


def _finish_loops(a, b, n, dts, h):
    J, K, I = (lambda j: j - b.jms), (lambda k: k - b.kms), (lambda i: i - b.ims)
    ihi, jhi = min(b.ite, b.ide - 1), min(b.jte, b.jde - 1)
    T = a["t"].dtype.type
    for j in range(b.jts, jhi + 1):
        for k in range(b.kts, b.kte):
            for i in range(b.its, ihi + 1):
                at, at2 = (J(j), K(k), I(i)), (J(j), I(i))
                x = a["t"][at]
                if h is not None:
                    c = T(dts) * T(n)
                    cm = c * a["mut"][at2]
                    x = x - cm * h[at]
                back = a["t_1"][at] * a["mut"][at2]
                a["t"][at] = (x + back) / a["muts"][at2]
    for j in range(b.jts, jhi + 1):
        for k in range(b.kts, b.kte + 1):
            for i in range(b.its, ihi + 1):
                a["ww"][J(j), K(k), I(i)] = a["ww"][J(j), K(k), I(i)] + a["ww_1"][J(j), K(k), I(i)]
    for j in range(b.jts, jhi + 1):
        for i in range(b.its, ihi + 1):
            a["mu"][J(j), I(i)] = a["mu"][J(j), I(i)] + a["mu_save"][J(j), I(i)]
    return a


@pytest.mark.parametrize("with_h", [False, True], ids=["no-heating", "heating"])
@pytest.mark.parametrize("rk_step", [1, 2])
@pytest.mark.parametrize("tile", ["whole", "interior", "east"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_reference_equals_the_three_loop_transcription(pkg, dtype, tile, rk_step, with_h):
    b = _bounds(pkg, tile)
    got = _arrays(b, dtype, 10 * rk_step + with_h)
    want = {k: v.copy() for k, v in got.items()}
    with np.errstate(all="ignore"):
        R.prep(got, b, rk_step)
        _prep_loops(want, b, rk_step)
        for name in R.PREP:
            assert bits_equal(got[name], want[name]), ("prep", name)
        rng = np.random.default_rng(5)                            # the sweeps in between: new t, ww, mu, muts
        for name in ("t", "ww", "mu"):
            got[name] = rng.uniform(-2.0, 2.0, got[name].shape).astype(dtype)
            want[name] = got[name].copy()
        h = got["h_diabatic"] if with_h else None
        R.finish(got, b, 3, DTS, h)
        _finish_loops(want, b, 3, DTS, h)
    for name in R.FINISH:
        assert bits_equal(got[name], want[name]), ("finish", name)
    assert np.isfinite(got["t"]).all()


@pytest.mark.parametrize("rk_step", [1, 2, 3])
@pytest.mark.parametrize("tile", ["whole", "interior", "east"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_what_is_not_read_may_be_nan_and_what_is_not_written_keeps_its_bits(pkg, dtype, tile, rk_step):
    """NaN with a payload of its own in every cell the contract does not read -- and, at rk_step 1, in the whole of the arrays
    whose old contents are not read.  Inside the ranges everything comes out finite; outside every bit is kept: column ide and
    row jde of a tile that reaches them, level kte of t, t_1 and t_old, the memory levels outside kts..kte, every input."""
    b = _bounds(pkg, tile)
    a = _arrays(b, dtype, 20 + rk_step)
    cells = {"t": R.cell_mask(b, "t"), "ww": R.cell_mask(b, "ww"), "col": R.column_mask(b)}
    read = {"t": cells["t"], "ww": cells["ww"], "mu": cells["col"], "mut": cells["col"], "mub": cells["col"]}
    if rk_step > 1:
        read.update(t_old=cells["t"], mu_old=cells["col"])
    for k, name in enumerate(R.PREP):
        poison = _nan_patterns(a[name].shape, dtype, k)
        keep = read.get(name, np.zeros(a[name].shape, bool))
        a[name][~keep] = poison[~keep]
    before = {k: v.copy() for k, v in a.items()}
    with np.errstate(invalid="raise"):
        R.prep(a, b, rk_step)
    written = {"t": cells["t"], "t_1": cells["t"], "ww_1": cells["ww"], "mu": cells["col"], "mu_save": cells["col"], "muts": cells["col"]}
    if rk_step == 1:
        written.update(t_old=cells["t"], mu_old=cells["col"], mudf=cells["col"])
    assert set(written) == set(R.prep_outputs(rk_step))
    for name in R.PREP:
        w = written.get(name, np.zeros(a[name].shape, bool))
        assert bits_equal(a[name][~w], before[name][~w]), name
        assert np.isfinite(a[name][w]).all(), name
    assert not cells["t"][:, b.kte - b.kms, :].any() and cells["ww"][:, b.kte - b.kms, :].any()
    if tile != "interior":
        assert not cells["col"][:, b.ide - b.ims].any()
    # finish on the same state: h_diabatic poisoned outside the t cells
    h = a["h_diabatic"]
    h[~cells["t"]] = _nan_patterns(h.shape, dtype, 20)[~cells["t"]]
    before = {k: v.copy() for k, v in a.items()}
    with np.errstate(invalid="raise"):
        R.finish(a, b, 2, DTS, h)
    written = {"t": cells["t"], "ww": cells["ww"], "mu": cells["col"]}
    for name in R.FINISH + ("h_diabatic",):
        w = written.get(name, np.zeros(a[name].shape, bool))
        assert bits_equal(a[name][~w], before[name][~w]), name
        assert np.isfinite(a[name][w]).all(), name


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_mu_is_m_minus_m_at_the_first_step(pkg, dtype):
    """Computed, not a stored zero: -0.0 gives +0.0, a NaN or an infinity gives a NaN; the copies keep every bit, a signalling
    NaN's included."""
    b = _bounds(pkg)
    a = _arrays(b, dtype, 31)
    col = R.column_mask(b)
    js, is_ = np.nonzero(col)
    snan = np.array([0x7FF0000000000123 if dtype is F64 else 0x7F800123], np.uint64 if dtype is F64 else np.uint32).view(dtype)[0]
    specials = [dtype(-0.0), dtype(np.nan), dtype(np.inf), dtype(-np.inf), snan, dtype(0.0), dtype(3.5)]
    for (j, i), v in zip(zip(js, is_), specials):
        a["mu"][j, i] = v
    m = a["mu"].copy()
    with np.errstate(all="ignore"):
        R.prep(a, b, 1)
    got = [a["mu"][j, i] for j, i in zip(js, is_)][:len(specials)]
    assert R.as_bits(np.array(got[0]))[()] == 0                    # -0.0 - -0.0 = +0.0
    assert all(np.isnan(g) for g in got[1:5])
    assert R.as_bits(np.array(got[5]))[()] == 0 and R.as_bits(np.array(got[6]))[()] == 0
    assert bits_equal(a["mu_save"][col], m[col]) and bits_equal(a["mu_old"][col], m[col])
    assert (R.as_bits(a["mudf"])[col] == 0).all()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_members_are_independent(pkg, dtype):
    b = _bounds(pkg, "east")
    singles = [_arrays(b, dtype, 40 + m) for m in range(3)]
    stacked = {k: np.stack([s[k] for s in singles]) for k in singles[0]}
    with np.errstate(all="ignore"):
        R.prep(stacked, b, 2)
        R.finish(stacked, b, 4, DTS, stacked["h_diabatic"])
        for s in singles:
            R.prep(s, b, 2)
            R.finish(s, b, 4, DTS, s["h_diabatic"])
    for m, s in enumerate(singles):
        for name in R.PREP:
            assert bits_equal(stacked[name][m], s[name]), (name, m)


# ---------------------------------------------------------------------------------------------
# the library's refusals: before any device call, with or without a device, nothing written
# ---------------------------------------------------------------------------------------------
OK, PRECONDITION, INVALID = 0, 2, 3


def _prep_call(pkg, dtype, arrays, b, *, rk_step=1, members=1, null=()):
    L = pkg.load_library()
    fn = L.amt_stage_prep_device_f64 if np.dtype(dtype).itemsize == 8 else L.amt_stage_prep_device_f32
    ptrs = [None if name in null else ctypes.c_void_p(arrays[name].ctypes.data) for name in R.PREP]
    return fn(None, members, *ptrs, rk_step, *b.as_tuple())


def _finish_call(pkg, dtype, arrays, b, *, n=2, members=1, null=(), h=True):
    L = pkg.load_library()
    fn = L.amt_stage_finish_device_f64 if np.dtype(dtype).itemsize == 8 else L.amt_stage_finish_device_f32
    ptrs = [None if name in null else ctypes.c_void_p(arrays[name].ctypes.data) for name in R.FINISH]
    return fn(None, members, *ptrs, DTS, n, ctypes.c_void_p(arrays["h_diabatic"].ctypes.data) if h else None, *b.as_tuple())


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_every_refusal_comes_back_with_its_status_and_writes_nothing(pkg, dtype):
    L = pkg.load_library()
    b = _bounds(pkg)
    arrays = _arrays(b, dtype, 8)
    before = {k: v.copy() for k, v in arrays.items()}
    bad_bounds = [("its < ims", b.replace(its=b.ims - 1)), ("ite > ime", b.replace(ite=b.ime + 1)), ("jts < jms", b.replace(jts=b.jms - 1)),
                  ("jte > jme", b.replace(jte=b.jme + 1)), ("kts != 1", b.replace(kts=2)), ("kte != kde", b.replace(kte=b.kde - 1)),
                  ("kme < kte", b.replace(kme=b.kte - 1))]
    for rk in (1, 2):
        for name in R.PREP:
            if name == "mudf" and rk > 1:                         # not touched and may be NULL: not refused for that
                if L.amt_device_count() == 0:
                    assert _prep_call(pkg, dtype, arrays, b, rk_step=rk, null=(name,)) in (1, 4), L.amt_last_error()
                continue
            assert _prep_call(pkg, dtype, arrays, b, rk_step=rk, null=(name,)) == INVALID and L.amt_last_error(), (name, rk)
    for name in R.FINISH:
        assert _finish_call(pkg, dtype, arrays, b, null=(name,)) == INVALID, name
    for what, kw in [("members 0", dict(members=0)), ("members -1", dict(members=-1)), ("rk_step 0", dict(rk_step=0)), ("rk_step -3", dict(rk_step=-3))]:
        assert _prep_call(pkg, dtype, arrays, b, **kw) == INVALID, (what, L.amt_last_error())
    for what, kw in [("members 0", dict(members=0)), ("n 0", dict(n=0)), ("n -2", dict(n=-2))]:
        assert _finish_call(pkg, dtype, arrays, b, **kw) == INVALID, (what, L.amt_last_error())
    for what, bounds in bad_bounds:
        assert _prep_call(pkg, dtype, arrays, bounds) == PRECONDITION, (what, L.amt_last_error())
        assert _finish_call(pkg, dtype, arrays, bounds) == PRECONDITION, (what, L.amt_last_error())
        assert L.amt_last_error(), what
    # an output that overlaps another array of the call: the same array, a shifted one, a 2-D array inside a 3-D one
    flat = arrays["t"].reshape(-1)
    inside2d = flat[5:5 + arrays["mut"].size].reshape(arrays["mut"].shape)
    prep_overlaps = [("t_1 is t", dict(t_1=arrays["t"])), ("ww one element into t", dict(ww=flat[1:])), ("mut inside t", dict(mut=inside2d)),
                     ("mu_save is mu", dict(mu_save=arrays["mu"])), ("mub is muts", dict(mub=arrays["muts"])),
                     ("mudf is the end of ww_1", dict(mudf=arrays["ww_1"].reshape(-1)[-3:])), ("t_old is ww", dict(t_old=arrays["ww"])),
                     ("mu_old is mub", dict(mu_old=arrays["mub"]))]
    for what, swap in prep_overlaps:
        assert _prep_call(pkg, dtype, dict(arrays, **swap), b) == INVALID, (what, L.amt_last_error())
    assert _prep_call(pkg, dtype, dict(arrays, t_old=arrays["t"]), b, rk_step=2) == INVALID       # t is an output at every step
    finish_overlaps = [("t_1 is t", dict(t_1=arrays["t"])), ("ww_1 is ww", dict(ww_1=arrays["ww"])), ("mu_save is mu", dict(mu_save=arrays["mu"])),
                       ("h_diabatic one element into t", dict(h_diabatic=flat[1:])), ("muts inside ww", dict(muts=arrays["ww"].reshape(-1)[3:3 + arrays["mut"].size]))]
    for what, swap in finish_overlaps:
        assert _finish_call(pkg, dtype, dict(arrays, **swap), b) == INVALID, (what, L.amt_last_error())
    # inputs may alias one another: not refused for that (without a device the call then stops at the missing device)
    if L.amt_device_count() == 0:
        assert _prep_call(pkg, dtype, dict(arrays, mub=arrays["mut"]), b) in (1, 4), L.amt_last_error()
        assert _prep_call(pkg, dtype, dict(arrays, t_old=arrays["ww"], mu_old=arrays["mub"]), b, rk_step=2) in (1, 4), L.amt_last_error()
        assert _finish_call(pkg, dtype, dict(arrays, ww_1=arrays["t_1"], h_diabatic=arrays["t_1"], mu_save=arrays["mut"], muts=arrays["mut"]), b) in (1, 4)
        assert _finish_call(pkg, dtype, arrays, b, h=False) in (1, 4), L.amt_last_error()
    for k, v in arrays.items():
        assert bits_equal(v, before[k]), k


def test_more_members_than_one_launch_carries_is_a_precondition(pkg):
    """65536 members of a one-cell patch: the arrays are real (the overlap check sees their full extent) and untouched."""
    L = pkg.load_library()
    b = pkg.synth.Bounds(ids=1, ide=2, jds=1, jde=2, kde=1, ims=1, ime=1, jms=1, jme=1, kms=1, kme=1, its=1, ite=1, jts=1, jte=1, kts=1, kte=1)
    members = 65536
    arrays = {n: np.full((members, 1, 1, 1) if n in R.PREP_3D + ("h_diabatic",) else (members, 1, 1), 1.5, F32) for n in R.PREP + ("h_diabatic",)}
    assert _prep_call(pkg, F32, arrays, b, members=members) == PRECONDITION, L.amt_last_error()
    assert b"65535" in L.amt_last_error()
    assert _finish_call(pkg, F32, arrays, b, members=members) == PRECONDITION, L.amt_last_error()
    assert all((a == F32(1.5)).all() for a in arrays.values())


# a handle that is not NULL, for the checks in front of the first use of the device: zeroed memory larger than either struct
# (the setting is off in it, its bounds are all zero)
_blank = (ctypes.c_char * 8192)()
BLANK = ctypes.cast(_blank, ctypes.c_void_p)
_room = (ctypes.c_double * 64)()
ROOM = [ctypes.c_void_p(ctypes.addressof(_room) + 64 * k) for k in range(4)]


@pytest.mark.parametrize("prefix,who", [("amt_domain", "null domain"), ("amt_ensemble", "null ensemble")])
def test_the_handle_calls_refuse_in_front_of_the_first_device_call(pkg, prefix, who):
    L = pkg.load_library()
    fn = lambda name: getattr(L, f"{prefix}_{name}")
    assert fn("set_stage")(None, 1, None, None, None, None) == INVALID and L.amt_last_error().decode() == who
    assert fn("stage_prep")(None, 1) == INVALID and L.amt_last_error().decode() == who
    assert fn("stage_finish")(None, 1, None) == INVALID and L.amt_last_error().decode() == who
    assert fn("stage_ptr")(None, 0) is None
    # the setting is off: prep and finish are preconditions, the pointers are NULL, whatever the other arguments
    for k in (-1, 0, 1, 2, 3, 4):
        assert fn("stage_ptr")(BLANK, k) is None
    assert fn("stage_prep")(BLANK, 1) == PRECONDITION and b"off" in L.amt_last_error()
    assert fn("stage_prep")(BLANK, 0) == PRECONDITION
    assert fn("stage_finish")(BLANK, 3, None) == PRECONDITION and b"off" in L.amt_last_error()
    assert fn("stage_finish")(BLANK, 0, ROOM[0]) == PRECONDITION
    # a mix of given and missing arrays; then the checks of the pointer-level call; the handle's (all-zero) bounds
    for mix in ([ROOM[0], None, None, None], [None, ROOM[1], ROOM[2], ROOM[3]], [ROOM[0], ROOM[1], None, ROOM[3]]):
        assert fn("set_stage")(BLANK, 1, *mix) == INVALID and b"all four" in L.amt_last_error(), mix
    assert fn("set_stage")(BLANK, 1, ROOM[0], ROOM[1], ROOM[2], ROOM[3]) == INVALID          # the blank handle's fields are NULL
    assert fn("set_stage")(BLANK, 1, None, None, None, None) == PRECONDITION and b"does not admit" in L.amt_last_error()
    for k in range(4):
        assert fn("stage_ptr")(BLANK, k) is None                  # a refusal changes nothing
    assert bytes(_blank) == bytes(8192)
