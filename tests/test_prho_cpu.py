"""The pressure diagnosis calc_p_rho (include/amt_advance_mu_t.h section 16) without a GPU: tests/prho_ref.py against a plain
three-loop scalar transcription, the clauses the contract spells out (what stays bit-unchanged, what is never read), the
identities that tie the contract to the physics, and every refusal of the library -- pointer level and handles --, which must
come back before any device call with the arrays untouched."""
import ctypes

import numpy as np
import pytest

import prho_ref as R
from conftest import bits_equal

DIMS = (7, 4, 5)                       # NI x NK x NJ mass cells
T0, SMDIV = 300.0, 0.1
F32, F64 = np.float32, np.float64


def _bounds(pkg, tile="whole"):
    b = pkg.synth.domain_bounds(*DIMS)
    b = b.replace(kms=-2, kme=b.kte + 1)                          # three memory levels below kts and one above kte
    if tile == "interior":
        b = b.replace(its=2, ite=5, jts=2, jte=4)
    elif tile == "edges":                                         # reaches ide and jde: column ide and row jde stay out
        b = b.replace(its=4, ite=b.ide, jts=3, jte=b.jde)
    return b


def _nan_patterns(shape, dtype, tag):
    u = np.uint64 if np.dtype(dtype).itemsize == 8 else np.uint32
    quiet = u(0x7FF8000000000000) if np.dtype(dtype).itemsize == 8 else u(0x7FC00000)
    n = int(np.prod(shape))
    return (quiet | (np.arange(1, n + 1, dtype=u) + u(4096 * tag))).reshape(shape).view(dtype)


def _arrays(b, dtype, seed, members=1):
    """Every array of the call, random and finite everywhere, of the magnitudes of a dry atmosphere in these units: theta
    perturbations of a few K on t0 = 300, alt near 1, column masses of order 1, c2a of order 10, dnw < 0 with rdnw = 1 / dnw."""
    rng = np.random.default_rng(seed)
    a = {}
    for name in R.NAMES:
        s = R.shape(b, name, members)
        lo, hi = {"alt": (0.7, 1.3), "c2a": (5.0, 15.0), "t": (-3.0, 3.0), "t_old": (-5.0, 5.0), "mu": (-0.2, 0.2),
                  "muts": (0.8, 1.2), "znu": (0.05, 0.95), "dnw": (-0.3, -0.1), "ph": (-50.0, 50.0)}.get(name, (-2.0, 2.0))
        a[name] = rng.uniform(lo, hi, s).astype(dtype)
    a["rdnw"] = (dtype(1) / a["dnw"]).astype(dtype)
    return a


def _loops(a, b, mode, step, t0, smdiv):
    """calc_p_rho, three loops, Fortran indices, scalar arithmetic in the arrays' type."""
    J, K, I = (lambda j: j - b.jms), (lambda k: k - b.kms), (lambda i: i - b.ims)
    ihi, jhi = min(b.ite, b.ide - 1), min(b.jte, b.jde - 1)
    T = a["t"].dtype.type
    t0, smdiv = T(t0), T(smdiv)
    for j in range(b.jts, jhi + 1):
        for k in range(b.kts, b.kte):
            for i in range(b.its, ihi + 1):
                at, up, c = (J(j), K(k), I(i)), (J(j), K(k + 1), I(i)), (J(j), I(i))
                mu, muts, alt, told = a["mu"][c], a["muts"][c], a["alt"][at], a["t_old"][at]
                q = (alt * (a["t"][at] - (mu * told))) / (muts * (t0 + told))
                if mode == 1:
                    al = (T(-1) / muts) * ((alt * mu) + (a["rdnw"][K(k)] * (a["ph"][up] - a["ph"][at])))
                    x = a["c2a"][at] * (q - al)
                else:
                    x = mu * a["znu"][K(k)]
                    al = q - (x / a["c2a"][at])
                    a["ph"][up] = a["ph"][at] - (a["dnw"][K(k)] * ((muts * al) + (mu * alt)))
                a["al"][at] = al
                a["p"][at] = x if step == 0 else x + (smdiv * (x - a["pm1"][at]))
                a["pm1"][at] = x
    return a


@pytest.mark.parametrize("step", [0, 2])
@pytest.mark.parametrize("mode", [1, 2], ids=["nonhydrostatic", "hydrostatic"])
@pytest.mark.parametrize("tile", ["whole", "interior", "edges"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_reference_equals_the_three_loop_transcription(pkg, dtype, tile, mode, step):
    b = _bounds(pkg, tile)
    assert b.kms == -2
    got = _arrays(b, dtype, 10 * mode + step)
    want = {k: v.copy() for k, v in got.items()}
    with np.errstate(all="ignore"):
        R.p_rho(got, b, mode, step, T0, SMDIV)
        _loops(want, b, mode, step, T0, SMDIV)
    for name in R.NAMES:
        assert bits_equal(got[name], want[name]), name
        assert np.isfinite(got[name]).all(), name
    assert not bits_equal(got["p"], got["pm1"]) or step == 0


@pytest.mark.parametrize("step", [0, 1])
@pytest.mark.parametrize("mode", [1, 2], ids=["nonhydrostatic", "hydrostatic"])
@pytest.mark.parametrize("tile", ["whole", "interior", "edges"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_what_is_not_read_may_be_nan_and_what_is_not_written_keeps_its_bits(pkg, dtype, tile, mode, step):
    """NaN with a payload of its own in every cell the contract does not read -- the whole of al and p, the old pm1 at step 0,
    ph above kts in mode 2, the level arrays the mode does not use.  Inside the ranges everything comes out finite; outside
    every bit is kept: column ide and row jde of a tile that reaches them, level kte of al, p, pm1, the memory levels outside
    kts..kte, ph(kts), every input."""
    b = _bounds(pkg, tile)
    a = _arrays(b, dtype, 20 + mode)
    for k, name in enumerate(R.NAMES):
        keep = R.read_mask(b, name, mode, step)
        keep = np.zeros(a[name].shape, bool) if keep is None else keep
        a[name][~keep] = _nan_patterns(a[name].shape, dtype, k)[~keep]
    before = {k: v.copy() for k, v in a.items()}
    with np.errstate(invalid="raise"):
        R.p_rho(a, b, mode, step, T0, SMDIV)
    for name in R.NAMES:
        w = R.written_mask(b, name, mode)
        w = np.zeros(a[name].shape, bool) if w is None else w
        assert bits_equal(a[name][~w], before[name][~w]), name
        assert np.isfinite(a[name][w]).all(), name
    cells = R.cell_mask(b, "t")
    assert not cells[:, b.kte - b.kms, :].any() and not cells[:, :b.kts - b.kms, :].any()
    if tile != "interior":
        assert not R.column_mask(b)[:, b.ide - b.ims].any()
    if tile == "edges":
        assert not R.column_mask(b)[b.jde - b.jms, :].any()
    written_ph = R.written_mask(b, "ph", mode)
    assert (written_ph is None) == (mode == 1)
    if mode == 2:
        assert not written_ph[:, b.kts - b.kms, :].any() and written_ph[:, b.kte - b.kms, :].any()


@pytest.mark.parametrize("mode", [1, 2], ids=["nonhydrostatic", "hydrostatic"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_without_damping_p_is_the_diagnosed_pressure(pkg, dtype, mode):
    """smdiv = 0 at step != 0: p = x + (0 * (x - pm1)) = x for finite operands, and pm1 == p; at step 0 the same two arrays
    whatever smdiv is.  al (and in mode 2 ph) never depend on the damping."""
    b = _bounds(pkg)
    start = _arrays(b, dtype, 33)
    runs = {}
    for key, (step, smdiv) in dict(undamped=(3, 0.0), first=(0, SMDIV), damped=(3, SMDIV)).items():
        runs[key] = R.p_rho({k: v.copy() for k, v in start.items()}, b, mode, step, T0, smdiv)
    cells = R.cell_mask(b, "t")
    for key in ("undamped", "first"):
        assert bits_equal(runs[key]["p"][cells], runs[key]["pm1"][cells]), key
    for name in ("p", "pm1", "al", "ph"):
        assert bits_equal(runs["undamped"][name], runs["first"][name]), name
    assert bits_equal(runs["damped"]["pm1"], runs["first"]["pm1"]) and bits_equal(runs["damped"]["al"], runs["first"]["al"])
    assert bits_equal(runs["damped"]["ph"], runs["first"]["ph"])
    assert (runs["damped"]["p"][cells] != runs["first"]["p"][cells]).any()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_the_hydrostatic_column_integrates_the_density(pkg, dtype):
    """Mode 2, recomputed level by level from the OUTPUT al: ph(k+1) is exactly ph(k) - (dnw(k) * ((muts * al) + (mu * alt))),
    so the difference ph(k+1) - ph(k), one more rounding, is -(that product) to within u * (|ph(k+1)| + |difference|) with u the
    unit roundoff; ph(kts) is what it was."""
    b = _bounds(pkg, "edges")
    a = _arrays(b, dtype, 41)
    ph_before = a["ph"].copy()
    R.p_rho(a, b, 2, 1, T0, SMDIV)
    u = np.finfo(dtype).eps / 2
    sj, si = R.columns(b)
    mu, muts = a["mu"][sj, si], a["muts"][sj, si]
    assert bits_equal(a["ph"][:, b.kts - b.kms, :], ph_before[:, b.kts - b.kms, :])
    for k in range(b.kts, b.kte):
        kk = k - b.kms
        d = a["dnw"][kk] * ((muts * a["al"][sj, kk, si]) + (mu * a["alt"][sj, kk, si]))
        lo, hi = a["ph"][sj, kk, si], a["ph"][sj, kk + 1, si]
        assert bits_equal(hi, lo - d), k
        diff = hi - lo
        assert (np.abs(diff + d) <= 2 * u * (np.abs(hi) + np.abs(diff))).all(), k
        assert (diff != 0).all()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_mode_1_on_the_geopotential_of_mode_2_returns_its_density(pkg, dtype):
    """With rdnw = fl(1 / dnw) a non-hydrostatic call on the ph a hydrostatic call produced diagnoses that call's al again, to
    within rounding.  The bound, with u the unit roundoff, A = muts * al, B = mu * alt (B has the same bits in both calls):
    mode 2 stores ph(k+1) = fl(ph(k) - d), d = fl(dnw * fl(fl(A) + B)): an absolute error of at most u |ph(k+1)|.  Mode 1 forms
    D = fl(ph(k+1) - ph(k)) (u |D|), fl(rdnw * D) with rdnw itself rounded (2 u |A + B|), adds B (u |A|) and multiplies by
    fl(-1 / muts) (2 u |al|).  The roundings that act on A + B are those of the sum, of dnw *, of rdnw, of rdnw * and of D: five;
    those that act on A alone are A's own and the last sum's: two.  Hence
        |al1 - al2| <= u * (5 (|A| + |B|) + 2 |A| + 2 |rdnw| (|ph(k)| + |ph(k+1)|)) / |muts| + 2 u |al2|,
    doubled below for the second-order terms."""
    b = _bounds(pkg)
    a = _arrays(b, dtype, 52)
    R.p_rho(a, b, 2, 0, T0, SMDIV)
    al2 = a["al"].copy()
    R.p_rho(a, b, 1, 0, T0, SMDIV)
    u = np.finfo(dtype).eps / 2
    sj, si = R.columns(b)
    mu, muts = np.abs(a["mu"][sj, si]).astype(F64), np.abs(a["muts"][sj, si]).astype(F64)
    worst = 0.0
    for k in range(b.kts, b.kte):
        kk = k - b.kms
        A = muts * np.abs(al2[sj, kk, si]).astype(F64)
        B = mu * np.abs(a["alt"][sj, kk, si]).astype(F64)
        ph = np.abs(a["ph"][sj, kk, si]).astype(F64) + np.abs(a["ph"][sj, kk + 1, si]).astype(F64)
        bound = 2 * (u * (5 * (A + B) + 2 * A + 2 * abs(float(a["rdnw"][kk])) * ph) / muts + 2 * u * np.abs(al2[sj, kk, si]).astype(F64))
        err = np.abs(a["al"][sj, kk, si].astype(F64) - al2[sj, kk, si].astype(F64))
        assert (err <= bound).all(), (k, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    assert 0 < worst                                               # rounding shows: the two calls are not the same arithmetic


@pytest.mark.parametrize("mode", [1, 2], ids=["nonhydrostatic", "hydrostatic"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_members_are_independent_and_share_the_level_arrays(pkg, dtype, mode):
    b = _bounds(pkg, "edges")
    singles = [_arrays(b, dtype, 60 + m) for m in range(3)]
    for s in singles[1:]:
        for name in R.IN_1D:
            s[name] = singles[0][name].copy()
    stacked = {k: (singles[0][k].copy() if k in R.IN_1D else np.stack([s[k] for s in singles])) for k in R.NAMES}
    R.p_rho(stacked, b, mode, 1, T0, SMDIV)
    for m, s in enumerate(singles):
        R.p_rho(s, b, mode, 1, T0, SMDIV)
        for name in R.NAMES:
            assert bits_equal(stacked[name] if name in R.IN_1D else stacked[name][m], s[name]), (name, m)


# ---------------------------------------------------------------------------------------------
# the library's refusals: before any device call, with or without a device, nothing written
# ---------------------------------------------------------------------------------------------
OK, PRECONDITION, INVALID = 0, 2, 3


def _call(pkg, dtype, arrays, b, *, mode=1, step=0, members=1, null=()):
    L = pkg.load_library()
    fn = L.amt_p_rho_device_f64 if np.dtype(dtype).itemsize == 8 else L.amt_p_rho_device_f32
    ptrs = [None if name in null else ctypes.c_void_p(arrays[name].ctypes.data) for name in R.NAMES]
    return fn(None, members, mode, step, *ptrs, T0, SMDIV, *b.as_tuple())


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_every_refusal_comes_back_with_its_status_and_writes_nothing(pkg, dtype):
    L = pkg.load_library()
    b = _bounds(pkg)
    arrays = _arrays(b, dtype, 8)
    before = {k: v.copy() for k, v in arrays.items()}
    for mode in (1, 2):
        for name in R.NAMES:
            assert _call(pkg, dtype, arrays, b, mode=mode, null=(name,)) == INVALID and L.amt_last_error(), (name, mode)
    for what, kw in [("members 0", dict(members=0)), ("members -1", dict(members=-1)), ("mode 0", dict(mode=0)), ("mode 3", dict(mode=3)),
                     ("mode -1", dict(mode=-1)), ("step -1", dict(step=-1))]:
        assert _call(pkg, dtype, arrays, b, **kw) == INVALID, (what, L.amt_last_error())
    bad_bounds = [("its < ims", b.replace(its=b.ims - 1)), ("ite > ime", b.replace(ite=b.ime + 1)), ("jts < jms", b.replace(jts=b.jms - 1)),
                  ("jte > jme", b.replace(jte=b.jme + 1)), ("kts != 1", b.replace(kts=2)), ("kte != kde", b.replace(kte=b.kde - 1)),
                  ("kme < kte", b.replace(kme=b.kte - 1))]
    for what, bounds in bad_bounds:
        for mode in (1, 2):
            assert _call(pkg, dtype, arrays, bounds, mode=mode) == PRECONDITION, (what, L.amt_last_error())
            assert L.amt_last_error(), what
    # an output that overlaps another array of the call: the same array, a shifted one, a 2-D or 1-D array inside a 3-D one
    flat = arrays["al"].reshape(-1)
    overlaps = [("p is al", dict(p=arrays["al"])), ("pm1 one element into al", dict(pm1=flat[1:])), ("alt is p", dict(alt=arrays["p"])),
                ("t is pm1", dict(t=arrays["pm1"])), ("mu inside al", dict(mu=flat[5:5 + arrays["mu"].size].reshape(arrays["mu"].shape))),
                ("dnw is the end of p", dict(dnw=arrays["p"].reshape(-1)[-arrays["dnw"].size:])), ("t_old is al", dict(t_old=arrays["al"]))]
    for what, swap in overlaps:
        for mode in (1, 2):
            assert _call(pkg, dtype, dict(arrays, **swap), b, mode=mode) == INVALID, (what, mode, L.amt_last_error())
    # ph is an output in mode 2 only
    assert _call(pkg, dtype, dict(arrays, alt=arrays["ph"]), b, mode=2) == INVALID
    assert _call(pkg, dtype, dict(arrays, ph=arrays["al"]), b, mode=1) == INVALID                  # al is an output in both
    # inputs may alias one another: not refused for that (without a device the call then stops at the missing device)
    if L.amt_device_count() == 0:
        assert _call(pkg, dtype, dict(arrays, alt=arrays["ph"], c2a=arrays["ph"]), b, mode=1) in (1, 4), L.amt_last_error()
        assert _call(pkg, dtype, dict(arrays, c2a=arrays["alt"], t_old=arrays["t"], muts=arrays["mu"], znu=arrays["rdnw"]), b, mode=2) in (1, 4)
    for k, v in arrays.items():
        assert bits_equal(v, before[k]), k


def test_more_members_than_one_launch_carries_is_a_precondition(pkg):
    """65536 members of a one-cell patch: the arrays are real (the overlap check sees their full extent) and untouched."""
    L = pkg.load_library()
    b = pkg.synth.Bounds(ids=1, ide=2, jds=1, jde=2, kde=2, ims=1, ime=1, jms=1, jme=1, kms=1, kme=2, its=1, ite=1, jts=1, jte=1, kts=1, kte=2)
    members = 65536
    arrays = {n: np.full(R.shape(b, n, members), 1.5, F32) for n in R.NAMES}
    for mode in (1, 2):
        assert _call(pkg, F32, arrays, b, mode=mode, members=members) == PRECONDITION, L.amt_last_error()
        assert b"65535" in L.amt_last_error()
    assert all((a == F32(1.5)).all() for a in arrays.values())


# a handle that is not NULL, for the checks in front of the first use of the device: zeroed memory larger than either struct
# (the settings are off in it, its bounds are all zero)
_blank = (ctypes.c_char * 8192)()
BLANK = ctypes.cast(_blank, ctypes.c_void_p)
_room = (ctypes.c_double * 128)()
ROOM = [ctypes.c_void_p(ctypes.addressof(_room) + 64 * k) for k in range(8)]


@pytest.mark.parametrize("prefix,who", [("amt_domain", "null domain"), ("amt_ensemble", "null ensemble")])
def test_the_handle_calls_refuse_in_front_of_the_first_device_call(pkg, prefix, who):
    L = pkg.load_library()
    fn = lambda name: getattr(L, f"{prefix}_{name}")
    none8 = [None] * 8
    assert fn("set_p_rho")(None, 1, 0, T0, SMDIV, *none8) == INVALID and L.amt_last_error().decode() == who
    assert fn("p_rho")(None, 0) == INVALID and L.amt_last_error().decode() == who
    assert fn("p_rho_ptr")(None, 0) is None
    # the setting is off: the diagnosis is a precondition, the pointers are NULL, whatever the other arguments
    for k in (-1, 0, 3, 7, 8):
        assert fn("p_rho_ptr")(BLANK, k) is None
    assert fn("p_rho")(BLANK, 0) == PRECONDITION and b"off" in L.amt_last_error()
    assert fn("p_rho")(BLANK, -1) == PRECONDITION
    # a mode that is none; a mix of given and missing arrays; the stage bracket, whose t_old the diagnosis reads, is off
    for mode in (-1, 3):
        assert fn("set_p_rho")(BLANK, mode, 1, T0, SMDIV, *none8) == INVALID and b"mode" in L.amt_last_error(), mode
    for mix in ([ROOM[0]] + [None] * 7, [None] + ROOM[1:], ROOM[:5] + [None] + ROOM[6:]):
        assert fn("set_p_rho")(BLANK, 1, 1, T0, SMDIV, *mix) == INVALID and b"all eight" in L.amt_last_error(), mix
    for mode in (1, 2):
        assert fn("set_p_rho")(BLANK, mode, 1, T0, SMDIV, *none8) == PRECONDITION and b"stage" in L.amt_last_error()
        assert fn("set_p_rho")(BLANK, mode, 0, T0, SMDIV, *ROOM) == PRECONDITION and b"stage" in L.amt_last_error()
    for k in range(8):
        assert fn("p_rho_ptr")(BLANK, k) is None                  # a refusal changes nothing
    assert bytes(_blank) == bytes(8192)
