"""The flux-average contract (include/amt_advance_mu_t.h section 14) without a GPU: tests/sumflux_ref.py against a plain
transcription of what WRF's sumflux does (zero the tile, add, average on the last sub-step), the properties the contract spells
out, and every refusal of the library, which must come back before any device call with the accumulators untouched."""
import ctypes

import numpy as np
import pytest

import sumflux_ref as R
from conftest import bits_equal

DIMS = (7, 4, 5)                       # NI x NK x NJ mass cells


def _bounds(pkg, tile="whole"):
    b = pkg.synth.domain_bounds(*DIMS)
    b = b.replace(kms=0, kme=b.kte + 1)                           # a memory level below kts and one above kte
    if tile == "interior":
        b = b.replace(its=2, ite=5, jts=2, jte=4)
    elif tile == "east":
        b = b.replace(its=4, ite=b.ide, jts=2, jte=4)
    return b


def _inputs(b, dtype, seed, members=1):
    rng = np.random.default_rng(seed)
    lead = (members,) if members > 1 else ()
    s3, s2 = lead + (b.jdim, b.kdim, b.idim), lead + (b.jdim, b.idim)
    inp = {n: rng.uniform(-2.0, 2.0, s3).astype(dtype) for n in R.INPUTS_3D}
    inp.update({n: rng.uniform(0.5, 1.5, s2).astype(dtype) for n in R.INPUTS[6:]})
    return inp


def _poison(b, dtype, members=1):
    lead = (members,) if members > 1 else ()
    shape = lead + (b.jdim, b.kdim, b.idim)
    u = np.uint64 if np.dtype(dtype).itemsize == 8 else np.uint32
    quiet = u(0x7FF8000000000000) if np.dtype(dtype).itemsize == 8 else u(0x7FC00000)
    return {n: (quiet | (np.arange(1, int(np.prod(shape)) + 1, dtype=u) + u(1000 * k))).reshape(shape).view(dtype)
            for k, n in enumerate(R.ACCUMULATORS)}


def _transcription(acc, inp, b, iteration, n):
    """Three loops per statement, Fortran indices, in the order of WRF's routine: the tile is zeroed at the first sub-step,
    then the sums, then -- at the last sub-step -- the averages."""
    T = acc["ru_m"].dtype.type
    J, K, I = (lambda j: j - b.jms), (lambda k: k - b.kms), (lambda i: i - b.ims)
    ru_m, rv_m, ww_m = acc["ru_m"], acc["rv_m"], acc["ww_m"]
    if iteration == 1:
        for j in range(b.jts, b.jte + 1):
            for k in range(b.kts, b.kte + 1):
                for i in range(b.its, b.ite + 1):
                    ru_m[J(j), K(k), I(i)] = T(0)
                    rv_m[J(j), K(k), I(i)] = T(0)
                    ww_m[J(j), K(k), I(i)] = T(0)
    for j in range(b.jts, min(b.jte, b.jde - 1) + 1):
        for k in range(b.kts, b.kte):
            for i in range(b.its, b.ite + 1):
                ru_m[J(j), K(k), I(i)] = ru_m[J(j), K(k), I(i)] + inp["u"][J(j), K(k), I(i)]
    for j in range(b.jts, b.jte + 1):
        for k in range(b.kts, b.kte):
            for i in range(b.its, min(b.ite, b.ide - 1) + 1):
                rv_m[J(j), K(k), I(i)] = rv_m[J(j), K(k), I(i)] + inp["v"][J(j), K(k), I(i)]
    for j in range(b.jts, min(b.jte, b.jde - 1) + 1):
        for k in range(b.kts, b.kte + 1):
            for i in range(b.its, min(b.ite, b.ide - 1) + 1):
                ww_m[J(j), K(k), I(i)] = ww_m[J(j), K(k), I(i)] + inp["ww"][J(j), K(k), I(i)]
    if iteration == n:
        for j in range(b.jts, min(b.jte, b.jde - 1) + 1):
            for k in range(b.kts, b.kte):
                for i in range(b.its, b.ite + 1):
                    ru_m[J(j), K(k), I(i)] = ru_m[J(j), K(k), I(i)] / T(n) \
                        + (inp["muu"][J(j), I(i)] * inp["u_1"][J(j), K(k), I(i)]) / inp["msfuy"][J(j), I(i)]
        for j in range(b.jts, b.jte + 1):
            for k in range(b.kts, b.kte):
                for i in range(b.its, min(b.ite, b.ide - 1) + 1):
                    rv_m[J(j), K(k), I(i)] = rv_m[J(j), K(k), I(i)] / T(n) \
                        + (inp["muv"][J(j), I(i)] * inp["v_1"][J(j), K(k), I(i)]) * inp["msfvx_inv"][J(j), I(i)]
        for j in range(b.jts, min(b.jte, b.jde - 1) + 1):
            for k in range(b.kts, b.kte + 1):
                for i in range(b.its, min(b.ite, b.ide - 1) + 1):
                    ww_m[J(j), K(k), I(i)] = ww_m[J(j), K(k), I(i)] / T(n) + inp["ww_1"][J(j), K(k), I(i)]
    return acc


@pytest.mark.parametrize("tile", ["whole", "interior", "east"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_reference_equals_the_three_loop_transcription(pkg, dtype, tile):
    b = _bounds(pkg, tile)
    for n in (1, 2, 4):
        got, want = _poison(b, dtype), _poison(b, dtype)
        for it in range(1, n + 1):
            inp = _inputs(b, dtype, 10 * n + it)
            R.sumflux(got, inp, b, it, n)
            _transcription(want, inp, b, it, n)
            for name in R.ACCUMULATORS:
                assert bits_equal(got[name], want[name]), (name, n, it)
        assert all(np.isfinite(got[name][R.tile_mask(b)]).all() for name in R.ACCUMULATORS)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_one_sub_step_is_first_plus_last(pkg, dtype):
    """n == 1: the sum from zero and the average in the one call -- acc = (0 + x) / 1 + base -- and three members at once equal
    three single calls."""
    b = _bounds(pkg)
    inp = _inputs(b, dtype, 3, members=3)
    got = R.sumflux(_poison(b, dtype, 3), inp, b, 1, 1, members=3)
    for m in range(3):
        one = R.sumflux(_poison(b, dtype), {k: v[m] for k, v in inp.items()}, b, 1, 1)
        for name in R.ACCUMULATORS:
            assert bits_equal(got[name][m][R.tile_mask(b)], one[name][R.tile_mask(b)]), (name, m)
    T = np.dtype(dtype).type
    x, base = inp["ww"][0], inp["ww_1"][0]
    mask = R.range_mask(b, "ww_m")
    assert bits_equal(got["ww_m"][0][mask], ((T(0) + x) / T(1) + base)[mask])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_negative_zero_becomes_positive_zero_at_the_first_iteration(pkg, dtype):
    b = _bounds(pkg)
    inp = _inputs(b, dtype, 4)
    for n in ("u", "v", "ww"):
        inp[n][...] = dtype(-0.0)
    acc = R.sumflux(_poison(b, dtype), inp, b, 1, 2)
    for name in R.ACCUMULATORS:
        cells = R.as_bits(acc[name])[R.tile_mask(b)]
        assert (cells == 0).all(), name                           # +0.0: all bits clear, in the range and outside it
    assert np.signbit(inp["u"]).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_poison_does_not_survive_the_first_iteration_and_stays_everywhere_else(pkg, dtype):
    b = _bounds(pkg, "interior")
    before = _poison(b, dtype)
    acc = R.sumflux({k: v.copy() for k, v in before.items()}, _inputs(b, dtype, 5), b, 1, 3)
    tile = R.tile_mask(b)
    for name in R.ACCUMULATORS:
        assert np.isfinite(acc[name][tile]).all(), name
        assert bits_equal(acc[name][~tile], before[name][~tile]), name          # outside the tile, levels kms and kme included
    assert not tile[:, 0, :].any() and not tile[:, -1, :].any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_cells_of_the_tile_outside_a_range_are_zeroed_at_the_first_iteration_only(pkg, dtype):
    b = _bounds(pkg)                                               # ite == ide, jte == jde: the three ranges differ
    masks = {n: R.range_mask(b, n) for n in R.ACCUMULATORS}
    tile = R.tile_mask(b)
    assert len({m.tobytes() for m in masks.values()}) == 3 and all((tile & ~m).any() for m in masks.values())
    acc = R.sumflux(_poison(b, dtype), _inputs(b, dtype, 6), b, 1, 3)
    for name, m in masks.items():
        assert (R.as_bits(acc[name])[tile & ~m] == 0).all(), name
    marked = _poison(b, dtype)
    for name, m in masks.items():
        acc[name][tile & ~m] = marked[name][tile & ~m]
    kept = {k: v.copy() for k, v in acc.items()}
    for it in (2, 3):
        R.sumflux(acc, _inputs(b, dtype, 6 + it), b, it, 3)
        for name, m in masks.items():
            assert bits_equal(acc[name][tile & ~m], kept[name][tile & ~m]), (name, it)
            assert not bits_equal(acc[name][m], kept[name][m]), (name, it)


# ---------------------------------------------------------------------------------------------
# the library's refusals: before any device call, with or without a device, nothing written
# ---------------------------------------------------------------------------------------------
INVALID, PRECONDITION = 3, 2
NAMES13 = R.ACCUMULATORS + R.INPUTS


def _call(pkg, dtype, arrays, b, *, iteration=1, n=2, members=1, null=None):
    L = pkg.load_library()
    fn = L.amt_sumflux_device_f64 if np.dtype(dtype).itemsize == 8 else L.amt_sumflux_device_f32
    ptrs = [None if name == null else ctypes.c_void_p(arrays[name].ctypes.data) for name in NAMES13]
    return fn(None, members, *ptrs, iteration, n, *b.as_tuple())


def _host_arrays(b, dtype, members=1):
    arrays = dict(_poison(b, dtype, members))
    arrays.update(_inputs(b, dtype, 8, members))
    return arrays


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_every_refusal_comes_back_with_its_status_and_writes_nothing(pkg, dtype):
    L = pkg.load_library()
    b = _bounds(pkg)
    arrays = _host_arrays(b, dtype)
    before = {k: v.copy() for k, v in arrays.items()}
    cases = [(f"null {name}", dict(null=name), b, INVALID) for name in NAMES13]
    cases += [("members 0", dict(members=0), b, INVALID), ("members -1", dict(members=-1), b, INVALID),
              ("n 0", dict(n=0, iteration=1), b, INVALID), ("n -2", dict(n=-2, iteration=1), b, INVALID),
              ("iteration 0", dict(iteration=0), b, INVALID), ("iteration n + 1", dict(iteration=3, n=2), b, INVALID),
              ("its < ims", {}, b.replace(its=b.ims - 1), PRECONDITION), ("ite > ime", {}, b.replace(ite=b.ime + 1), PRECONDITION),
              ("jts < jms", {}, b.replace(jts=b.jms - 1), PRECONDITION), ("jte > jme", {}, b.replace(jte=b.jme + 1), PRECONDITION),
              ("kts != 1", {}, b.replace(kts=2), PRECONDITION), ("kte != kde", {}, b.replace(kte=b.kde - 1), PRECONDITION),
              ("kme < kte", {}, b.replace(kme=b.kte - 1), PRECONDITION)]
    for what, kw, bounds, status in cases:
        assert _call(pkg, dtype, arrays, bounds, **kw) == status, (what, L.amt_last_error())
        assert L.amt_last_error(), what
    # an accumulator that overlaps another array of the call: the same array, a shifted one, a 2-D input inside it
    flat = arrays["ru_m"].reshape(-1)
    shifted = flat[1:]
    inside2d = flat[5:5 + arrays["muu"].size].reshape(arrays["muu"].shape)
    overlaps = [("ru_m is u", dict(u=arrays["ru_m"])), ("rv_m is ru_m", dict(rv_m=arrays["ru_m"])),
                ("ww_m one element into ru_m", dict(ww_m=shifted)), ("ww_1 one element into ru_m", dict(ww_1=shifted)),
                ("muu inside ru_m", dict(muu=inside2d)), ("msfvx_inv is the end of ww_m", dict(msfvx_inv=arrays["ww_m"].reshape(-1)[-3:]))]
    for what, swap in overlaps:
        assert _call(pkg, dtype, dict(arrays, **swap), b) == INVALID, (what, L.amt_last_error())
    # inputs may alias one another: not refused for that (without a device the call then stops at the missing device)
    shared = dict(arrays, v=arrays["u"], ww=arrays["u"], v_1=arrays["u_1"], ww_1=arrays["u_1"], muv=arrays["muu"])
    if L.amt_device_count() == 0:
        assert _call(pkg, dtype, shared, b) in (1, 4), L.amt_last_error()
        assert _call(pkg, dtype, arrays, b) in (1, 4), L.amt_last_error()
    for k, v in arrays.items():
        assert bits_equal(v, before[k]), k


def test_more_members_than_one_launch_carries_is_a_precondition(pkg):
    """65536 members of a one-cell patch: the arrays are real (the overlap check sees their full extent) and untouched."""
    L = pkg.load_library()
    b = pkg.synth.Bounds(ids=1, ide=2, jds=1, jde=2, kde=1, ims=1, ime=1, jms=1, jme=1, kms=1, kme=1, its=1, ite=1, jts=1, jte=1, kts=1, kte=1)
    members = 65536
    arrays = {n: np.full((members, 1, 1, 1) if n in R.ACCUMULATORS + R.INPUTS_3D else (members, 1, 1), 1.5, np.float32) for n in NAMES13}
    assert _call(pkg, np.float32, arrays, b, members=members) == PRECONDITION, L.amt_last_error()
    assert b"65535" in L.amt_last_error()
    assert all((a == np.float32(1.5)).all() for a in arrays.values())


def test_the_handle_calls_refuse_a_null_handle(pkg):
    L = pkg.load_library()
    n, nxt = ctypes.c_int(-7), ctypes.c_int(-7)
    for prefix in ("amt_domain", "amt_ensemble"):
        assert getattr(L, f"{prefix}_set_sumflux")(None, 2, None, None, None) == INVALID
        assert getattr(L, f"{prefix}_sumflux_accumulate")(None) == INVALID
        assert getattr(L, f"{prefix}_sumflux_state")(None, ctypes.byref(n), ctypes.byref(nxt)) == INVALID
        assert getattr(L, f"{prefix}_sumflux_ptr")(None, 0) is None
    assert (n.value, nxt.value) == (-7, -7)
