"""tests/packed_state.py on the CPU: the layout's properties, the harness against the oracle (the oracle run on views of one
pool gives the bits it gives on separate arrays and leaves every guard byte alone), and planted defects, each of which ``diff``
must find and name.  The last part is the evidence that tests/test_gpu_17c_packed_state.py can fail."""
import numpy as np
import pytest

import cases
import packed_state as PS
from conftest import bits_equal

DTYPES = [np.float32, np.float64]


def _per(dtype):
    return 16 // np.dtype(dtype).itemsize


def _all_bounds(S):
    """Every memory shape the GPU file packs."""
    out = {}
    for dims, aligned in (((130, 13, 9), False), ((100, 20, 18), True), ((37, 40, 5), False), ((37, 20, 5), False), ((20, 241, 3), False),
                          ((130, 3, 7), False), ((67, 9, 5), False), ((128, 12, 6), True), ((37, 5, 11), False), ((35, 4, 9), False)):
        out[f"{dims}-{'aligned' if aligned else 'minimal'}"] = S.domain_bounds(*dims, aligned=aligned)
    out["40x5x11-ims-3"] = S.domain_bounds(32, 4, 9).replace(ims=-3, ime=36)
    for vw, kpt, hl in ((1, 4, 1), (1, 2, 1), (1, 4, 4), (2, 4, 1), (2, 6, 4)):               # the forced march geometries
        tc = (64 // hl) * vw
        for nk in (3 * kpt * hl, 2 * kpt * hl + 1):
            for aligned in (True, False):
                out[f"march-vw{vw}-kpt{kpt}-hl{hl}-nk{nk}-{aligned}"] = S.domain_bounds(2 * tc + tc // 2 + 3, nk, 7, aligned=aligned)
    return out


# ---------------------------------------------------------------------------------------------
# the layout
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_layout_properties(pkg, dtype, members):
    per, es = _per(dtype), np.dtype(dtype).itemsize
    for what, b in _all_bounds(pkg.synth).items():
        lays = [PS.layout(b, dtype, members, r) for r in range(per)]
        off_line = False
        for r, lay in enumerate(lays):
            assert lay.names == PS.FIELD_NAMES and lay.guard == b.idim * b.kdim + 128, what
            at = 0
            for n in lay.names:                                           # no overlap, every guard wide enough and no wider than the rule
                assert tuple(lay.shapes[n]) == PS.field_shape(b, n, members)
                assert lay.guard <= lay[n] - at <= lay.guard + 2 * per - 1, (what, r, n)
                at = lay.end(n)
            assert lay.length - at == lay.guard, (what, r)
            for x, y in PS.PAIRS:
                assert lay.phase_bytes(x) != lay.phase_bytes(y), (what, r, x, y)
            off_line |= any(lay.phase_bytes(n) == 0 and (lay[n] * es) % 128 for n in PS.RANK3)
        for n in PS.FIELD_NAMES:
            assert sorted(lay.phase_bytes(n) for lay in lays) == [16 * k // per for k in range(per)], (what, n)
        assert off_line, f"{what}: no 3-D array on a 16-byte boundary off a 128-byte line in any rotation"
    with pytest.raises(ValueError):
        PS.layout(b, dtype, members, per)


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_views_are_contiguous_and_alias_the_pool(pkg, dtype, members):
    import torch
    b = pkg.synth.domain_bounds(37, 5, 11)
    lay = PS.layout(b, dtype, members, 1)
    pool = PS.aligned_empty(lay.length, dtype)
    assert pool.ctypes.data % 128 == 0
    pool.view(PS._uint(dtype))[:] = PS.guard_pattern(lay.length, dtype)
    tpool = torch.from_numpy(pool)
    nv, tv = PS.views(pool, lay, b, members), PS.views(tpool, lay, b, members)
    for n in lay.names:
        a, t = nv[n], tv[n]
        assert a.flags["C_CONTIGUOUS"] and np.shares_memory(a, pool) and tuple(a.shape) == tuple(lay.shapes[n])
        assert a.ctypes.data == pool.ctypes.data + lay[n] * pool.itemsize
        assert t.is_contiguous() and t.data_ptr() == tpool.data_ptr() + lay[n] * pool.itemsize and tuple(t.shape) == tuple(lay.shapes[n])
    if members > 1:
        assert nv["t"].shape == (members, b.jdim, b.kdim, b.idim) and nv["t"].reshape(members * b.jdim, b.kdim, b.idim).base is not None
        assert nv["dnw"].shape == (b.kdim,)
    nv["mu"][...] = 1.0                                                    # a write through a view lands in the pool, nowhere else
    want = PS.guard_pattern(lay.length, dtype)
    want[lay["mu"]:lay.end("mu")] = np.ones(1, dtype).view(PS._uint(dtype))[0]
    assert np.array_equal(pool.view(PS._uint(dtype)), want)
    with pytest.raises(ValueError):
        PS.views(pool[:-1], lay)
    with pytest.raises(ValueError):
        PS.views(pool, lay, b, members + 1)


def test_guard_pattern_is_nan_with_a_payload_of_its_own():
    for dtype in DTYPES:
        g = PS.guard_pattern(1000, dtype)
        assert np.unique(g).size == g.size and np.isnan(g.view(dtype)).all()
        quiet = 1 << (51 if np.dtype(dtype).itemsize == 8 else 22)
        assert ((g[0::2] & quiet) != 0).all() and ((g[1::2] & quiet) == 0).all()       # quiet, signalling, quiet ...
    with pytest.raises(ValueError):
        PS.guard_pattern(1 << 22, np.float32)


# ---------------------------------------------------------------------------------------------
# the harness against the oracle
# ---------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle_case(pkg, oracle, shape, flag, dtype):
    """(inputs, oracle outputs on separate arrays): computed once, shared, left unchanged."""
    key = (shape, flag, np.dtype(dtype).name)
    if key not in _ORACLE:
        host = cases.make_case(pkg, shape, flag, dtype)
        want = host.copy()
        oracle.advance_mu_t(*want.args())
        _ORACLE[key] = (host, want)
    return _ORACLE[key]


def _packed(pkg, patch, lay, pool):
    """The patch whose arrays are the views of ``pool``."""
    return pkg.synth.Patch(patch.bounds, patch.config, PS.views(pool, lay, patch.bounds), patch.rdx, patch.rdy, patch.dts, patch.epssm)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("flag", list(cases.FLAG_COMBOS))
@pytest.mark.parametrize("shape", ["37x5x11_ragged", "130x3x7_tile"])
def test_oracle_on_pool_views_equals_oracle_on_separate_arrays(pkg, oracle, shape, flag, dtype):
    host, want = _oracle_case(pkg, oracle, shape, flag, dtype)
    for rotation in range(_per(dtype)):
        lay = PS.layout(host.bounds, dtype, 1, rotation)
        pool = PS.place(host.arrays, lay)
        oracle.advance_mu_t(*_packed(pkg, host, lay, pool).args())
        got = PS.views(pool, lay)
        for n in lay.names:
            assert bits_equal(got[n], want.arrays[n]), (rotation, n)
        assert PS.diff(pool, PS.place(want.arrays, lay), lay) is None              # the guards included
        assert PS.diff(pool, PS.place(host.arrays, lay), lay)["region"] in pkg.synth.OUTPUTS


# ---------------------------------------------------------------------------------------------
# planted defects
# ---------------------------------------------------------------------------------------------
@pytest.fixture(params=DTYPES, ids=["f32", "f64"])
def clean(request, pkg, oracle):
    """(layout, expected pool, bounds) of 37x5x11_ragged / specified after the oracle, rotation 1."""
    host, want = _oracle_case(pkg, oracle, "37x5x11_ragged", "specified", request.param)
    lay = PS.layout(host.bounds, request.param, 1, 1)
    return lay, PS.place(want.arrays, lay), host.bounds


def _bits(pool):
    return pool.view(PS._uint(pool.dtype))


def test_equal_pools_have_no_difference(clean):
    lay, want, _ = clean
    assert PS.diff(PS.clone(want), want, lay) is None
    with pytest.raises(ValueError):
        PS.diff(want[:-1], want, lay)


def test_one_element_written_just_before_t(clean):
    lay, want, _ = clean
    got = PS.clone(want)
    _bits(got)[lay["t"] - 1] = 0
    d = PS.diff(got, want, lay)
    assert d["region"] == "guard before t" and d["distance"] == 1 and d["counts"] == {"guard before t": 1}, d


def test_one_element_written_just_after_ww(clean):
    lay, want, _ = clean
    got = PS.clone(want)
    got[lay.end("ww")] = 300.0
    d = PS.diff(got, want, lay)
    assert d["region"] == "guard after ww" and d["distance"] == 1 and d["counts"] == {"guard after ww": 1}, d
    got[lay["ww_1"] - 3] = 300.0                                            # and three elements in front of the next array
    d = PS.diff(got, want, lay)
    assert d["counts"] == {"guard after ww": 1, "guard before ww_1": 1} and d["region"] == "guard after ww", d


def test_an_output_row_shifted_by_one_element(clean):
    lay, want, b = clean
    got = PS.clone(want)
    j, k = 4, 2
    t = PS.views(got, lay)["t"]
    row = t[j, k].copy()
    start = lay["t"] + (j * b.kdim + k) * b.idim
    _bits(got)[start + 1:start + 1 + b.idim] = _bits(row)                    # the row stored one element late
    first = 1 + int(np.argmax(_bits(row)[:-1] != _bits(row)[1:]))
    d = PS.diff(got, want, lay)
    assert d["region"] == "t" and d["index"] == (j, k, first) and set(d["counts"]) == {"t"}, d
    assert d["counts"]["t"] >= b.idim // 2


def test_a_16_byte_chunk_duplicated_into_a_guard(clean):
    lay, want, _ = clean
    per = 16 // want.itemsize
    got = PS.clone(want)
    _bits(got)[lay.end("mu"):lay.end("mu") + per] = _bits(got)[lay.end("mu") - per:lay.end("mu")]        # array data, one chunk on
    d = PS.diff(got, want, lay)
    assert d["region"] == "guard after mu" and d["distance"] == 1 and d["counts"] == {"guard after mu": per}, d
    got = PS.clone(want)
    e = lay["v"] - 40
    _bits(got)[e:e + per] = _bits(got)[e + per:e + 2 * per]                  # guard bits, one chunk early: the payloads give it away
    d = PS.diff(got, want, lay)
    assert d["region"] == "guard before v" and d["distance"] == 40 and d["counts"] == {"guard before v": per}, d


def test_an_input_changed_in_its_halo(clean):
    lay, want, b = clean
    got = PS.clone(want)
    PS.views(got, lay)["u"][0, 1, b.idim - 1] += 1.0                        # row jms is halo: no window row
    d = PS.diff(got, want, lay)
    assert d["region"] == "u" and d["index"] == (0, 1, b.idim - 1) and d["counts"] == {"u": 1}, d


def test_nan_payloads_are_free_inside_arrays_only(clean):
    lay, want, _ = clean
    u = PS._uint(want.dtype)
    got, ref = PS.clone(want), PS.clone(want)
    e = lay["t"] + 5
    _bits(ref)[e] = PS.guard_pattern(8, want.dtype)[0]                      # a quiet NaN with a payload in the expected array ...
    got[e] = -np.nan                                                       # ... and another NaN where it is
    assert PS.diff(got, ref, lay)["region"] == "t"
    assert PS.diff(got, ref, lay, nan_payloads_free=True) is None
    _bits(got)[lay["t"] - 2] ^= u(1)                                        # a guard's payload stays bytes
    d = PS.diff(got, ref, lay, nan_payloads_free=True)
    assert d["region"] == "guard before t" and d["distance"] == 2, d


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_a_result_that_depends_on_a_guard_element_is_nan(pkg, oracle, dtype):
    """t_1 packed one j row short: the oracle, which trusts the bounds, reads row jme of t_1 from the guard behind it.  Every
    cell of the window's last row then holds NaN, the guard itself keeps its bytes."""
    S = pkg.synth
    host, want = _oracle_case(pkg, oracle, "37x5x11_ragged", "none", dtype)
    b = host.bounds
    shapes = {n: PS.field_shape(b, n) for n in PS.FIELD_NAMES}
    shapes["t_1"] = (b.jdim - 1, b.kdim, b.idim)
    lay = PS.layout(b, dtype, 1, 0, names=shapes)
    short = dict(host.arrays, t_1=host.arrays["t_1"][:-1])
    pool = PS.place(short, lay)
    arrays = PS.views(pool, lay)
    full = b.jdim * b.kdim * b.idim
    assert lay["t_1"] + full <= lay["t_ave"] - 128                          # the missing row lies inside the guard
    arrays["t_1"] = pool[lay["t_1"]:lay["t_1"] + full].reshape(b.jdim, b.kdim, b.idim)
    oracle.advance_mu_t(*S.Patch(b, host.config, arrays, host.rdx, host.rdy, host.dts, host.epssm).args())
    expected = PS.place(dict(want.arrays, t_1=want.arrays["t_1"][:-1]), lay)
    d = PS.diff(pool, expected, lay)
    last = b.jde - 1 - b.jms                                               # the window's last row reads t_1(j + 1) = row jme
    assert d is not None and d["region"] == "t" and d["index"][0] == last and set(d["counts"]) == {"t"}, d
    t = PS.views(pool, lay)["t"]
    assert np.isnan(t[last, :b.kte - 1, b.ids - b.ims:b.ide - b.ims]).all()
    assert np.isfinite(t[:last]).all()
    assert d["counts"]["t"] == (b.kte - 1) * (b.ide - b.ids)
