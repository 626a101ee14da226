"""tests/stream_gate.py without a device: the verdict function on numpy arrays with each of the defects the gated GPU tests
(tests/test_gpu_26_stream_order.py) are there to find planted by hand -- and on a clean case --, and the sizing rule of the gate
as arithmetic.  The planted twins are what a reviewer holds the three library mutations of DESIGN.md section 5 "Stream order"
against: a sweep on the null stream reads poison or runs before the fill (TRUTH / NAN), a dropped join lets boundary cells land
after `done` (LATE, or NAN where the snapshot came first), a record read before its stream wrote it describes poison."""
import numpy as np
import pytest

import stream_gate as G

DTYPES = [np.float64, np.float32]
SHAPE = (5, 4, 7)


def _case(dtype, index=3):
    """(truth, want): inputs as filled and what the oracle makes of them -- it rewrites an interior box."""
    rng = np.random.default_rng(11)
    truth = rng.standard_normal(SHAPE).astype(dtype)
    want = truth.copy()
    want[1:4, 1:3, 1:6] = (truth[1:4, 1:3, 1:6] * dtype(1.5) + dtype(2.0)).astype(dtype)
    return truth, want


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_clean_array_has_no_verdict(dtype):
    truth, want = _case(dtype)
    assert G.verdict(want.copy(), want, truth=truth, index=3, after=want.copy()) is None
    assert G.verdict(truth.copy(), truth, truth=truth, index=3, after=truth.copy()) is None       # an input: the oracle leaves it as filled


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_never_written(dtype):
    truth, want = _case(dtype)
    kind, detail = G.verdict(G.poisoned(SHAPE, dtype, 3), want, truth=truth, index=3)
    assert kind == G.POISON and "array was never written" in detail
    kind, detail = G.verdict(G.poisoned(SHAPE, dtype, 3, snapshot=True), want, truth=truth, index=3)
    assert kind == G.POISON and "snapshot was never written" in detail
    # another array's poison is not this array's: a copy that landed in the wrong place is not "never written"
    kind, _ = G.verdict(G.poisoned(SHAPE, dtype, 4), want, truth=truth, index=3)
    assert kind == G.NAN


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_the_chain_ran_before_the_fill(dtype):
    """The sweep went ahead (to another stream), wrote NaN results, and the fill behind the gate then overwrote them."""
    truth, want = _case(dtype)
    kind, detail = G.verdict(truth.copy(), want, truth=truth, index=3)
    assert kind == G.TRUTH and kind in G.RAN_AHEAD and "before the fill" in detail


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_the_chain_read_poison(dtype):
    """Part of the work (boundary cells on a stream that was not forked behind the inputs) read poison: NaN in those cells."""
    truth, want = _case(dtype)
    got = want.copy()
    got[1:4, 1:3, 5] = np.nan
    kind, detail = G.verdict(got, want, truth=truth, index=3)
    assert kind == G.NAN and kind in G.RAN_AHEAD and "6 cells" in detail and "(1, 1, 5)" in detail
    # cells of the array that nobody wrote hold the poison itself: the same verdict, the bits say which NaN
    got = want.copy()
    got.view(G._uint(dtype))[2, 2, 2] = G.poison_bits(dtype, 3)
    kind, detail = G.verdict(got, want, truth=truth, index=3)
    assert kind == G.NAN and hex(G.poison_bits(dtype, 3)) in detail


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_changed_after_done(dtype):
    """Right in the snapshot, different once everything has been synchronised: work landed behind `done` -- a missing join."""
    truth, want = _case(dtype)
    after = want.copy()
    after[3, 2, 1] += dtype(1.0)
    kind, detail = G.verdict(want.copy(), want, truth=truth, index=3, after=after)
    assert kind == G.LATE and "(3, 2, 1)" in detail
    assert G.verdict(want.copy(), want, truth=truth, index=3, after=None) is None       # earlier snapshots are not held against `after`


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_any_other_difference_and_the_nan_rule(dtype):
    truth, want = _case(dtype)
    got = want.copy()
    got.view(G._uint(dtype))[1, 1, 1] ^= 1                        # one bit
    kind, detail = G.verdict(got, want, truth=truth, index=3)
    assert kind == G.WRONG and "1 cells" in detail
    assert G.verdict(want.astype(np.float32 if dtype == np.float64 else np.float64), want)[0] == G.WRONG
    # a planted NaN propagates with a platform's own payload: equal only where the case says so; a NaN too many is still NAN
    want_nan = want.copy()
    want_nan[2, 2, 3] = np.nan
    got = want_nan.copy()
    got.view(G._uint(dtype))[2, 2, 3] |= 5
    assert G.verdict(got, want_nan, nan_payloads_free=True) is None
    assert G.verdict(got, want_nan)[0] == G.WRONG
    got[2, 2, 4] = np.nan
    assert G.verdict(got, want_nan, nan_payloads_free=True)[0] == G.NAN


def test_poison_numbers_every_array_and_its_snapshot():
    for dtype in DTYPES:
        seen = set()
        for index in range(40):
            for snapshot in (False, True):
                bits = G.poison_bits(dtype, index, snapshot)
                a = np.array([bits], dtype=G._uint(dtype)).view(dtype)
                assert np.isnan(a[0]) and bits not in seen
                quiet = 1 << (51 if np.dtype(dtype).itemsize == 8 else 22)
                assert bits & quiet
                seen.add(bits)
    with pytest.raises(ValueError):
        G.poison_bits(np.float32, 1 << 21)


def test_verdicts_walks_every_snapshot_and_holds_the_last_against_after():
    truth, want = _case(np.float64)
    names = ["a", "b"]
    late = want.copy()
    late[0, 0, 0] = 7.0
    r = G.Result(names=names, snaps=[dict(a=want.copy(), b=truth.copy()), dict(a=want.copy(), b=want.copy())],
                 after=dict(a=late, b=want.copy()))
    got = G.verdicts(r, [dict(a=want, b=want), dict(a=want, b=want)], dict(a=truth, b=truth))
    assert [(s, n, kind) for s, n, kind, _ in got] == [(0, "b", G.TRUTH), (1, "a", G.LATE)]


def test_sizing_rule():
    """At least MARGIN x the host time of the chain and at least FLOOR_MS; repetitions round up, with HEADROOM, never below one."""
    assert (G.MARGIN, G.FLOOR_MS, G.RETRY_FACTOR) == (20.0, 50.0, 4)
    assert G.gate_ms_needed(0.0) == 50.0
    assert G.gate_ms_needed(1e-3) == 50.0                         # 20 x 1 ms = 20 ms: the floor holds
    assert G.gate_ms_needed(2.5e-3) == 50.0
    assert G.gate_ms_needed(4e-3) == pytest.approx(80.0)
    assert G.gate_ms_needed(0.1) == pytest.approx(2000.0)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            G.gate_ms_needed(bad)
    assert G.HEADROOM >= 1.0
    for need, per in ((50.0, 0.13), (80.0, 0.27), (50.0, 49.0), (50.0, 500.0), (200.0, 1.0)):
        n = G.repetitions(need, per)
        assert n >= 1 and n * per >= need * G.HEADROOM - 1e-9
        assert (n - 1) * per < need * G.HEADROOM or n == 1            # and not one more than that
    assert G.repetitions(50.0, 500.0) == 1
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            G.repetitions(50.0, bad)
    # the retry: four times the need gives four times the repetitions, up to rounding
    n1, n4 = G.repetitions(50.0, 0.13), G.repetitions(50.0 * G.RETRY_FACTOR, 0.13)
    assert 4 * n1 - 4 <= n4 <= 4 * n1
