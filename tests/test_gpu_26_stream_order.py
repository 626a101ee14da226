"""Stream-order parity (tests/stream_gate.py): every device path of the library enqueued behind a BUSY stream.  Each case
runs twice on fresh state -- ungated (the warm-up and timing run, which must already equal the oracle), then behind a gate
that is still running while the host enqueues the fill of the inputs, the library chain and the snapshot.  The arrays the
library is given hold poison (NaNs that name their array) until the fill behind the gate has run, so work on a wrong stream,
in front of a missing fork, or read by the host before its stream wrote it, shows as poison, as NaN, as the untouched inputs,
or as a change after the stream reported done (stream_gate.verdict).

a: pointer level on the caller's stream (asynchronous): the sweep in every kernel family, the ensemble call, the chain cyclic
   refresh -> sweep -> boundary-zone update -> moments, the synthetic fill, three sweeps with refills behind ONE gate;
b: pointer level, host-waiting: statistics and comparison on the gated stream, and two host threads of which one is gated;
c: resident handles (library-owned on its own stream, wrapped over the caller's stream, ensembles with moments into a domain);
d: the non-finite guard: step returns AMT_OK while the gate runs, sync reports, the next step enqueues nothing;
e: the host-owned halo exchange 1 x 2 and 2 x 1 with this file as the transport (begin behind gates, halo_wait must wait),
   and the native steppers as their own neighbour over the IPC transport (tests/workers/stream_order_rank.py): in process the
   host-waited default and AMT_SLAB_NO_OVERLAP, in ONE fresh child process the device-waited schedule;
f: three independent handles behind three gates at once;
g: the detector detects: the chain of (a) with its sweep on a stream that is NOT ordered behind the fill must come out dirty.

Not here: RCCL and real multi-process schedules (they stay with tests/test_gpu_30..35).  No wall-clock assertion decides a
parity verdict; the gate times are measured, printed, and written as JSON to the file AMT_STREAM_ORDER_RECORD names, if set."""
import ctypes
import json
import os
import threading
import time
from pathlib import Path

import numpy as np
import pytest

import cases
import cyclic_ref as CR
import diag_ref as D
import moments_ref as R
import specbdy_ref as SB
import stream_gate as G
from conftest import bits_equal

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
X = CR.CYCLIC_X
LEFT, RIGHT = 4, 8
RECORD = {}

# name -> (dtype, (ni, nk, nj), padded rows)
SHAPES = {
    "f64-130x12x9": (F64, (130, 12, 9), False),            # unpadded odd rows (132 elements: no whole 128-byte lines)
    "f32-130x12x9": (F32, (130, 12, 9), False),
    "f64-257x60x33": (F64, (257, 60, 33), True),           # the headline LDS-DMA shape <double,1,4,1,0,true,true,16>: a CU whole
    "f32-130x40x9": (F32, (130, 40, 9), False),            # two columns per lane
    "f64-37x70x5": (F64, (37, 70, 5), False),              # 70 levels: the column kernel recomputes
}
NAMES5 = ("t", "ft", "mu", "muts", "mu_tend")
NAMES9 = ("u", "u_1", "v", "v_1", "t_1", "muu", "muv", "msfuy", "msfvx_inv")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def gate(pkg, torch_mod):
    """The session's gate and its calibration; the record of every case is printed at the end, and written to the file the
    environment variable AMT_STREAM_ORDER_RECORD names when it is set (its folder must exist)."""
    g = G.Gate(torch_mod, pkg.load_library())
    RECORD["calibration"] = dict(bytes_per_repetition=g.nbytes, ms_per_repetition=round(g.ms_per_repetition, 4),
                                 margin=G.MARGIN, floor_ms=G.FLOOR_MS, headroom=G.HEADROOM)
    yield g
    print("stream order:", json.dumps(RECORD))
    out = os.environ.get("AMT_STREAM_ORDER_RECORD")
    if out and Path(out).parent.is_dir():
        Path(out).write_text(json.dumps(RECORD, indent=1) + "\n")


@pytest.fixture()
def force(pkg):
    L = pkg.load_library()
    yield lambda *a: L.amt_march_force_shape(*a)
    L.amt_march_force_shape(0, 0, 0, -1, 1, 0, 0)


# ---------------------------------------------------------------------------------------------
# shared: inputs, references (computed once, never changed), the assertion
# ---------------------------------------------------------------------------------------------
_TRUTH = {}


def _truth(pkg, shape, flag, seed, members=1):
    """(bounds, config, first member's host patch, name -> numpy array: member-stacked where members > 1).  Cached; read only."""
    key = (shape, flag, seed, members)
    if key not in _TRUTH:
        S = pkg.synth
        dtype, dims, aligned = SHAPES[shape]
        b = S.domain_bounds(*dims, aligned=aligned)
        cfg = pkg.GridConfig(**cases.FLAG_COMBOS[flag])
        ps = [S.make_patch(b, cfg, dtype=dtype, seed=seed + 10 * m, global_dims=dims) for m in range(members)]
        arrays = ps[0].arrays if members == 1 else \
            {n: (ps[0].arrays[n] if S.field_rank(n) == 1 else np.stack([p.arrays[n] for p in ps])) for n in S.FIELD_NAMES}
        _TRUTH[key] = (b, cfg, ps[0], arrays)
    return _TRUTH[key]


def _copy(arrays):
    return {n: a.copy() for n, a in arrays.items()}


def _member(S, p0, arrays, m, members):
    one = arrays if members == 1 else {n: (a if S.field_rank(n) == 1 else a[m]) for n, a in arrays.items()}
    return S.Patch(p0.bounds, p0.config, one, p0.rdx, p0.rdy, p0.dts, p0.epssm, p0.global_dims)


def _sweep(pkg, oracle, p0, arrays, members):
    for m in range(members):
        oracle.advance_mu_t(*_member(pkg.synth, p0, arrays, m, members).args())


def _flags(cfg):
    return tuple(int(x) for x in cfg.as_ints())


def _to_device(torch, arrays):
    return {n: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for n, a in arrays.items()}


def _blank(torch, arrays):
    """Fresh device tensors of the arrays' shapes (run_gated poisons them)."""
    return {n: torch.empty(a.shape, dtype=torch.float64 if a.dtype == np.float64 else torch.float32, device="cuda:0")
            for n, a in arrays.items()}


def _clean(label, pair, wants, truth=None, nan_payloads_free=False):
    """Both runs of a case against the oracle: no array of any snapshot has a verdict."""
    for which, result in zip(("ungated", "gated"), pair):
        bad = G.verdicts(result, wants, truth, nan_payloads_free=nan_payloads_free)
        assert not bad, f"{label}, {which} run: " + "; ".join(f"snapshot {s} {n}: {kind} ({detail})" for s, n, kind, detail in bad[:8])
    assert pair[1].gate_ms >= G.MARGIN * pair[0].host_s * 1e3 and pair[1].gate_ms >= G.FLOOR_MS, \
        f"{label}: the gate lasted {pair[1].gate_ms:.1f} ms for a chain of {pair[0].host_s * 1e3:.2f} ms host time"


def _kernel(pkg):
    return pkg.load_library().amt_march_last_kernel().decode()


# ---------------------------------------------------------------------------------------------
# a: pointer level, the caller's stream
# ---------------------------------------------------------------------------------------------
AUTO, COLUMN, MARCH = 0, 1, 2
# id: (shape, flags, forced wave shape or None, variant, members, what the kernel's name must hold)
CALLS = {
    "dma-headline": ("f64-257x60x33", "specified_periodic_x", (1, 4, 1, 0, 1, 0, 16), MARCH, 1, "amt_march_kernel<double, 1, 4, 1, 0, FULL, true, 16, nt>"),
    "register-twin": ("f64-257x60x33", "none", (1, 4, 1, 0, 0, 0, 16), MARCH, 1, "amt_march_kernel<double, 1, 4, 1, 0, FULL, false, 16, nt>"),
    "auto-f64-odd-rows": ("f64-130x12x9", "specified_periodic_x", None, AUTO, 1, ", cached>"),
    "auto-f64-60-levels": ("f64-257x60x33", "none", None, AUTO, 1, "amt_march_kernel<double"),
    "f32-two-columns": ("f32-130x40x9", "none", (2, 0, 0, -1, 1, 0, 0), MARCH, 1, "amt_march_kernel<float, 2, "),
    "column-lds": ("f64-130x12x9", "none", None, COLUMN, 1, "amt_column_kernel"),
    "column-recompute-70": ("f64-37x70x5", "specified_periodic_x", None, COLUMN, 1, "amt_column_kernel"),
    "ensemble-3": ("f64-130x12x9", "specified_periodic_x", None, AUTO, 3, "members=3"),
    "ensemble-3-f32-column": ("f32-130x12x9", "none", None, COLUMN, 3, "amt_column_kernel"),
}


@pytest.mark.parametrize("case", list(CALLS))
def test_device_call_behind_a_busy_stream(pkg, oracle, torch_mod, gate, force, case):
    """amt_advance_mu_t_device_* / amt_advance_mu_t_ensemble_device_* on the caller's stream: all 26 arrays at `done` are the
    oracle's (outputs) or the inputs as filled, and nothing moves afterwards."""
    torch, S = torch_mod, pkg.synth
    shape, flag, forced, variant, members, name = CALLS[case]
    b, cfg, p0, truth = _truth(pkg, shape, flag, 260, members)
    want = _copy(truth)
    _sweep(pkg, oracle, p0, want, members)
    truth_dev = _to_device(torch, truth)
    if forced:
        force(*forced)                                             # before any gate: process state, not stream work
    seen = []

    def make():
        live = _blank(torch, truth)
        patch = S.Patch(b, cfg, live, p0.rdx, p0.rdy, p0.dts, p0.epssm)

        def chain(ctx):
            if members == 1:
                pkg.advance_mu_t(*patch.args(), stream=ctx.stream, variant=variant)
            else:
                pkg.advance_mu_t_ensemble(*patch.args(), stream=ctx.stream, variant=variant)
            seen.append(_kernel(pkg))
        return dict(chain=chain, live=live, truth=truth_dev, stream=torch.cuda.Stream())

    pair = G.run_case(make, gate, torch=torch, record=RECORD, label=f"a/device-call/{case}")
    assert all(name in k for k in seen), (case, seen)
    _clean(case, pair, [want], truth)


@pytest.mark.parametrize("shape", ["f64-130x12x9", "f32-130x12x9"])
def test_refresh_sweep_zone_update_moments_chain(pkg, oracle, torch_mod, gate, shape):
    """amt_cyclic_fill_device -> ensemble sweep -> amt_spec_bdy_update_device -> amt_moments_device (all four outputs of t over
    three members, an odd box) on one stream.  The wrap cells of the inputs hold NaN as filled: the refresh has to come first."""
    torch, S = torch_mod, pkg.synth
    members = 3
    b, cfg, p0, made = _truth(pkg, shape, "specified_periodic_x", 270, members)
    dtype = SHAPES[shape][0]
    truth = _copy(made)
    _poison_wrap_cells(truth, b)
    ext = (b.ims, b.ime, b.jms, b.jme, b.kms, b.kme)
    box = (b.ims + 1, b.ime - 1, b.kms, b.kme - 1, b.jms + 1, b.jme - 1)
    want = _copy(truth)
    CR.cyclic_fill(want, b, X, _flags(cfg))
    _sweep(pkg, oracle, p0, want, members)
    SB.spec_bdy_update(want, b, _flags(cfg), p0.dts)
    ref, idx = R.moments(want["t"], ext, box), R.member_index(want["t"], ext, box)
    one = want["t"].shape[1:]
    for k, n in enumerate(R.NAMES):                                # outside the box an output keeps its poison
        want[n] = R.expected(G.poisoned(one, dtype, len(S.FIELD_NAMES) + k), ref[n], idx)
    truth_dev = _to_device(torch, truth)

    def make():
        live = _blank(torch, truth)
        outs = _blank(torch, {n: want[n] for n in R.NAMES})

        def chain(ctx):
            pkg.cyclic_fill(*[live[n] for n in NAMES9], cfg, *b.as_tuple(), axes=X, members=members, stream=ctx.stream)
            pkg.advance_mu_t_ensemble(*S.Patch(b, cfg, live, p0.rdx, p0.rdy, p0.dts, p0.epssm).args(), stream=ctx.stream)
            pkg.spec_bdy_update(*[live[n] for n in NAMES5], p0.dts, cfg, *b.as_tuple(), members=members, stream=ctx.stream)
            pkg.diag.moments(live["t"], extents=ext, box=box, stream=ctx.stream, want=R.NAMES, out=outs)
        return dict(chain=chain, live=live, truth=truth_dev, stream=torch.cuda.Stream(), outputs=outs)

    pair = G.run_case(make, gate, torch=torch, record=RECORD, label=f"a/chain/{shape}")
    _clean(shape, pair, [want], truth)


def _poison_wrap_cells(arrays, b):
    """NaN where a cyclic-x refresh writes: column ide of u, u_1, t_1, muu, msfuy and column ids-1 of t_1 (numpy or torch)."""
    for n in CR.COLS_FROM_RIGHT:
        arrays[n][..., b.ide - b.ims] = np.nan
    arrays["t_1"][..., b.ids - 1 - b.ims] = np.nan


def test_synthetic_fill_is_the_fill(pkg, oracle, torch_mod, gate):
    """amt_synth_fill_device of all 26 arrays behind the gate, then a sweep: the inputs at `done` are amt_synth_fill_host's."""
    torch, S = torch_mod, pkg.synth
    from wrf_model_cuda_sample_amd import lib
    L = pkg.load_library()
    shape = "f32-130x40x9"
    b, cfg, p0, truth = _truth(pkg, shape, "none", 280)
    dims = SHAPES[shape][1]
    want = _copy(truth)
    _sweep(pkg, oracle, p0, want, 1)

    def make():
        live = _blank(torch, truth)

        def fill(ctx):
            for n in S.FIELD_NAMES:
                fa, _rank = S._fill_args(b, n, dims)
                lib.check(L.amt_synth_fill_device(ctypes.c_void_p(ctx.handle), S.FIELD_ID[n], live[n].element_size(),
                                                  ctypes.c_void_p(live[n].data_ptr()), ctypes.c_uint64(280), *fa))

        def chain(ctx):
            pkg.advance_mu_t(*S.Patch(b, cfg, live, p0.rdx, p0.rdy, p0.dts, p0.epssm).args(), stream=ctx.stream)
        return dict(chain=chain, live=live, truth=None, stream=torch.cuda.Stream(), fill=fill)

    pair = G.run_case(make, gate, torch=torch, record=RECORD, label="a/synth-fill")
    _clean("synthetic fill", pair, [want], truth)


@pytest.mark.parametrize("shape", ["f64-257x60x33", "f32-130x40x9"])
def test_three_sweeps_with_refills_behind_one_gate(pkg, oracle, torch_mod, gate, shape):
    """Sweep s is followed by new u, v, u_1, v_1, t_1 for sweep s + 1 with no host wait in between: a refill that overtakes the
    sweep in front of it (write after read), or a sweep that overtakes its refill, changes a snapshot."""
    torch, S = torch_mod, pkg.synth
    names = ("u", "v", "u_1", "v_1", "t_1")
    b, cfg, p0, truth = _truth(pkg, shape, "none", 290)
    fresh = [None] + [{n: _truth(pkg, shape, "none", 290 + 100 * s)[3][n] for n in names} for s in (1, 2)]
    wants, state = [], _copy(truth)
    for s in range(3):
        if s:
            state.update(_copy(fresh[s]))
        _sweep(pkg, oracle, p0, state, 1)
        wants.append(_copy(state))
    truth_dev = _to_device(torch, truth)
    fresh_dev = [None] + [_to_device(torch, f) for f in fresh[1:]]

    def make():
        live = _blank(torch, truth)
        args = S.Patch(b, cfg, live, p0.rdx, p0.rdy, p0.dts, p0.epssm).args()

        def chain(ctx):
            for s in range(3):
                if s:
                    G.copy_fill(ctx, live, fresh_dev[s])
                pkg.advance_mu_t(*args, stream=ctx.stream)
                if s < 2:
                    ctx.snapshot()
        return dict(chain=chain, live=live, truth=truth_dev, stream=torch.cuda.Stream(), snapshots=3)

    pair = G.run_case(make, gate, torch=torch, record=RECORD, label=f"a/three-sweeps/{shape}")
    _clean(shape, pair, wants)


# ---------------------------------------------------------------------------------------------
# b: pointer level, calls that wait on the host by contract
# ---------------------------------------------------------------------------------------------
def _diag_truth(pkg, dtype):
    """(a, b, extents, box): a member-stacked t and a copy with two flipped bits, a NaN and an Inf per member."""
    shape = "f64-130x12x9" if dtype == F64 else "f32-130x12x9"
    bd, _cfg, _p0, arrays = _truth(pkg, shape, "none", 300, 3)
    a = arrays["t"]
    other = a.copy()
    u = G._uint(dtype)
    other.view(u)[:, 3, 2, 17] ^= u(1)
    other.view(u)[:, 7, 9, 101] ^= u(4)
    other[:, 5, 4, 60] = np.nan
    other[:, 6, 1, 9] = np.inf
    ext = (0, bd.idim - 1, 0, bd.jdim - 1, 0, bd.kdim - 1)
    box = (1, bd.idim - 2, 1, bd.kdim - 1, 1, bd.jdim - 2)
    return a, other, ext, box


def _stats_match(rec, ref, what):
    assert (rec.count, rec.n_nan, rec.n_inf, rec.first_nonfinite, rec.min, rec.max, rec.max_abs) == \
           (ref["count"], ref["n_nan"], ref["n_inf"], ref["first_nonfinite"], ref["min"], ref["max"], ref["max_abs"]), (what, rec)
    assert abs(rec.sum - ref["sum"]) <= D.sum_bound(ref["count"], ref["abs_sum"]), (what, rec.sum, ref["sum"])


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["stats", "compare"])
def test_host_waiting_diagnostics_behind_a_busy_stream(pkg, torch_mod, gate, kind, dtype):
    """amt_stats_device_* / amt_compare_device_* enqueue on the gated stream and wait for it: the gate is still running
    immediately before the call, and the records describe the inputs the fill behind the gate wrote -- not the poison the
    arrays held when the call was made (every cell NaN, every pair different), and not what the calling thread's page-locked
    record buffer held before: the pointer-level calls keep that buffer per host thread, so before EACH run (before the gate)
    a scrub call on OTHER operands leaves a record in it that differs from the expected one in every member.  A call that
    copied the buffer before its stream had written it would return the scrub's record -- in the gated run every time, since
    the kernel then sits behind a gate of 50 ms; in the ungated run only as far as the copy wins the race with a 20 us kernel."""
    torch = torch_mod
    a, other, ext, box = _diag_truth(pkg, dtype)
    truth = dict(a=a, b=other)
    truth_dev = _to_device(torch, truth)
    got, scrubs = [], []

    def expected(m):
        if kind == "stats":
            return D.stats(other[m], ext, box)
        return D.diff(a[m], other[m], ext, box)

    def matches(rec, ref):
        if kind == "stats":
            try:
                _stats_match(rec, ref, "")
                return True
            except AssertionError:
                return False
        return (rec.count, rec.n_diff, rec.first_diff, rec.max_abs_diff) == (ref["count"], ref["n_diff"], ref["first_diff"], ref["max_abs_diff"])

    def make():
        live = _blank(torch, truth)
        # the scrub, on the idle device and before the gate: statistics of `a` (no NaN, no Inf) / `a` against itself (no difference)
        if kind == "stats":
            scrubs.append(pkg.diag.field_stats(truth_dev["a"], stacked=True, extents=ext, box=box))
        else:
            scrubs.append(pkg.diag.compare(truth_dev["a"], truth_dev["a"], stacked=True, extents=ext, box=box))
        torch.cuda.synchronize()

        def chain(ctx):
            ctx.gate_must_be_running(kind)
            if kind == "stats":
                got.append(pkg.diag.field_stats(live["b"], stacked=True, extents=ext, box=box, stream=ctx.stream))
            else:
                got.append(pkg.diag.compare(live["a"], live["b"], stacked=True, extents=ext, box=box, stream=ctx.stream))
        return dict(chain=chain, live=live, truth=truth_dev, stream=torch.cuda.Stream())

    label = f"b/{kind}/{np.dtype(dtype).name}"
    pair = G.run_case(make, gate, torch=torch, asynchronous=False, record=RECORD, label=label)
    assert len(got) >= 2 and len(scrubs) == len(got)
    for m in range(3):                                             # the record a too-early read would return is not the expected one
        left = D.stats(a[m], ext, box) if kind == "stats" else D.diff(a[m], a[m], ext, box)
        assert (left["n_nan"], left["n_inf"]) != (expected(m)["n_nan"], expected(m)["n_inf"]) if kind == "stats" \
            else left["n_diff"] != expected(m)["n_diff"], (label, m)
    wrong = [(which, m, str(records[m])) for which, records in (("ungated", got[0]), ("gated", got[-1])) for m in range(3)
             if not matches(records[m], expected(m))]
    assert not wrong, f"{label}: records that do not describe the inputs behind the gate (run, member, record): {wrong}"
    assert bytes(got[0][0]) == bytes(got[-1][0])                   # the same bytes as on the idle device
    for which, result in zip(("ungated", "gated"), pair):          # and the operands are the inputs as filled
        bad = G.verdicts(result, [truth], truth)
        assert not bad, (label, which, bad)


def test_two_host_threads_one_of_them_gated(pkg, torch_mod, gate):
    """Two host threads, a stream each, amt_stats_device_f64 in both; thread A's stream is gated.  The workspace is per thread:
    B's call returns while A's gate is still running (no device-wide wait, no shared record), and both records are right."""
    torch = torch_mod
    a, other, ext, box = _diag_truth(pkg, F64)
    dev = _to_device(torch, dict(a=a, b=other))

    def stats(t, s):
        return pkg.diag.field_stats(t, stacked=True, extents=ext, box=box, stream=s)

    def once(factor):
        live_a = torch.empty_like(dev["b"])
        G._fill_bits(torch, live_a, G.poison_bits(F64, 0))
        streams = dict(A=torch.cuda.Stream(), B=torch.cuda.Stream())
        out, errors, times = {}, [], {}
        warmed, enqueued = threading.Barrier(2), threading.Event()
        torch.cuda.synchronize()

        def thread_a():
            try:
                torch.cuda.set_device(0)
                t0 = time.perf_counter()
                stats(dev["a"], streams["A"])                      # this thread's workspace exists before the gate (OTHER data:
                times["warm"] = time.perf_counter() - t0           # a record left over from here is not the gated call's)
                warmed.wait(30)
                run = gate.enqueue(streams["A"], factor * G.gate_ms_needed(4 * times["warm"]))
                with torch.cuda.stream(streams["A"]):
                    live_a.copy_(dev["b"], non_blocking=True)
                times["gate"] = run
                enqueued.set()
                times["a_running_before"] = not run.done.query()
                out["A"] = stats(live_a, streams["A"])
                times["a_done"] = time.perf_counter()
            except BaseException as e:                             # noqa: BLE001 -- reported by the main thread
                errors.append(e)
                enqueued.set()

        def thread_b():
            try:
                torch.cuda.set_device(0)
                stats(dev["b"], streams["B"])
                warmed.wait(30)
                assert enqueued.wait(30)
                out["B"] = stats(dev["a"], streams["B"])
                times["b_done"] = time.perf_counter()
                times["a_running_at_b_return"] = "gate" in times and not times["gate"].done.query()
            except BaseException as e:                             # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=thread_a), threading.Thread(target=thread_b)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(60)
        torch.cuda.synchronize()
        assert not errors, errors
        assert not any(t.is_alive() for t in threads)
        return out, times

    out, times = once(1)
    retried = not (times["a_running_before"] and times["a_running_at_b_return"]
                   and times["gate"].ms() >= G.gate_ms_needed(times["warm"]))
    if retried:                                                    # a descheduled host thread: once more, four times the gate
        out, times = once(G.RETRY_FACTOR)
    RECORD["b/two-threads"] = dict(host_enqueue_ms=round(times["warm"] * 1e3, 3), gate_needed_ms=round(times["gate"].need_ms, 3),
                                   gate_measured_ms=round(times["gate"].ms(), 3), retried_4x=retried,
                                   gate_running_before_gated_call=bool(times["a_running_before"]),
                                   gate_running_when_ungated_thread_returned=bool(times["a_running_at_b_return"]))
    assert times["a_running_before"], "the gate had ended before thread A's call: the case proves nothing"
    assert times["a_running_at_b_return"], "the ungated thread's call waited for the gated thread's stream"
    assert times["b_done"] < times["a_done"]
    # the sizing rule, against the host time of thread A's own (warm-up) call -- its first, workspace allocation included
    assert times["gate"].ms() >= G.gate_ms_needed(times["warm"]), \
        f"the gate lasted {times['gate'].ms():.1f} ms for a call of {times['warm'] * 1e3:.2f} ms host time"
    for m in range(3):
        _stats_match(out["A"][m], D.stats(other[m], ext, box), ("thread A", m))
        _stats_match(out["B"][m], D.stats(a[m], ext, box), ("thread B", m))


# ---------------------------------------------------------------------------------------------
# c: resident handles
# ---------------------------------------------------------------------------------------------
def _exchanged_mask(S):
    m = 0
    for n in S.EXCHANGED_INPUTS:
        m |= 1 << S.FIELD_ID[n]
    return m


def _fill_args(b, dims):
    return (b.ims, b.kms - 1, b.jms, dims[0] + 2, dims[1] + 1, dims[2] + 2)


def _views(pkg, torch, owner, b, dtype):
    S = pkg.synth
    return {n: torch.as_tensor(owner.view(S.FIELD_ID[n], b.shape(n), "<f8" if dtype == F64 else "<f4"), device="cuda:0")
            for n in S.FIELD_NAMES}


def test_library_owned_handle_on_its_own_stream(pkg, oracle, torch_mod, gate):
    """amt_domain_create, gated through ExternalStream(amt_domain_stream(h)), cyclic refresh + boundary-zone update + guard armed
    TOGETHER on a periodic_x + specified channel.  Behind ONE gate: amt_domain_fill_synthetic, then per sweep
    amt_domain_fill_fields(seed + s), NaN into the wrap cells, amt_domain_step(h, 1), a snapshot.  Per-sweep references as
    tests/test_gpu_17c_packed_state.py builds them: refill, poison, cyclic_ref, the oracle, specbdy_ref."""
    torch, S = torch_mod, pkg.synth
    from wrf_model_cuda_sample_amd import lib
    L = pkg.load_library()
    shape, seed = "f64-257x60x33", 310
    dtype, dims, _al = SHAPES[shape]
    b, cfg, p0, truth = _truth(pkg, shape, "specified_periodic_x", seed)
    flags = _flags(cfg)
    wants, state = [], _copy(truth)
    host = S.Patch(b, cfg, state, p0.rdx, p0.rdy, p0.dts, p0.epssm, dims)
    for s in range(3):
        S.refresh_exchanged_inputs(host, seed, s)
        _poison_wrap_cells(state, b)
        CR.cyclic_fill(state, b, X, flags)
        _sweep(pkg, oracle, p0, state, 1)
        SB.spec_bdy_update(state, b, flags, p0.dts)
        wants.append(_copy(state))
    reports = []

    def make():
        owner = S.NativeDomain(b, cfg, np.dtype(dtype).itemsize)
        h = owner.handle
        live = _views(pkg, torch, owner, b, dtype)
        stream = torch.cuda.ExternalStream(int(L.amt_domain_stream(h)))
        lib.check(L.amt_domain_set_scalars(h, p0.rdx, p0.rdy, p0.dts, p0.epssm))
        lib.check(L.amt_domain_set_cyclic(h, X))
        lib.check(L.amt_domain_set_spec_bdy(h, 1))
        lib.check(L.amt_domain_set_guard(h, 1))

        def fill(ctx):
            lib.check(L.amt_domain_fill_synthetic(h, ctypes.c_uint64(seed), *_fill_args(b, dims)))

        def chain(ctx):
            for s in range(3):
                lib.check(L.amt_domain_fill_fields(h, ctypes.c_uint64(_exchanged_mask(S)), ctypes.c_uint64(seed + s), *_fill_args(b, dims)))
                with torch.cuda.stream(ctx.stream):
                    _poison_wrap_cells(live, b)
                lib.check(L.amt_domain_step(h, 1))
                if s < 2:
                    ctx.snapshot()

        def finish():
            lib.check(L.amt_domain_sync(h))
            rep = lib.GuardReport()
            lib.check(L.amt_domain_guard_report(h, ctypes.byref(rep)))
            reports.append(rep)
        return dict(chain=chain, live=live, truth=None, stream=stream, fill=fill, snapshots=3, finish=finish)

    pair = G.run_case(make, gate, torch=torch, record=RECORD, label="c/domain-create")
    _clean("amt_domain_create handle", pair, wants)
    for rep in reports:
        assert (rep.sweeps_checked, rep.sweep, rep.n_nonfinite) == (3, 0, 0), rep


@pytest.mark.parametrize("kind,shape", [("domain", "f32-130x40x9"), ("ensemble", "f64-130x12x9")])
def test_wrapped_handles_use_the_callers_stream_for_everything(pkg, oracle, torch_mod, gate, kind, shape):
    """amt_domain_wrap / amt_ensemble_wrap (3 members) over torch tensors on a torch.cuda.Stream(): step(3) with the cyclic
    refresh, the boundary-zone update and the guard armed; the ensemble then takes amt_ensemble_moments of t (window) into the
    fields of a same-shaped amt_domain.  Everything -- refresh, sweeps, update, guard launches, moments -- is behind the
    caller's gate."""
    torch, S = torch_mod, pkg.synth
    from wrf_model_cuda_sample_amd import lib
    L = pkg.load_library()
    members = 3 if kind == "ensemble" else 1
    dtype, dims, _al = SHAPES[shape]
    b, cfg, p0, made = _truth(pkg, shape, "specified_periodic_x", 320, members)
    flags = _flags(cfg)
    truth = _copy(made)
    _poison_wrap_cells(truth, b)
    want = _copy(truth)
    for _s in range(3):
        CR.cyclic_fill(want, b, X, flags)
        _sweep(pkg, oracle, p0, want, members)
        SB.spec_bdy_update(want, b, flags, p0.dts)
    into = dict(mean="t", var="t_1", lo="ww", hi="u")              # moment -> the field of the amt_domain that receives it
    if kind == "ensemble":
        ext = (b.ims, b.ime, b.jms, b.jme, b.kms, b.kme)
        i0, i1, j0, j1, k0, k1 = pkg.compute_window(cfg, b.ids, b.ide, b.jds, b.jde, b.its, b.ite, b.jts, b.jte, b.kts, b.kte)
        box = (i0, i1, k0, k1, j0, j1)
        ref, idx = R.moments(want["t"], ext, box), R.member_index(want["t"], ext, box)
        one = want["t"].shape[1:]
        for k, n in enumerate(R.NAMES):
            want["moment_" + n] = R.expected(G.poisoned(one, dtype, len(S.FIELD_NAMES) + k), ref[n], idx)
    truth_dev = _to_device(torch, truth)
    reports = []

    def make():
        live = _blank(torch, truth)
        stream = torch.cuda.Stream()
        if kind == "ensemble":
            ens = pkg.Ensemble.wrap(live, b, cfg, stream=stream)
            assert ens.stream == stream.cuda_stream
            ens.set_scalars(p0.rdx, p0.rdy, p0.dts, p0.epssm)
            ens.set_cyclic(X)
            ens.set_spec_bdy(True)
            ens.set_guard(1)
            state = S.NativeDomain(b, cfg, np.dtype(dtype).itemsize)
            fields = _views(pkg, torch, state, b, dtype)
            outs = {"moment_" + n: fields[into[n]] for n in R.NAMES}

            def chain(ctx):
                ens.step(3)
                ens.moments("t", "window", want=R.NAMES, out={n: outs["moment_" + n] for n in R.NAMES})

            def finish():
                ens.sync()
                reports.append(ens.guard_report())
            return dict(chain=chain, live=live, truth=truth_dev, stream=stream, outputs=outs, finish=finish, close=ens.close)
        h = ctypes.c_void_p()
        ptrs = (ctypes.c_void_p * len(S.FIELD_NAMES))(*[live[n].data_ptr() for n in S.FIELD_NAMES])
        lib.check(L.amt_domain_wrap(ctypes.byref(h), np.dtype(dtype).itemsize, *cfg.as_ints(), *b.as_tuple(), ptrs, ctypes.c_void_p(stream.cuda_stream)))
        assert int(L.amt_domain_stream(h) or 0) == stream.cuda_stream
        lib.check(L.amt_domain_set_scalars(h, p0.rdx, p0.rdy, p0.dts, p0.epssm))
        lib.check(L.amt_domain_set_cyclic(h, X))
        lib.check(L.amt_domain_set_spec_bdy(h, 1))
        lib.check(L.amt_domain_set_guard(h, 1))

        def chain(ctx):
            lib.check(L.amt_domain_step(h, 3))

        def finish():
            lib.check(L.amt_domain_sync(h))
            rep = lib.GuardReport()
            lib.check(L.amt_domain_guard_report(h, ctypes.byref(rep)))
            reports.append(rep)
        return dict(chain=chain, live=live, truth=truth_dev, stream=stream, finish=finish, close=lambda: L.amt_domain_destroy(h))

    pair = G.run_case(make, gate, torch=torch, record=RECORD, label=f"c/wrap/{kind}")
    _clean(f"wrapped {kind}", pair, [want], truth)
    for rep in reports:
        assert (rep.sweeps_checked, rep.sweep, rep.n_nonfinite) == (3, 0, 0), rep


# ---------------------------------------------------------------------------------------------
# d: the guard under real asynchrony
# ---------------------------------------------------------------------------------------------
def test_guard_finds_a_nan_that_arrives_behind_the_gate(pkg, oracle, torch_mod, gate):
    """The inputs the fill writes behind the gate carry one NaN in t_1 (its footprint: tests/test_special_values_cpu.py).
    amt_domain_step(d, 3) returns AMT_OK while the gate is still running -- the guard does not wait on the host and has found
    nothing yet --, amt_domain_sync then returns AMT_ERR_NONFINITE, the report names sweep 1 and the field, member and offset
    numpy finds in the oracle's first sweep, and the next amt_domain_step returns 7 WITHOUT enqueuing: the arrays hold the same
    bytes before and after that call."""
    torch, S = torch_mod, pkg.synth
    from wrf_model_cuda_sample_amd import lib
    L = pkg.load_library()
    shape = "f64-130x12x9"
    dtype = SHAPES[shape][0]
    b, cfg, p0, made = _truth(pkg, shape, "none", 330)
    truth = _copy(made)
    truth["t_1"][4, 5, 77] = np.nan
    want = _copy(truth)
    _sweep(pkg, oracle, p0, want, 1)
    ext = (b.ims, b.ime, b.jms, b.jme, b.kms, b.kme)
    i0, i1, j0, j1, k0, k1 = pkg.compute_window(cfg, b.ids, b.ide, b.jds, b.jde, b.its, b.ite, b.jts, b.jte, b.kts, b.kte)
    first = None
    for n in ("ww", "t", "mu"):                                    # the guard's order of "first" within a sweep
        st = D.stats(want[n], ext, (i0, i1, k0, k1, j0, j1))
        if st["first_nonfinite"] >= 0:
            first = (S.FIELD_ID[n], st["first_nonfinite"], st["n_nan"] + st["n_inf"])
            break
    assert first is not None
    for _s in range(2):
        _sweep(pkg, oracle, p0, want, 1)
    truth_dev = _to_device(torch, truth)
    seen = []

    def make():
        live = _blank(torch, truth)
        stream = torch.cuda.Stream()
        h = ctypes.c_void_p()
        ptrs = (ctypes.c_void_p * len(S.FIELD_NAMES))(*[live[n].data_ptr() for n in S.FIELD_NAMES])
        lib.check(L.amt_domain_wrap(ctypes.byref(h), np.dtype(dtype).itemsize, *cfg.as_ints(), *b.as_tuple(), ptrs, ctypes.c_void_p(stream.cuda_stream)))
        lib.check(L.amt_domain_set_scalars(h, p0.rdx, p0.rdy, p0.dts, p0.epssm))
        lib.check(L.amt_domain_set_guard(h, 1))
        this = {}
        seen.append(this)

        def chain(ctx):
            this["step"] = int(L.amt_domain_step(h, 3))

        def finish():
            this["sync"] = int(L.amt_domain_sync(h))
            rep = lib.GuardReport()
            lib.check(L.amt_domain_guard_report(h, ctypes.byref(rep)))
            this["report"] = rep
            torch.cuda.synchronize()
            before = {n: live[n].cpu().numpy() for n in S.FIELD_NAMES}
            this["next_step"] = int(L.amt_domain_step(h, 1))
            torch.cuda.synchronize()
            this["moved"] = [n for n in S.FIELD_NAMES if not bits_equal(before[n], live[n].cpu().numpy())]
        return dict(chain=chain, live=live, truth=truth_dev, stream=stream, finish=finish, close=lambda: L.amt_domain_destroy(h))

    pair = G.run_case(make, gate, torch=torch, record=RECORD, label="d/guard")
    _clean("guard", pair, [want], truth, nan_payloads_free=True)
    assert len(seen) >= 2
    for this in seen:
        rep = this["report"]
        assert this["step"] == lib.OK, this
        assert this["sync"] == lib.ERR_NONFINITE, this
        assert (rep.sweep, rep.field, rep.member, rep.offset, rep.n_nonfinite) == (1, first[0], 0, first[1], first[2]), (rep, first)
        assert rep.sweeps_checked == 3, rep
        assert this["next_step"] == lib.ERR_NONFINITE and this["moved"] == [], this


# ---------------------------------------------------------------------------------------------
# e: the host-owned halo exchange, this file as the transport
# ---------------------------------------------------------------------------------------------
E_SEED, E_DIMS = 17, (37, 5, 11)
_UNSPLIT = {}


def _unsplit(pkg, oracle, specified, sweeps):
    """The unsplit oracle run: per sweep the exchanged inputs of seed + s, the oracle and -- specified -- the zone update."""
    key = (specified, sweeps)
    if key not in _UNSPLIT:
        S = pkg.synth
        cfg = pkg.GridConfig(specified=specified)
        full = S.make_patch(S.domain_bounds(*E_DIMS), cfg, dtype=F64, seed=E_SEED)
        for s in range(sweeps):
            if s:
                S.refresh_exchanged_inputs(full, E_SEED, s)
            oracle.advance_mu_t(*full.args())
            if specified:
                SB.spec_bdy_update(full.arrays, full.bounds, _flags(cfg), full.dts)
        _UNSPLIT[key] = full
    return _UNSPLIT[key]


def _external_run(pkg, torch, gate, pi, pj, specified, overlap, need_ms):
    """Two sweeps of pi x pj external steppers, a stream and a gate each.  Sweep 0: behind the gates amt_domain_fill_synthetic,
    amt_domain_poison_halos, step_begin; the gate of a patch must be running right before its halo_wait and over when it
    returns; the messages are carried on a transport stream that waits for nothing but itself; step_end.  Sweep 1: new inputs
    (seed + 1), poisoned halos, no host wait but halo_wait.  Returns (steppers' bounds, results, host seconds, gate runs, flags)."""
    S, P = pkg.synth, pkg.patch
    from wrf_model_cuda_sample_amd import lib
    gb = S.domain_bounds(*E_DIMS)
    gb = gb.replace(ite=gb.ide - 1, jte=gb.jde - 1)
    cfg = pkg.GridConfig(specified=specified)
    steppers, runs = [], []
    for r in range(pi * pj):
        ri, rj = r % pi, r // pi
        pb = S.patch_bounds(gb, ri, rj, pi, pj)
        arrays = {n: torch.empty(pb.shape(n), dtype=torch.float64, device="cuda:0") for n in S.FIELD_NAMES}
        patch = S.Patch(pb, cfg, arrays, global_dims=E_DIMS)
        st = P.ExternalGridStepper(patch, ri, rj, pi, pj, overlap=overlap, stream=torch.cuda.Stream(), spec_bdy=specified)
        st.messages()
        steppers.append(st)
        runs.append(G.Run(torch, arrays, st.stream))
    transport = torch.cuda.Stream()
    torch.cuda.synchronize()
    flags = dict(running_before_wait=[], over_after_wait=[])
    try:
        t0 = time.perf_counter()
        for st, run in zip(steppers, runs):
            run.open(gate, need_ms)
        for sweep in range(2):
            for st in steppers:
                if sweep == 0:
                    b = st.patch.bounds
                    lib.check(st.L.amt_domain_fill_synthetic(st._dom, ctypes.c_uint64(E_SEED), *_fill_args(b, E_DIMS)))
                    lib.check(st.L.amt_domain_poison_halos(st._dom, st._halo_sides))
                else:
                    st.next_substep_inputs(E_SEED, sweep)
                st.begin()
            if sweep == 0:
                host_s = time.perf_counter() - t0
            if sweep == 0 and gate is not None:                    # every patch's gate, before the first host wait
                flags["running_before_wait"] = [not run.gate_run.done.query() for run in runs]
            for st, run in zip(steppers, runs):
                st.halo_wait()
                if sweep == 0 and run.gate_run is not None:
                    flags["over_after_wait"].append(bool(run.gate_run.done.query()))
            with torch.cuda.stream(transport):                     # what an MPI host does between halo_wait and step_end
                for r, st in enumerate(steppers):
                    for m in st.messages():
                        dst = [o for o in steppers[m.peer].messages() if o.peer == r and o.side == P.OPPOSITE_SIDE[m.side]]
                        assert len(dst) == 1
                        dst[0].recv.copy_(m.send, non_blocking=True)
            transport.synchronize()                                # the receives are complete; nothing else is waited for
            for st in steppers:
                st.end()
        for run in runs:
            run.close()
        for run in runs:
            run.read()
        results = [run.settle(st.sync) for st, run in zip(steppers, runs)]
        return [st.patch.bounds for st in steppers], results, host_s, [run.gate_run for run in runs], flags
    finally:
        torch.cuda.synchronize()
        for st in steppers:
            st.close()


@pytest.mark.parametrize("pi,pj,specified,overlap", [(1, 2, False, True), (2, 1, True, True), (2, 1, False, False)],
                         ids=["1x2", "2x1-spec_bdy", "2x1-no-overlap"])
def test_external_halo_exchange_behind_gates(pkg, oracle, torch_mod, gate, pi, pj, specified, overlap):
    """Every owned cell of every output of both patches, at `done` and afterwards, equals the unsplit oracle run; with
    spec_bdy the zone update sat behind the join (it reads t, mu, muts the boundary launches write)."""
    torch, S = torch_mod, pkg.synth
    full = _unsplit(pkg, oracle, specified, 2)
    gb = full.bounds
    label = f"e/external/{pi}x{pj}{'-spec_bdy' if specified else ''}{'' if overlap else '-no-overlap'}"

    def check(bounds, results, which):
        for r, (b, res) in enumerate(zip(bounds, results)):
            own = (slice(b.jts - b.jms, b.jte - b.jms + 1), Ellipsis, slice(b.its - b.ims, b.ite - b.ims + 1))
            for n in S.OUTPUTS:
                want = full.arrays[n][b.jts - gb.jms: b.jte - gb.jms + 1, ..., b.its - gb.ims: b.ite - gb.ims + 1]
                v = G.verdict(res.snaps[0][n][own], want, after=res.after[n][own])
                assert v is None, f"{label}, {which} run, rank {r}, {n}: {v}"

    bounds, results, host_s, _gates, _flags = _external_run(pkg, torch, None, pi, pj, specified, overlap, 0.0)
    check(bounds, results, "ungated")
    need, retried = G.gate_ms_needed(host_s), False
    for attempt in range(2):
        bounds, results, _h, gates, flags = _external_run(pkg, torch, gate, pi, pj, specified, overlap, need)
        if all(flags["running_before_wait"]) and min(g.ms() for g in gates) >= G.gate_ms_needed(host_s):
            break
        assert attempt == 0, f"{label}: {G.GATE_TOO_SHORT}"
        need, retried = need * G.RETRY_FACTOR, True
    RECORD[label] = dict(host_enqueue_ms=round(host_s * 1e3, 3), gate_needed_ms=round(need, 3),
                         gate_measured_ms=[round(g.ms(), 3) for g in gates], retried_4x=retried,
                         gate_running_before_halo_wait=flags["running_before_wait"], gate_over_after_halo_wait=flags["over_after_wait"])
    assert all(flags["over_after_wait"]), f"{label}: halo_wait returned while the gate of its patch was still running"
    check(bounds, results, "gated")
    assert min(g.ms() for g in gates) >= G.MARGIN * host_s * 1e3


def _worker():
    import sys
    path = str(Path(__file__).resolve().parent / "workers")
    if path not in sys.path:
        sys.path.insert(0, path)
    import stream_order_rank
    return stream_order_rank


@pytest.mark.parametrize("overlap", [True, False], ids=["host-waited", "no-overlap"])
@pytest.mark.parametrize("kind", ["slab", "grid"])
def test_loopback_steppers_over_ipc_behind_a_gate(pkg, oracle, torch_mod, gate, kind, overlap):
    """amt_slab_* (rows) and amt_grid_* (all four sides) as their own neighbour over the IPC transport, in this process: the
    host-waited default schedule and AMT_SLAB_NO_OVERLAP.  Three sweeps behind one gate, new exchanged inputs and re-poisoned
    halos in front of each on the domain's stream; the step may wait on the host, so the gate is asked right before the first."""
    label = f"e/loopback-ipc/{kind}/{'host-waited' if overlap else 'no-overlap'}"
    found = _worker().loopback_case(pkg, oracle, torch_mod, gate, kind, overlap, False, RECORD, label)
    assert not found, found[:8]


def test_device_waited_schedule_in_one_fresh_child(pkg, oracle, torch_mod, gate):
    """AMT_IPC_HOST_WAIT=0 is read once per process: ONE child (tests/workers/stream_order_rank.py) runs the same protocol on
    the device-waited schedule, where amt_grid_step / amt_slab_step must return while the gate is still running, and prints its
    verdicts.  A child that ends on a signal or at its time limit ends the test."""
    import os
    import subprocess
    import sys
    torch_mod.cuda.synchronize()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "AMT_TEST_FAULT")}
    env.update(AMT_IPC_HOST_WAIT="0", AMT_IPC_DEVICE_TIMEOUT_S="20")
    cmd = [sys.executable, str(Path(__file__).resolve().parent / "workers" / "stream_order_rank.py")]
    child = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    try:
        out = child.communicate(timeout=150)[0]
    except subprocess.TimeoutExpired:
        child.kill()
        raise AssertionError("the child of the device-waited schedule ran into its time limit:\n" + (child.communicate()[0] or ""))
    lines = [ln for ln in out.splitlines() if ln.startswith("STREAM_ORDER ")]
    assert child.returncode in (0, 1) and len(lines) == 1, f"the child ended with {child.returncode}:\n{out[-3000:]}"
    verdict = json.loads(lines[0][len("STREAM_ORDER "):])
    RECORD.update(verdict["record"])
    assert verdict["findings"] == [] and child.returncode == 0, verdict["findings"][:8]
    assert all(r["gate_running_at_return"] for r in verdict["record"].values()) and len(verdict["record"]) == 2


# ---------------------------------------------------------------------------------------------
# f: independent work at once
# ---------------------------------------------------------------------------------------------
def test_three_handles_behind_three_gates_at_once(pkg, oracle, torch_mod, gate):
    """Two amt_domain handles (fp64 60-level DMA shape, fp32) and a 3-member ensemble with moments, a stream and a gate each,
    all three chains enqueued before anything is waited for.  Every result equals its oracle, and field_stats of t of each
    handle -- asked while the other streams may still be busy -- gives the bytes the same handle gave on the idle device."""
    torch, S = torch_mod, pkg.synth
    from wrf_model_cuda_sample_amd import lib
    L = pkg.load_library()
    T = S.FIELD_ID["t"]
    specs = [("domain", "f64-257x60x33", "none", 1), ("domain", "f32-130x40x9", "specified_periodic_x", 1), ("ensemble", "f64-130x12x9", "none", 3)]
    truths, wants = [], []
    for kind, shape, flag, members in specs:
        b, cfg, p0, truth = _truth(pkg, shape, flag, 340, members)
        want = _copy(truth)
        for _s in range(2):
            _sweep(pkg, oracle, p0, want, members)
        if kind == "ensemble":
            ref = R.moments(want["t"])
            for k, n in enumerate(R.NAMES):
                want["moment_" + n] = ref[n]
        truths.append(truth)
        wants.append(want)
    truth_devs = [_to_device(torch, t) for t in truths]

    def once(g, needs):
        handles, runs, closers = [], [], []
        try:
            for (kind, shape, flag, members), truth in zip(specs, truths):
                b, cfg, p0, _t = _truth(pkg, shape, flag, 340, members)
                dtype = SHAPES[shape][0]
                live = _blank(torch, truth)
                stream = torch.cuda.Stream()
                if kind == "ensemble":
                    ens = pkg.Ensemble.wrap(live, b, cfg, stream=stream)
                    ens.set_scalars(p0.rdx, p0.rdy, p0.dts, p0.epssm)
                    outs = _blank(torch, {"moment_" + n: truth["t"][0] for n in R.NAMES})
                    handles.append(ens)
                    closers.append(ens.close)
                    runs.append(G.Run(torch, live, stream, outputs=outs))
                else:
                    h = ctypes.c_void_p()
                    ptrs = (ctypes.c_void_p * len(S.FIELD_NAMES))(*[live[n].data_ptr() for n in S.FIELD_NAMES])
                    lib.check(L.amt_domain_wrap(ctypes.byref(h), np.dtype(dtype).itemsize, *cfg.as_ints(), *b.as_tuple(), ptrs,
                                                ctypes.c_void_p(stream.cuda_stream)))
                    lib.check(L.amt_domain_set_scalars(h, p0.rdx, p0.rdy, p0.dts, p0.epssm))
                    handles.append(h)
                    closers.append(lambda h=h: L.amt_domain_destroy(h))
                    runs.append(G.Run(torch, live, stream))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for run, need in zip(runs, needs):
                run.open(g, need)
            for (kind, *_rest), h, run, truth_dev in zip(specs, handles, runs, truth_devs):
                G.copy_fill(run.ctx, run.everything, truth_dev)
                if kind == "ensemble":
                    h.step(2)
                    h.moments("t", "memory", want=R.NAMES, out={n: run.everything["moment_" + n] for n in R.NAMES})
                else:
                    lib.check(L.amt_domain_step(h, 2))
            for run in runs:
                run.close()
            host_s = time.perf_counter() - t0
            stats = []
            for (kind, *_rest), h, run in zip(specs, handles, runs):
                run.read()
                if kind == "ensemble":
                    stats.append(b"".join(bytes(r) for r in h.field_stats(T, lib.REGION_WINDOW)))
                else:
                    rec = lib.FieldStats()
                    lib.check(L.amt_domain_field_stats(h, T, lib.REGION_WINDOW, ctypes.byref(rec)))
                    stats.append(bytes(rec))
            results = [run.settle(h.sync if kind == "ensemble" else (lambda h=h: lib.check(L.amt_domain_sync(h))))
                       for (kind, *_rest), h, run in zip(specs, handles, runs)]
            return results, stats, host_s, [run.gate_run for run in runs]
        finally:
            torch.cuda.synchronize()
            for c in closers:
                c()

    idle, idle_stats, host_s, _g = once(None, [0.0] * 3)
    need, retried = G.gate_ms_needed(host_s), False
    for attempt in range(2):
        busy, busy_stats, _h, gates = once(gate, [need] * 3)
        if all(r.running_at_return for r in busy) and min(g.ms() for g in gates) >= G.gate_ms_needed(host_s):
            break
        assert attempt == 0, f"f/three-handles: {G.NOT_ASYNCHRONOUS if not all(r.running_at_return for r in busy) else G.GATE_TOO_SHORT}"
        need, retried = need * G.RETRY_FACTOR, True
    RECORD["f/three-handles"] = dict(host_enqueue_ms=round(host_s * 1e3, 3), gate_needed_ms=round(need, 3),
                                     gate_measured_ms=[round(g.ms(), 3) for g in gates], retried_4x=retried,
                                     gate_running_at_return=[bool(r.running_at_return) for r in busy])
    for (kind, shape, _f, _m), want, truth, r_idle, r_busy in zip(specs, wants, truths, idle, busy):
        for which, res in (("ungated", r_idle), ("gated", r_busy)):
            bad = G.verdicts(res, [want], truth)
            assert not bad, f"{kind} {shape}, {which} run: {bad[:6]}"
    assert busy_stats == idle_stats
    assert min(g.ms() for g in gates) >= G.MARGIN * host_s * 1e3


# ---------------------------------------------------------------------------------------------
# g: the detector detects
# ---------------------------------------------------------------------------------------------
def test_a_sweep_on_an_unordered_stream_is_seen(pkg, oracle, torch_mod, gate):
    """The test's own misuse; the library is as it is.  The chain of (a) with the sweep issued on a SECOND stream that is not
    ordered behind the fill: it reads poison while the gate runs, and its outputs come out as the untouched inputs (the fill
    overwrote its NaNs) or as NaN -- a verdict of the kind "ran ahead".  The streams of a process share a few hardware queues,
    and two streams on one queue serialise by accident; so up to four freshly created streams are tried and at least one has to
    discriminate.  If none does, cases a-f prove nothing on this runtime, and that must not pass silently.  Only NaNs are read
    here: nothing in this control can fault."""
    torch, S = torch_mod, pkg.synth
    members, shape = 3, "f64-130x12x9"
    b, cfg, p0, truth = _truth(pkg, shape, "specified_periodic_x", 270, members)
    want = _copy(truth)
    CR.cyclic_fill(want, b, X, _flags(cfg))
    _sweep(pkg, oracle, p0, want, members)
    SB.spec_bdy_update(want, b, _flags(cfg), p0.dts)
    truth_dev = _to_device(torch, truth)
    tried, found = [], None
    for attempt in range(4):
        live = _blank(torch, truth)
        stream, stray = torch.cuda.Stream(), torch.cuda.Stream()

        def chain(ctx):
            pkg.cyclic_fill(*[live[n] for n in NAMES9], cfg, *b.as_tuple(), axes=X, members=members, stream=ctx.stream)
            pkg.advance_mu_t_ensemble(*S.Patch(b, cfg, live, p0.rdx, p0.rdy, p0.dts, p0.epssm).args(), stream=stray)   # the misuse
            pkg.spec_bdy_update(*[live[n] for n in NAMES5], p0.dts, cfg, *b.as_tuple(), members=members, stream=ctx.stream)

        res = G.run_gated(chain, live, truth_dev, stream, torch=torch, gate=gate, need_ms=2 * G.FLOOR_MS)
        kinds = sorted({kind for _s, n, kind, _d in G.verdicts(res, [want], truth) if n in S.OUTPUTS})
        tried.append(dict(stream=attempt, gate_running_at_return=bool(res.running_at_return), verdicts=kinds))
        if res.running_at_return and any(k in G.RAN_AHEAD for k in kinds):
            found = attempt
            break
    RECORD["g/detector"] = dict(tried=tried, discriminating_stream=found)
    assert found is not None, \
        f"no stream out of four ran ahead of the gated one: every pair shares a hardware queue, cases a-f prove nothing here: {tried}"
