"""TEST INFRASTRUCTURE: stream-order parity.  Every other GPU test calls the library on an idle device and synchronises before it
looks: a 20 us kernel has finished before the host issues the next call, so a launch on the wrong stream, a missing fork or
join between the library's streams, a host read of a page-locked record before its stream has written it, or a hidden
device-wide synchronisation all pass.  Here the library enqueues behind a GATE -- a bounded amount of device work that is
still running while the host enqueues -- on state that holds poison until the work behind the gate fills it.

The gate.  Repeated ``amt_calib_stream_copy`` of GATE_BYTES on one stream, public calls only.  It always ends by itself: no
kernel waits for a host flag, so an assertion that fires in between leaves nothing waiting.  ``Gate.calibrate`` times one
repetition with two events on an idle stream.  Sizing rule (``gate_ms_needed``, ``repetitions``): a gate lasts at least MARGIN
x the host time of the enqueue chain it protects (measured with time.perf_counter in the ungated warm-up run of the same
chain; the margin is there because a host thread on a shared machine can be descheduled for milliseconds) and at least
FLOOR_MS.  HEADROOM covers the noise of the calibration; the gate's real device time is measured by two events around it and
reported.  The only question ever asked of a gate is ``done.query()``.

The protocol (``run_gated``):
 1. every tensor, handle and workspace exists before the gate (``truth``: the real inputs on the device; ``live``: what the
    library is given; the snapshots); ``torch.cuda.synchronize()``.  Nothing allocates inside the gated region.
 2. ``live`` and the snapshots hold quiet NaNs whose payload names the array (``poison_bits``); synchronise.
 3. on ONE stream, with no host wait: the gate; the fill (``live[f].copy_(truth[f])``, or the case's own); the library chain;
    ``snap[f].copy_(live[f])`` for every array and every output of the chain; an event ``done``.
 4. chains documented as asynchronous: ``gate.done.query()`` is False when the last enqueue has returned -- otherwise the run
    proves nothing and ``run_case`` repeats it once behind a gate RETRY_FACTOR times as long, then fails.  Chains that wait on
    the host by contract ask the same question immediately before the waiting call (``Context.gate_must_be_running``).  A gate
    whose measured time fell short of the sizing rule (the calibration is one sample) is repeated the same way.
 5. ``done.synchronize()``; the snapshots are compared with the oracle run on ``truth`` (``verdict``).
 6. the handle is synchronised, then the device; ``live`` must still equal the snapshot: a difference is work that landed
    after the stream said it was done -- a missing join.

``verdict`` names what went wrong with an array: it holds its poison (never written), it holds ``truth`` (the chain ran
before the fill), it has NaN where the oracle is finite (the chain read poison: it ran ahead of the gate), or it changed after
``done``.  tests/test_stream_gate_cpu.py plants each of these by hand.  Plain numpy and torch; no HIP code of its own.
"""
from __future__ import annotations

import ctypes
import math
import time

import numpy as np

MARGIN = 20.0            # gate time / host time of the chain behind it
FLOOR_MS = 50.0          # and never shorter than this
HEADROOM = 1.25          # repetitions are chosen for this much more than needed: the calibration is one sample
RETRY_FACTOR = 4         # the one retry of an asynchrony check that found its gate finished
GATE_BYTES = 256 << 20   # one repetition copies this much (reads it and writes it)

POISON, TRUTH, NAN, LATE, WRONG = ("holds its poison", "holds truth", "NaN where the oracle is finite", "changed after done",
                                   "differs from the oracle")
RAN_AHEAD = (TRUTH, NAN)          # the two faces of work that did not wait for what was enqueued in front of it


# ---------------------------------------------------------------------------------------------
# arithmetic and numpy: no device needed
# ---------------------------------------------------------------------------------------------
def gate_ms_needed(host_s: float) -> float:
    """Device time a gate must last to protect a chain whose enqueue took ``host_s`` seconds of host time."""
    if not host_s >= 0.0:
        raise ValueError(f"host time {host_s!r}")
    return max(FLOOR_MS, MARGIN * host_s * 1e3)


def repetitions(need_ms: float, ms_per_repetition: float) -> int:
    """Repetitions of the calibrated unit of work for a gate of ``need_ms`` (with HEADROOM); at least one."""
    if not ms_per_repetition > 0.0:
        raise ValueError(f"calibration gave {ms_per_repetition!r} ms per repetition")
    return max(1, int(math.ceil(need_ms * HEADROOM / ms_per_repetition)))


def _uint(dtype):
    return np.uint64 if np.dtype(dtype).itemsize == 8 else np.uint32


def poison_bits(dtype, index: int, snapshot: bool = False) -> int:
    """Bit pattern of the quiet NaN array number ``index`` of a case holds before anything writes it: payload 2 index + 1 in what
    the library is given, 2 index + 2 in its snapshot (as tests/packed_state.py numbers its guards: a copied or shifted
    array cannot pass for another)."""
    payload = 2 * int(index) + (2 if snapshot else 1)
    if np.dtype(dtype).itemsize == 8:
        return 0x7FF8000000000000 | payload
    if payload >= 1 << 22:
        raise ValueError("a float32 payload has 22 bits")
    return 0x7FC00000 | payload


def poisoned(shape, dtype, index: int, snapshot: bool = False):
    """A numpy array of poison (the CPU test's stand-in for a device array nobody wrote)."""
    return np.full(shape, poison_bits(dtype, index, snapshot), dtype=_uint(dtype)).view(dtype)


def verdict(snap, want, *, truth=None, index=None, after=None, nan_payloads_free=False):
    """None when ``snap`` (the snapshot taken on the stream) has the bits of ``want`` (the oracle's) and ``after`` (the same
    array once everything was synchronised; None: not looked at) still has the snapshot's.  Otherwise (kind, detail) with kind
    POISON: every cell still holds poison number ``index`` (the live array's or the snapshot's own);  TRUTH: the array equals
    ``truth`` although the oracle changed it;  NAN: NaN in cells where the oracle is finite;  WRONG: any other difference;
    LATE: right at ``done``, different afterwards.  ``nan_payloads_free``: a NaN equals any NaN (cases that plant one:
    special_values.same_up_to_nan_payload)."""
    snap, want = np.ascontiguousarray(snap), np.ascontiguousarray(want)
    if snap.shape != want.shape or snap.dtype != want.dtype:
        return WRONG, f"shape / dtype {snap.shape} {snap.dtype}, the oracle has {want.shape} {want.dtype}"
    u = _uint(snap.dtype)
    sb, wb = snap.view(u), want.view(u)
    bad = sb != wb
    if nan_payloads_free:
        bad &= ~(np.isnan(snap) & np.isnan(want))
    if not bad.any():
        if after is not None:
            moved = np.ascontiguousarray(after).view(u) != sb
            if moved.any():
                at = tuple(int(x) for x in np.argwhere(moved)[0])
                return LATE, f"{int(moved.sum())} cells changed after the stream reported done, first at {at}"
        return None
    if index is not None:
        mine, its = u(poison_bits(snap.dtype, index)), u(poison_bits(snap.dtype, index, snapshot=True))
        if ((sb == mine) | (sb == its)).all():
            return POISON, "the snapshot was never written" if (sb == its).all() else "the array was never written"
    if truth is not None:
        tb = np.ascontiguousarray(truth).view(u)
        if tb.shape == sb.shape and np.array_equal(tb, sb):
            return TRUTH, f"the inputs as filled, {int(bad.sum())} cells the oracle changed are unchanged: the work ran before the fill"
    nan = np.isnan(snap) & np.isfinite(want)
    at = tuple(int(x) for x in np.argwhere(nan if nan.any() else bad)[0])
    if nan.any():
        return NAN, f"{int(nan.sum())} cells, first at {at} (bits {hex(int(sb[at]))}): the work read poison"
    return WRONG, f"{int(bad.sum())} cells, first at {at}: {hex(int(sb[at]))} for {hex(int(wb[at]))}"


# ---------------------------------------------------------------------------------------------
# the gate
# ---------------------------------------------------------------------------------------------
class GateRun:
    """One enqueued gate: ``done`` is the event right behind it, ``ms()`` its measured device time (after it has ended)."""

    def __init__(self, start, done, reps, need_ms):
        self.start, self.done, self.reps, self.need_ms = start, done, reps, need_ms

    def ms(self) -> float:
        self.done.synchronize()
        return float(self.start.elapsed_time(self.done))


class Gate:
    """Owns the two buffers the gate's copies move and the calibration of one repetition.  One per session."""

    def __init__(self, torch, library, nbytes: int = GATE_BYTES):
        self.torch, self.L, self.nbytes = torch, library, int(nbytes)
        self.src = torch.zeros(self.nbytes // 8, dtype=torch.float64, device="cuda")
        self.dst = torch.empty_like(self.src)
        torch.cuda.synchronize()
        self.ms_per_repetition = self.calibrate()

    def _repeat(self, stream, reps: int) -> None:
        handle = ctypes.c_void_p(stream.cuda_stream)
        dst, src = ctypes.c_void_p(self.dst.data_ptr()), ctypes.c_void_p(self.src.data_ptr())
        fn, n = self.L.amt_calib_stream_copy, ctypes.c_size_t(self.nbytes)
        for _ in range(reps):
            status = fn(handle, dst, src, n, 16)
            if status:
                raise RuntimeError(f"amt_calib_stream_copy returned {status}")

    def calibrate(self, reps: int = 16) -> float:
        """ms of one repetition: ``reps`` of them on an idle stream between two events (two more in front as a warm-up)."""
        torch = self.torch
        stream = torch.cuda.Stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        self._repeat(stream, 2)
        e0.record(stream)
        self._repeat(stream, reps)
        e1.record(stream)
        e1.synchronize()
        return float(e0.elapsed_time(e1)) / reps

    def enqueue(self, stream, need_ms: float) -> GateRun:
        torch = self.torch
        reps = repetitions(need_ms, self.ms_per_repetition)
        start, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        self._repeat(stream, reps)
        done.record(stream)
        return GateRun(start, done, reps, need_ms)


# ---------------------------------------------------------------------------------------------
# the protocol
# ---------------------------------------------------------------------------------------------
def _fill_bits(torch, tensor, bits: int) -> None:
    as_int = tensor.view(torch.int64 if tensor.element_size() == 8 else torch.int32)
    as_int.fill_(bits if bits < (1 << (8 * tensor.element_size() - 1)) else bits - (1 << (8 * tensor.element_size())))


class Context:
    """What a chain sees: the stream to enqueue on, ``snapshot()`` (one more copy of every array, behind what was enqueued so
    far) and ``gate_must_be_running`` for the calls that wait on the host by contract."""

    def __init__(self, torch, stream, live, snaps, gate_run):
        self.torch, self.stream, self.live, self._snaps, self.gate_run = torch, stream, live, snaps, gate_run
        self.taken = 0
        self.asked = 0

    @property
    def handle(self) -> int:
        return self.stream.cuda_stream

    def snapshot(self) -> None:
        snap = self._snaps[self.taken]
        self.taken += 1
        with self.torch.cuda.stream(self.stream):
            for name, t in self.live.items():
                snap[name].copy_(t, non_blocking=True)

    def gate_must_be_running(self, what: str) -> None:
        """Immediately before a call that waits on the host: the work it waits for is still behind a running gate."""
        self.asked += 1
        if self.gate_run is not None and self.gate_run.done.query():
            raise GateFinished(what)


class GateFinished(Exception):
    """The gate had ended where it had to be running: the run proves nothing about ordering."""


class Result:
    """``snaps``: one dict name -> numpy array per snapshot;  ``after``: the arrays once handle and device were synchronised;
    ``host_s``: host time of the enqueue (fill, chain, snapshots);  ``gate_ms`` / ``gate_need_ms`` / ``gate_reps`` (None:
    ungated);  ``running_at_return``: gate.done.query() was False when the last enqueue returned;  ``value``: what the chain
    returned."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class Run:
    """The protocol in phases, for cases that keep several streams busy at once (one Run per stream): construct every Run
    (steps 1, 2: the snapshots are allocated, everything is poisoned), ``torch.cuda.synchronize()``, then per Run ``open``
    (the gate), the fill and the chain through ``run.ctx``, ``close`` (the last snapshots, ``done``); then ``read`` (step 5) of
    every Run, and ``settle`` (step 6) of every Run.  ``run_gated`` is the one-stream sequence of these."""

    def __init__(self, torch, live, stream, *, outputs=None, snapshots=1):
        self.torch, self.stream = torch, stream
        self.everything = dict(live)
        self.everything.update(outputs or {})
        self.names = list(self.everything)
        self.snaps = [{n: torch.empty_like(t) for n, t in self.everything.items()} for _ in range(snapshots)]
        for k, n in enumerate(self.names):
            dt = _np_dtype(torch, self.everything[n])
            _fill_bits(torch, self.everything[n], poison_bits(dt, k))
            for snap in self.snaps:
                _fill_bits(torch, snap[n], poison_bits(dt, k, snapshot=True))
        self.done = torch.cuda.Event()
        self.gate_run = self.ctx = None

    def open(self, gate=None, need_ms=0.0):
        self.gate_run = gate.enqueue(self.stream, need_ms) if gate is not None else None
        self.ctx = Context(self.torch, self.stream, self.everything, self.snaps, self.gate_run)
        self.t0 = time.perf_counter()
        return self.ctx

    def close(self):
        while self.ctx.taken < len(self.snaps):
            self.ctx.snapshot()
        self.done.record(self.stream)
        self.host_s = time.perf_counter() - self.t0
        # 4: was the gate still running when the last enqueue returned?
        self.running = (not self.gate_run.done.query()) if self.gate_run is not None else None

    def read(self):
        """5: wait for ``done`` alone and read the snapshots."""
        self.done.synchronize()
        self.got = [{n: snap[n].cpu().numpy() for n in self.names} for snap in self.snaps]

    def settle(self, finish=None, value=None):
        """6: the handle, then the device; what ``live`` holds now."""
        if finish is not None:
            finish()
        self.torch.cuda.synchronize()
        after = {n: self.everything[n].cpu().numpy() for n in self.names}
        g = self.gate_run
        return Result(snaps=self.got, after=after, names=self.names, host_s=self.host_s, running_at_return=self.running,
                      value=value, asked=self.ctx.asked, gate_ms=g.ms() if g else None, gate_need_ms=g.need_ms if g else None,
                      gate_reps=g.reps if g else None)


def run_gated(chain, live, truth, stream, *, torch, gate=None, need_ms=0.0, fill=None, outputs=None, snapshots=1, finish=None):
    """One run of the protocol.  ``live``: name -> device tensor the library is given;  ``truth``: name -> device tensor of the
    same shape that the default fill copies into ``live`` behind the gate (``fill(ctx)`` replaces the copies);  ``outputs``:
    further name -> device tensor the chain writes, poisoned and snapshotted with the rest;  ``chain(ctx)`` enqueues the library
    calls on ``ctx.stream`` and may call ``ctx.snapshot()`` up to ``snapshots - 1`` times itself -- the last snapshot is taken
    behind it;  ``gate``: a Gate, None for the ungated warm-up run;  ``finish()`` synchronises the case's handles in step 6."""
    run = Run(torch, live, stream, outputs=outputs, snapshots=snapshots)          # 1, 2: allocate, poison, synchronise
    torch.cuda.synchronize()
    ctx = run.open(gate, need_ms)                                                 # 3: gate, fill, chain, snapshot, `done`
    if fill is not None:
        fill(ctx)
    else:
        copy_fill(ctx, live, truth)
    value = chain(ctx)
    run.close()
    run.read()
    return run.settle(finish, value)


def copy_fill(ctx, live, truth) -> None:
    """The default fill: ``live[f].copy_(truth[f])`` for every array of ``truth``, on the stream, no host wait."""
    with ctx.torch.cuda.stream(ctx.stream):
        for n, t in truth.items():
            live[n].copy_(t, non_blocking=True)


def _np_dtype(torch, tensor):
    return np.float64 if tensor.dtype == torch.float64 else np.float32


NOT_ASYNCHRONOUS = "a call documented as asynchronous waited for the device"
GATE_TOO_SHORT = "the gate ended before the work it protects was enqueued, or sooner than its sizing rule asks"


def run_case(make, gate, *, torch, asynchronous=True, record=None, label=""):
    """The two runs of a case, each on FRESH state: ``make()`` returns the keyword arguments of ``run_gated`` (chain, live,
    truth, stream, and the optional ones) plus an optional ``close`` to call afterwards.  First ungated -- the warm-up and the
    timing run, which must already equal the oracle --, then behind a gate sized from the ungated run's host time.
    ``asynchronous``: the chain must return while its gate runs; one retry behind a gate RETRY_FACTOR times as long, then the
    test fails with NOT_ASYNCHRONOUS.  Host-waiting chains (``asynchronous=False``) must ask ``ctx.gate_must_be_running``
    before their waiting call; the same retry applies.  Returns (ungated Result, gated Result); ``record[label]`` gets the
    measured figures."""
    def once(g, need):
        kw = dict(make())
        close = kw.pop("close", None)
        try:
            return run_gated(torch=torch, gate=g, need_ms=need, **kw)
        finally:
            torch.cuda.synchronize()          # (a chain that raised has left work enqueued)
            if close is not None:
                close()

    warm = once(None, 0.0)
    need = gate_ms_needed(warm.host_s)
    retried = False
    for attempt in range(2):
        try:
            gated = once(gate, need)
            ok = gated.running_at_return if asynchronous else gated.asked > 0
            ok = ok and gated.gate_ms >= gate_ms_needed(warm.host_s)      # a gate that ran faster than its calibration: too short
            if not asynchronous and gated.asked == 0:
                raise AssertionError(f"{label}: a host-waiting chain never asked whether its gate was running")
        except GateFinished:
            gated, ok = None, False
        if ok:
            break
        if attempt == 1:
            message = NOT_ASYNCHRONOUS if asynchronous and gated is not None and not gated.running_at_return else GATE_TOO_SHORT
            raise AssertionError(f"{label}: {message} (gates of {need / RETRY_FACTOR:.0f} ms, then {need:.0f} ms)")
        retried, need = True, need * RETRY_FACTOR
    if record is not None:
        record[label] = dict(host_enqueue_ms=round(warm.host_s * 1e3, 3), gated_host_enqueue_ms=round(gated.host_s * 1e3, 3),
                             gate_needed_ms=round(gated.gate_need_ms, 3), gate_measured_ms=round(gated.gate_ms, 3),
                             gate_repetitions=gated.gate_reps, gate_over_host=round(gated.gate_ms / max(warm.host_s * 1e3, 1e-6), 1),
                             retried_4x=retried, asynchronous=bool(asynchronous),
                             gate_running_at_return=bool(gated.running_at_return))
    return warm, gated


def verdicts(result, wants, truth=None, *, nan_payloads_free=False):
    """[(snapshot number, array, kind, detail)] of every array of every snapshot of ``result`` that is not clean; ``wants``:
    one dict name -> numpy array (the oracle's) per snapshot;  ``truth``: name -> numpy array as filled (may be None).  The
    LAST snapshot is also held against ``result.after``."""
    out = []
    assert len(wants) == len(result.snaps), (len(wants), len(result.snaps))
    for s, (snap, want) in enumerate(zip(result.snaps, wants)):
        last = s == len(wants) - 1
        for k, n in enumerate(result.names):
            v = verdict(snap[n], want[n], truth=None if truth is None or n not in truth else truth[n], index=k,
                        after=result.after[n] if last else None, nan_payloads_free=nan_payloads_free)
            if v is not None:
                out.append((s, n, v[0], v[1]))
    return out
