"""Stream-order parity of the native steppers in loopback over the IPC transport (tests/test_gpu_26_stream_order.py, case e).
One rank that is its own neighbour -- amt_slab_* on rows, amt_grid_* on all four sides -- steps three sweeps behind ONE gate
(tests/stream_gate.py): behind the gate amt_domain_fill_synthetic and amt_domain_poison_halos, then per sweep
amt_domain_fill_fields(seed + s), re-poisoned halos, one step and a snapshot, with no host wait of the test's own -- the rule of
tests/multirank.py.  Expected per sweep: the oracle on host arrays with the halo rows and columns copied by hand.

``loopback_case`` is called in-process by the test (AMT_SLAB_NO_OVERLAP and the host-waited default schedule: the step waits on
the host by contract, so the gate must still be running immediately before the first step).  As a program this file is the ONE
fresh child process that runs the device-waited schedule, which the library reads once per process (AMT_IPC_HOST_WAIT=0 in the
child's environment): there amt_slab_step / amt_grid_step must return while the gate is still running.  It prints one JSON line
with its verdicts and the measured gate figures and exits 0 only when every case is clean."""
import ctypes
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (ROOT, ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

SEED = 41
# kind -> (global dims, which patch)
GEOMETRY = {"slab": (200, 12, 60), "grid": (190, 14, 45)}


def _bounds(S, kind):
    gdims = GEOMETRY[kind]
    if kind == "slab":
        return gdims, S.slab_bounds(S.domain_bounds(*gdims, aligned=True), 1, 3)
    return gdims, S.patch_bounds(S.domain_bounds(*gdims), 1, 1, 3, 3, align_elems=32)


_WANTS = {}


def expected(pkg, oracle, kind):
    """(bounds, [name -> array after sweep s]) -- computed once, never changed."""
    if kind not in _WANTS:
        from multirank import loopback_halos_by_hand
        S = pkg.synth
        gdims, b = _bounds(S, kind)
        want = S.make_patch(b, pkg.GridConfig(), dtype=np.float64, seed=SEED, global_dims=gdims)
        per_sweep = []
        for s in range(3):
            if s:
                S.refresh_exchanged_inputs(want, SEED, s)
            loopback_halos_by_hand(pkg, want, rows=True, columns=(kind == "grid"))
            oracle.advance_mu_t(*want.args())
            per_sweep.append({n: want.arrays[n].copy() for n in S.OUTPUTS})
        _WANTS[kind] = (b, per_sweep)
    return _WANTS[kind]


def loopback_case(pkg, oracle, torch, gate, kind, overlap, asynchronous, record=None, label=""):
    """Both runs (ungated, gated) of one loopback stepper; returns the list of findings (empty: clean)."""
    import stream_gate as G
    S, P, lib = pkg.synth, pkg.patch, pkg.lib
    gdims, b = _bounds(S, kind)
    _b, wants = expected(pkg, oracle, kind)
    own = (slice(1, -1), Ellipsis, slice(b.its - b.ims, b.ite - b.ims + 1)) if kind == "grid" else (slice(1, -1), Ellipsis)
    fill_args = (b.ims, b.kms - 1, b.jms, gdims[0] + 2, gdims[1] + 1, gdims[2] + 2)
    synced = []

    def make():
        live = {n: torch.zeros(b.shape(n), dtype=torch.float64, device="cuda:0") for n in S.FIELD_NAMES}
        patch = S.Patch(b, pkg.GridConfig(), live, global_dims=gdims)
        stream = torch.cuda.Stream()
        uid = P.NativeGridStepper.comm_unique_id()
        kw = dict(loopback=True, overlap=overlap, transport="ipc", stream=stream)
        st = P.NativeSlabStepper(patch, 0, 1, uid, **kw) if kind == "slab" else P.NativeGridStepper(patch, 0, 0, 1, 1, uid, **kw)
        st.step(1)                                   # the connection set-up (mappings, staging buffers) happens before the gate
        st.sync()

        def fill(ctx):
            lib.check(st.L.amt_domain_fill_synthetic(st._dom, ctypes.c_uint64(SEED), *fill_args))
            lib.check(st.L.amt_domain_poison_halos(st._dom, st._halo_sides))

        def chain(ctx):
            for s in range(3):
                if s:
                    st.next_substep_inputs(SEED, s)
                elif not asynchronous:
                    ctx.gate_must_be_running(f"amt_{kind}_step")
                st.step(1)
                if s < 2:
                    ctx.snapshot()

        def finish():
            st.sync()
            synced.append(True)
        return dict(chain=chain, live=live, truth=None, stream=stream, fill=fill, snapshots=3, finish=finish, close=st.close)

    pair = G.run_case(make, gate, torch=torch, asynchronous=asynchronous, record=record, label=label)
    found = []
    for which, res in zip(("ungated", "gated"), pair):
        for s in range(3):
            for n in S.OUTPUTS:
                v = G.verdict(res.snaps[s][n][own], wants[s][n][own], after=res.after[n][own] if s == 2 else None)
                if v is not None:
                    found.append(f"{label}, {which} run, sweep {s}, {n}: {v[0]} ({v[1]})")
        u = np.uint64
        for n in res.names:                          # every array, whole: nothing lands after the stepper's sync
            if not np.array_equal(res.snaps[2][n].view(u), res.after[n].view(u)):
                found.append(f"{label}, {which} run, {n}: {G.LATE}")
    if len(synced) < 2:
        found.append(f"{label}: a run did not reach its sync")
    return found


def main():
    import torch
    import __graft_entry__ as g
    import stream_gate as G
    assert os.environ.get("AMT_IPC_HOST_WAIT") == "0", "this program is the device-waited schedule's process"
    pkg, oracle = g.load_package(), g.load_oracle()
    oracle.lib()
    torch.cuda.set_device(0)
    gate = G.Gate(torch, pkg.load_library())
    record, found = {}, []
    for kind in ("grid", "slab"):
        try:
            found += loopback_case(pkg, oracle, torch, gate, kind, True, True, record, f"e/child-device-waited/{kind}")
        except AssertionError as e:                  # the asynchrony check of run_case
            found.append(str(e))
    print("STREAM_ORDER " + json.dumps(dict(findings=found, record=record)), flush=True)
    return 1 if found else 0


if __name__ == "__main__":
    sys.exit(main())
