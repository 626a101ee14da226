#!/usr/bin/env python3
"""A/B of the host-owned halo exchange (include/amt_advance_mu_t.h section 11) on ONE GPU: one j-slab of
8 (default 4096 x 60 x 512 of 4096 x 60 x 4096, fp64, aligned rows) that is its own neighbour above and below.

  A  the IPC transport in loopback, host-waited schedule: amt_slab_step, one sweep per call;
  B  AMT_SLAB_TRANSPORT_EXTERNAL: step_begin, halo_wait, a device-to-device copy of the slab's own messages (what it sends
     below into what it receives from above and the reverse -- this script is the transport), step_end.

Both are timed on the host clock around `sweeps` sweeps and a final sync (B's schedule has a host wait per sweep by design, and
so has A's), `reps` repeats each, alternating.  The pack and the unpack launch are also timed alone (HIP events around `--launches`
back-to-back launches) against their byte model: every message byte is read once and written once.

  python profiles/halo_ab.py [--reps 5] [--sweeps 10] [--dims 4096x60x4096] [--world 8] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--dims", default="4096x60x4096")
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import os
    os.environ.setdefault("AMT_SLAB_TRANSPORT", "ipc")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    S, P = pkg.synth, pkg.patch
    torch.cuda.set_device(0)
    dims = tuple(int(x) for x in args.dims.split("x"))
    rank = args.world // 2 - 1                                   # an inner slab: a neighbour on both sides
    sb = S.slab_bounds(S.domain_bounds(*dims, aligned=True), rank, args.world)
    cfg = pkg.GridConfig()

    def patch():
        p = S.make_patch(sb, cfg, dtype=np.float64, seed=11, global_dims=dims, device="cuda:0")
        torch.cuda.synchronize()
        return p

    pa = patch()
    a = P.NativeSlabStepper(pa, 0, 1, P.NativeSlabStepper.comm_unique_id(), loopback=True, transport="ipc")
    pb = patch()
    b = P.ExternalSlabStepper(pb, rank, args.world)
    below, above = b.messages()
    assert (below.side, above.side) == (S.SIDE_BELOW, S.SIDE_ABOVE)

    def sweeps_a(n):
        for _ in range(n):
            a.step(1)
        a.sync()

    def sweeps_b(n):
        for _ in range(n):
            b.begin()
            b.halo_wait()
            above.recv.copy_(below.send)                         # the transport: the slab is its own neighbour
            below.recv.copy_(above.send)
            torch.cuda.current_stream().synchronize()            # the receives are complete
            b.end()
        b.sync()

    def wall(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(n)
        return (time.perf_counter() - t0) * 1e3 / n

    for fn in (sweeps_a, sweeps_b, sweeps_a, sweeps_b):
        fn(2)
    ta, tb = [], []
    for _ in range(args.reps):
        ta.append(wall(sweeps_a, args.sweeps))
        tb.append(wall(sweeps_b, args.sweeps))
    label = pkg.load_library().amt_march_last_kernel().decode()

    def launch_us(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        call()
        b.sync()
        e0.record(b.stream)
        for _ in range(args.launches):
            call()
        e1.record(b.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.launches

    sent = sum(len(m.send) for m in b.messages())
    received = sum(len(m.recv) for m in b.messages())
    pack_us, unpack_us = launch_us(b.halo_pack), launch_us(b.halo_unpack)
    ni, nk, nj = dims[0], dims[1], sb.jte - sb.jts + 1
    ma, mb = statistics.median(ta), statistics.median(tb)
    rec = {"case": f"slab {rank} of {args.world} of {args.dims} f64, own neighbour above and below",
           "A_ipc_loopback_ms_per_sweep": round(ma, 4), "B_external_ms_per_sweep": round(mb, 4), "B_over_A": round(mb / ma, 4),
           "spread_A": round((max(ta) - min(ta)) / ma, 4), "spread_B": round((max(tb) - min(tb)) / mb, 4),
           "A_repeats": [round(x, 4) for x in ta], "B_repeats": [round(x, 4) for x in tb],
           "message_bytes_sent": sent, "message_bytes_received": received,
           "sent_over_sweep_bytes": round(sent / (8 * ni * nj * (11 * nk + 14)), 6),
           "pack_us": round(pack_us, 2), "pack_model_bytes": 2 * sent, "pack_GBps": round(2 * sent / pack_us / 1e3, 1),
           "unpack_us": round(unpack_us, 2), "unpack_model_bytes": 2 * received, "unpack_GBps": round(2 * received / unpack_us / 1e3, 1),
           "label": label}
    print(json.dumps(rec), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rec) + "\n")
    a.close()
    b.close()


if __name__ == "__main__":
    main()
