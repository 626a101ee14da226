#!/usr/bin/env python3
"""What the flux averages cost (include/amt_advance_mu_t.h section 14), in ONE process on one MI355X,
after warm-up, on resident handles (amt_domain_create / amt_ensemble_create), fp64.

  first / middle / last   one amt_*_sumflux_accumulate alone, as iteration 1, 2 and 3 of n = 3
  off                     one sweep (amt_*_step(1)) with the setting off
  on_first / _middle / _last   one sweep with the setting on: the sweep plus that accumulation, one interval
  read(k)                 k calls of amt_calib_stream_rate (mode 1: read only) over W * cells contiguous bytes of the handle's t:
                          the box's own read rate over the pass's model bytes (k = 6, 9, 12 elements per cell)
  copy(k)                 k / 2 calls of mode 0 (read + write; one more read for an odd k) over the same bytes: the same model
                          bytes as a read / write mix

`cells` = the tile box ni * nk * nj (times the members).  Model bytes per cell, in elements: first 6 (x in, acc out, three
fields), middle 9 (acc in as well), last 12 (the linearisation state as well; the 2-D factors are 1 / nk of a stream and are
left out).  Device time between two events on the handle's stream, the arms alternating, median of `reps`.

  python profiles/sumflux_ab.py [--reps 7] [--cases 1x4096x60x4096,32x128x60x128] [--unaligned] [--out FILE]

--unaligned lays the domain out with domain_bounds(..., aligned=False): rows that start off a 16-byte boundary, so that the
chunks of the pass move element by element.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ELEMENTS = {"first": 6, "middle": 9, "last": 12}
SWEEP_ELEMENTS = 11                       # what one sweep moves per cell at 60 levels


def measure(pkg, torch, members, dims, reps, aligned=True, seed=11):
    from wrf_model_cuda_sample_amd import lib
    S, L = pkg.synth, pkg.load_library()
    ni, nk, nj = dims
    b = S.domain_bounds(ni, nk, nj, aligned=aligned)
    cfg = pkg.GridConfig()
    ensemble = members > 1
    h = pkg.Ensemble(b, members, cfg, np.float64) if ensemble else S.NativeDomain(b, cfg, 8)
    prefix = "amt_ensemble" if ensemble else "amt_domain"
    fn = lambda name: getattr(L, f"{prefix}_{name}")
    try:
        lib.check(fn("fill_synthetic")(h.handle, ctypes.c_uint64(seed), b.ims, b.kms - 1, b.jms, ni + 2, nk + 1, nj + 2))
        h.step(1)
        h.sync()
        W = 8
        cells = members * (b.ite - b.its + 1) * (b.kte - b.kts + 1) * (b.jte - b.jts + 1)
        raw = fn("stream")(h.handle)
        stream = torch.cuda.ExternalStream(raw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        shape = ((members,) if ensemble else ()) + tuple(b.shape("ww"))
        acc = [torch.zeros(shape, dtype=torch.float64, device="cuda:0") for _ in range(3)]
        scratch = torch.zeros(W * cells // 8, dtype=torch.float64, device="cuda:0")       # the copy yardstick's destination
        sink = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        base = ctypes.c_void_p(fn("field_ptr")(h.handle, S.FIELD_ID["t"]))
        nbytes = (W * cells) // 16 * 16

        def timed(run):
            e0.record(stream)
            run()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def read(k):
            for _ in range(k):
                lib.check(L.amt_calib_stream_rate(ctypes.c_void_p(raw), ctypes.c_void_p(sink.data_ptr()), base, nbytes, 1))

        def copy(k):                                           # k elements per cell as k / 2 copies (+ one read for an odd k)
            for _ in range(k // 2):
                lib.check(L.amt_calib_stream_rate(ctypes.c_void_p(raw), ctypes.c_void_p(scratch.data_ptr()), base, nbytes, 0))
            read(k % 2)

        on = lambda: h.set_sumflux(3, *acc)                    # the caller's arrays: off and on again allocates nothing
        ms = {}
        note = lambda key, t, r: ms.setdefault(key, []).append(t) if r >= 2 else None
        for r in range(reps + 2):
            on()
            for which in ("first", "middle", "last"):          # the counter runs 1, 2, 3
                note(which, timed(h.sumflux_accumulate), r)
                note(f"read({ELEMENTS[which]})", timed(lambda: read(ELEMENTS[which])), r)
                note(f"copy({ELEMENTS[which]})", timed(lambda: copy(ELEMENTS[which])), r)
            h.set_sumflux(0)
            note("off", timed(lambda: h.step(1)), r)
            on()
            for which in ("first", "middle", "last"):
                note(f"on_{which}", timed(lambda: h.step(1)), r)
            h.set_sumflux(0)
            note("off", timed(lambda: h.step(1)), r)
        h.sync()
    finally:
        h.close() if ensemble else None
    rec = {"case": f"sumflux {members}x{ni}x{nk}x{nj} f64" + ("" if aligned else " unaligned"), "members": members, "cells": cells}
    for key, times in ms.items():
        rec[key] = {"ms": round(statistics.median(times), 4), "repeats": [round(x, 4) for x in times]}
    for which, k in ELEMENTS.items():
        model = k * W * cells
        rec[which].update(model_bytes=model, GBps=round(model / rec[which]["ms"] / 1e6, 1),
                          over_read=round(rec[which]["ms"] / rec[f"read({k})"]["ms"], 3),
                          over_copy=round(rec[which]["ms"] / rec[f"copy({k})"]["ms"], 3))
        rec[f"on_{which}"].update(added_ms=round(rec[f"on_{which}"]["ms"] - rec["off"]["ms"], 4),
                                  over_off=round(rec[f"on_{which}"]["ms"] / rec["off"]["ms"], 3))
    rec["loop_of_3_on_over_off"] = round(sum(rec[f"on_{w}"]["ms"] for w in ELEMENTS) / (3 * rec["off"]["ms"]), 3)
    rec["byte_model_on_over_off"] = round(1 + sum(ELEMENTS.values()) / 3 / SWEEP_ELEMENTS, 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="1x4096x60x4096,32x128x60x128")
    ap.add_argument("--unaligned", action="store_true", help="rows off the 16-byte boundaries: the element-by-element chunks")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    torch.cuda.set_device(0)
    lines = []
    for case in args.cases.split(","):
        m, *dims = (int(x) for x in case.split("x"))
        rec = measure(pkg, torch, m, tuple(dims), args.reps, aligned=not args.unaligned)
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(json.dumps(x) for x in lines) + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
