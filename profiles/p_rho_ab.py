#!/usr/bin/env python3
"""What the pressure diagnosis of an acoustic sub-step costs (include/amt_advance_mu_t.h section 16), in
ONE process on one MI355X, after warm-up, on resident handles (amt_domain_create / amt_ensemble_create), fp64.

  m1s0 / m1s1        one amt_*_p_rho alone, non-hydrostatic, at step 0 and at step 1
  m2s0 / m2s1        the same, hydrostatic (the column recurrence of ph)
  sweep              one sweep (amt_*_step(1)) with the per-sweep setting off, the yardstick of the sub-step it closes
  read(k)            k calls of amt_calib_stream_rate (mode 1: read only) over W * cells contiguous bytes of the handle's t:
                     the box's own read rate over the pass's model bytes
  copy(k)            k / 2 calls of amt_calib_stream_copy (16 bytes per lane; read + write; one more read for an odd k) over
                     the same bytes

`cells` = the tile box ni * nk * nj (times the members).  Model bytes per cell, in elements, the 2-D and 1-D terms left out:
mode 1 reads 6 (alt, t, t_old, c2a, ph, pm1) and writes 3 (al, p, pm1), mode 2 reads 5 and writes 4 (ph too); step 0 reads one
fewer (no pm1).  A sweep moves 11.  Device time between two events on the handle's stream, the arms alternating, median of
`reps`.

  python profiles/p_rho_ab.py [--reps 7] [--cases 1x4096x60x4096,32x128x60x128,1x128x60x128] [--out FILE]
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

ELEMENTS = {"m1s0": 8, "m1s1": 9, "m2s0": 8, "m2s1": 9}
ARMS = {"m1s0": (1, 0), "m1s1": (1, 1), "m2s0": (2, 0), "m2s1": (2, 1)}
SWEEP_ELEMENTS = 11                       # what one sweep moves per cell at 60 levels
FILL = dict(al=0.0, p=0.0, ph=10.0, pm1=0.0, alt=1.0, c2a=10.0, znu=0.5, dnw=-0.016)   # which 0..7 of amt_*_p_rho_ptr


def measure(pkg, torch, members, dims, reps, seed=11):
    from wrf_model_cuda_sample_amd import lib
    S, L = pkg.synth, pkg.load_library()
    ni, nk, nj = dims
    b = S.domain_bounds(ni, nk, nj, aligned=True)
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
        lead = (members,) if ensemble else ()
        scratch = torch.zeros(W * cells // 8, dtype=torch.float64, device="cuda:0")       # the copy yardstick's destination
        sink = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
        h.set_stage(True)                                          # the library's t_old, mu_old, mu_save, mub
        mub = torch.as_tensor(lib.DeviceView(h, h.stage_ptr(3), lead + tuple(b.shape("mu")), "<f8"), device="cuda:0")
        mub.fill_(1.0e5)
        h.stage_prep(1)                                            # t_old, muts
        h.set_p_rho(1, False, 300.0, 0.1)                          # the library's eight arrays
        for which, (name, value) in enumerate(FILL.items()):
            shape = (b.kdim,) if which >= 6 else lead + tuple(b.shape("t"))
            torch.as_tensor(lib.DeviceView(h, h.p_rho_ptr(which), shape, "<f8"), device="cuda:0").fill_(value)
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
                lib.check(L.amt_calib_stream_copy(ctypes.c_void_p(raw), ctypes.c_void_p(scratch.data_ptr()), base, nbytes, 16))
            read(k % 2)

        def arm(which):
            mode, step = ARMS[which]
            h.set_p_rho(mode, False, 300.0, 0.1, *[h.p_rho_ptr(k) for k in range(8)])      # host work, outside the events
            return lambda: h.p_rho(step)

        ms = {}
        note = lambda key, t, r: ms.setdefault(key, []).append(t) if r >= 2 else None
        for r in range(reps + 2):
            for which in ("m1s0", "m2s1", "m1s1", "m2s0"):
                run = arm(which)
                note(which, timed(run), r)
                note(f"read({ELEMENTS[which]})", timed(lambda: read(ELEMENTS[which])), r)
                note(f"copy({ELEMENTS[which]})", timed(lambda: copy(ELEMENTS[which])), r)
                note("sweep", timed(lambda: h.step(1)), r)
        h.sync()
    finally:
        h.close() if ensemble else None
    rec = {"case": f"p_rho {members}x{ni}x{nk}x{nj} f64", "members": members, "cells": cells}
    for key, times in ms.items():
        rec[key] = {"ms": round(statistics.median(times), 4), "repeats": [round(x, 4) for x in times]}
    for which, k in ELEMENTS.items():
        model = k * W * cells
        rec[which].update(model_bytes=model, GBps=round(model / rec[which]["ms"] / 1e6, 1),
                          over_read=round(rec[which]["ms"] / rec[f"read({k})"]["ms"], 3),
                          over_copy=round(rec[which]["ms"] / rec[f"copy({k})"]["ms"], 3),
                          over_sweep=round(rec[which]["ms"] / rec["sweep"]["ms"], 3))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="1x4096x60x4096,32x128x60x128,1x128x60x128")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    torch.cuda.set_device(0)
    lines = []
    for case in args.cases.split(","):
        m, *dims = (int(x) for x in case.split("x"))
        rec = measure(pkg, torch, m, tuple(dims), args.reps)
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(json.dumps(x) for x in lines) + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
