#!/usr/bin/env python3
"""What the bracket of a Runge-Kutta stage costs (include/amt_advance_mu_t.h section 15), in ONE process
on one MI355X, after warm-up, on resident handles (amt_domain_create / amt_ensemble_create), fp64.

  prep1 / prep2      one amt_*_stage_prep alone, at rk_step 1 and at rk_step 2
  finish_h / finish  one amt_*_stage_finish alone, with and without h_diabatic
  sweep              one sweep (amt_*_step(1)), the yardstick of the loop the bracket encloses
  read(k)            k calls of amt_calib_stream_rate (mode 1: read only) over W * cells contiguous bytes of the handle's t:
                     the box's own read rate over the pass's model bytes
  copy(k)            k / 2 calls of amt_calib_stream_copy (16 bytes per lane; read + write; one more read for an odd k) over
                     the same bytes
  mix(k)             the same with amt_calib_stream_rate's mode 0, the copy yardstick profiles/sumflux_ab.py uses

`cells` = the tile box ni * nk * nj (times the members).  Model bytes per cell, in elements, the 2-D terms left out: prep 6 (t
read and three stores at rk_step 1, t and t_old read and two stores after that; ww read, ww_1 stored), finish 6 without and 7
with h_diabatic (t, t_1 [, h_diabatic] read, t stored; ww, ww_1 read, ww stored).  A sweep moves 11.  Device time between two
events on the handle's stream, the arms alternating, median of `reps`.

  python profiles/stage_ab.py [--reps 7] [--cases 1x4096x60x4096,32x128x60x128] [--unaligned] [--out FILE]

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

ELEMENTS = {"prep1": 6, "prep2": 6, "finish_h": 7, "finish": 6}
SWEEP_ELEMENTS = 11                       # what one sweep moves per cell at 60 levels
SUBSTEPS = (1, 2, 4)                      # sub-steps of the three stages of a time step, for the bracket's share of it


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
        lead = (members,) if ensemble else ()
        heat = torch.full(lead + tuple(b.shape("t")), 1e-4, dtype=torch.float64, device="cuda:0")
        scratch = torch.zeros(W * cells // 8, dtype=torch.float64, device="cuda:0")       # the copy yardstick's destination
        sink = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
        h.set_stage(True)                                          # the library's t_old, mu_old, mu_save, mub
        mub = torch.as_tensor(lib.DeviceView(h, h.stage_ptr(3), lead + tuple(b.shape("mu")), "<f8"), device="cuda:0")
        mub.fill_(1.0e5)
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

        def mix(k):
            for _ in range(k // 2):
                lib.check(L.amt_calib_stream_rate(ctypes.c_void_p(raw), ctypes.c_void_p(scratch.data_ptr()), base, nbytes, 0))
            read(k % 2)

        arms = {"prep1": lambda: h.stage_prep(1), "prep2": lambda: h.stage_prep(2),
                "finish_h": lambda: h.stage_finish(3, heat), "finish": lambda: h.stage_finish(3, None)}
        ms = {}
        note = lambda key, t, r: ms.setdefault(key, []).append(t) if r >= 2 else None
        for r in range(reps + 2):
            for which in ("prep1", "finish_h", "prep2", "finish"):         # every prep is followed by a finish, as in a stage
                note(which, timed(arms[which]), r)
                note(f"read({ELEMENTS[which]})", timed(lambda: read(ELEMENTS[which])), r)
                note(f"copy({ELEMENTS[which]})", timed(lambda: copy(ELEMENTS[which])), r)
                note(f"mix({ELEMENTS[which]})", timed(lambda: mix(ELEMENTS[which])), r)
                note("sweep", timed(lambda: h.step(1)), r)
        h.sync()
    finally:
        h.close() if ensemble else None
    rec = {"case": f"stage {members}x{ni}x{nk}x{nj} f64" + ("" if aligned else " unaligned"), "members": members, "cells": cells}
    for key, times in ms.items():
        rec[key] = {"ms": round(statistics.median(times), 4), "repeats": [round(x, 4) for x in times]}
    for which, k in ELEMENTS.items():
        model = k * W * cells
        rec[which].update(model_bytes=model, GBps=round(model / rec[which]["ms"] / 1e6, 1),
                          over_read=round(rec[which]["ms"] / rec[f"read({k})"]["ms"], 3),
                          over_copy=round(rec[which]["ms"] / rec[f"copy({k})"]["ms"], 3),
                          over_mix=round(rec[which]["ms"] / rec[f"mix({k})"]["ms"], 3),
                          over_sweep=round(rec[which]["ms"] / rec["sweep"]["ms"], 3))
    # a time step of three stages: prep at rk_step 1, 2, 3 and three finishes (with h_diabatic), beside 1 + 2 + 4 sweeps
    brackets = rec["prep1"]["ms"] + 2 * rec["prep2"]["ms"] + 3 * rec["finish_h"]["ms"]
    rec["brackets_over_sweeps_of_a_time_step"] = round(brackets / (sum(SUBSTEPS) * rec["sweep"]["ms"]), 3)
    rec["byte_model_brackets_over_sweeps"] = round((3 * 6 + 3 * 7) / (sum(SUBSTEPS) * SWEEP_ELEMENTS), 3)
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
