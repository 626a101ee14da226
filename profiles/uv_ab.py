#!/usr/bin/env python3
"""What the momentum update of an acoustic sub-step costs (include/amt_advance_mu_t.h section 17), in
ONE process on one MI355X, after warm-up, on resident handles (amt_domain_create / amt_ensemble_create), fp64.  The pass has no
handle setting: the pointer-level call runs on the handle's stream over the handle's fields and the pressure diagnosis's arrays
(ten distinct 3-D inputs, so no array is found in cache because another name has just read it).

  uv_h / uv_nh       one amt_advance_uv_device_f64 alone, hydrostatic / non-hydrostatic
  p_rho              one amt_*_p_rho, mode 1, step 1: the sibling pass
  sweep              one sweep (amt_*_step(1)), the yardstick of the sub-step the pass opens
  read(k) / copy(k)  the box's own read rate / copy rate over the pass's model bytes (amt_calib_stream_rate, _copy)

`cells` = the tile box ni * nk * nj (times the members).  Model bytes per cell, in elements, the 2-D and 1-D terms, the group
overlap and the u part's single elements left out: the two parts move 18 hydrostatic, 20 non-hydrostatic (DESIGN.md section
7.12).  Device time between two events on the handle's stream, the arms alternating, median of `reps`.

  python profiles/uv_ab.py [--reps 7] [--cases 1x4096x60x4096,32x128x60x128,1x128x60x128] [--out FILE]
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

ELEMENTS = {"uv_h": 18, "uv_nh": 20}
ARMS = {"uv_h": 0, "uv_nh": 1}
SCALARS = (1.0e-3, 1.25e-3, 2.0, 1.5, -0.75, 0.25, 0.01)   # rdx rdy dts cf1 cf2 cf3 emdiv
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
        cells = members * (b.ite - b.its + 1) * (b.kte - b.kts) * (b.jte - b.jts + 1)       # the pass has cells on kts..kte-1
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

        field = lambda name: int(fn("field_ptr")(h.handle, S.FIELD_ID[name]))
        # u v | ru_tend rv_tend p pb ph php alt al | mu muu muv mudf | cqu cqv | msfux msfuy msfvx msfvx_inv msfvy | fnm fnp rdnw
        arrays = [field("u"), field("v"), field("ft"), field("t_ave"), h.p_rho_ptr(1), h.p_rho_ptr(5), h.p_rho_ptr(2), h.p_rho_ptr(3),
                  h.p_rho_ptr(4), h.p_rho_ptr(0), field("mu"), field("muu"), field("muv"), field("mudf"), field("t_1"), field("ww_1"),
                  field("msftx"), field("msfuy"), field("msfty"), field("msfvx_inv"), field("msfty"), field("fnm"), field("fnp"),
                  field("rdnw")]

        def arm(which):
            nh = ARMS[which]
            return lambda: pkg.advance_uv(nh, *arrays, *SCALARS, False, False, False, *b.as_tuple(), members=members, stream=stream,
                                          dtype=torch.float64)

        ms = {}
        note = lambda key, t, r: ms.setdefault(key, []).append(t) if r >= 2 else None
        for r in range(reps + 2):
            for which in ("uv_h", "uv_nh"):
                run = arm(which)
                note(which, timed(run), r)
                note("p_rho", timed(lambda: h.p_rho(1)), r)
                note(f"read({ELEMENTS[which]})", timed(lambda: read(ELEMENTS[which])), r)
                note(f"copy({ELEMENTS[which]})", timed(lambda: copy(ELEMENTS[which])), r)
                note("sweep", timed(lambda: h.step(1)), r)
        h.sync()
    finally:
        h.close()
    rec = {"case": f"advance_uv {members}x{ni}x{nk}x{nj} f64", "members": members, "cells": cells}
    for key, times in ms.items():
        rec[key] = {"ms": round(statistics.median(times), 4), "repeats": [round(x, 4) for x in times]}
    for which, k in ELEMENTS.items():
        model = k * W * cells
        rec[which].update(model_bytes=model, GBps=round(model / rec[which]["ms"] / 1e6, 1),
                          over_read=round(rec[which]["ms"] / rec[f"read({k})"]["ms"], 3),
                          over_copy=round(rec[which]["ms"] / rec[f"copy({k})"]["ms"], 3),
                          over_sweep=round(rec[which]["ms"] / rec["sweep"]["ms"], 3),
                          over_p_rho=round(rec[which]["ms"] / rec["p_rho"]["ms"], 3))
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
