#!/usr/bin/env python3
"""What the statistics pass and the non-finite guard cost (include/amt_advance_mu_t.h section 10), in
ONE process, after warm-up:

  stats     amt_domain_field_stats(T, AMT_REGION_MEMORY) on one amt_domain_create handle (default 4096 x 60 x 4096 fp64): wall
            time of the synchronous call, median of `reps`, beside the time amt_calib_stream_rate (mode 1: read only) needs
            for the SAME bytes of the same array -- the box's own read rate, not a data-sheet figure.
  guard     sweep time through the handle's own *_step_timed with the guard off (A), every = 1 (B1) and every = 4 (B4),
            alternating on the SAME handle; `model` = (2 NK + 1) / (11 NK + 14), the guard's share of the sweep's bytes.
  ensemble  the same three for one amt_ensemble_create handle (default 32 members of 128 x 60 x 128 fp64).

  python profiles/diag_ab.py [--reps 5] [--sweeps 8] [--domain 4096x60x4096] [--ensemble 32x128x60x128] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

T, MEMORY = 13, 1


def interleave(step_timed, set_guard, reps, sweeps):
    for every in (0, 1, 4, 0):
        set_guard(every)
        step_timed(4)
    out = {0: [], 1: [], 4: []}
    for _ in range(reps):
        for every in (0, 1, 4):
            set_guard(every)
            out[every].append(step_timed(sweeps) / sweeps)
    set_guard(0)
    return out


def guard_record(what, t, nk, label):
    a, b1, b4 = (statistics.median(t[k]) for k in (0, 1, 4))
    mdl = (2 * nk + 1) / (11 * nk + 14)
    return {"case": what, "off_ms_per_sweep": round(a, 5), "every1_ms_per_sweep": round(b1, 5), "every4_ms_per_sweep": round(b4, 5),
            "every1_over_off": round(b1 / a, 5), "every4_over_off": round(b4 / a, 5), "model_every1": round(1 + mdl, 5),
            "model_every4": round(1 + mdl / 4, 5), "spread_off": round((max(t[0]) - min(t[0])) / a, 5),
            "off_repeats": [round(x, 5) for x in t[0]], "every1_repeats": [round(x, 5) for x in t[1]],
            "every4_repeats": [round(x, 5) for x in t[4]], "label": label}


def measure_domain(pkg, torch, dims, reps, sweeps, seed=11):
    from wrf_model_cuda_sample_amd import lib
    S, L = pkg.synth, pkg.load_library()
    ni, nk, nj = dims
    b = S.domain_bounds(ni, nk, nj, aligned=True).replace(ite=ni, jte=nj)
    patch = S.make_patch(b, pkg.GridConfig(), dtype=np.float64, seed=seed, global_dims=dims, device="cuda:0", native_domain=True)
    torch.cuda.synchronize()
    dom = patch.owner
    # the statistics pass against the read-only stream over the same bytes of the same array, alternating
    t_arr = patch.arrays["t"]
    nbytes = t_arr.numel() * t_arr.element_size()
    sink = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stats_ms, read_ms, rec = [], [], None
    for k in range(reps + 2):
        t0 = time.perf_counter()
        rec = dom.field_stats(T, MEMORY)
        dt = (time.perf_counter() - t0) * 1e3
        e0.record(stream)
        lib.check(L.amt_calib_stream_rate(ctypes.c_void_p(stream.cuda_stream), ctypes.c_void_p(sink.data_ptr()),
                                          ctypes.c_void_p(t_arr.data_ptr()), nbytes, 1))
        e1.record(stream)
        e1.synchronize()
        if k >= 2:
            stats_ms.append(dt)
            read_ms.append(e0.elapsed_time(e1))
    s, r = statistics.median(stats_ms), statistics.median(read_ms)
    stats = {"case": f"stats T memory {ni}x{nk}x{nj} f64", "bytes": nbytes, "count": rec.count, "stats_ms": round(s, 4),
             "stats_GBps": round(nbytes / s / 1e6, 1), "box_read_ms": round(r, 4), "box_read_GBps": round(nbytes / r / 1e6, 1),
             "fraction_of_box_read_rate": round(r / s, 4), "stats_repeats": [round(x, 4) for x in stats_ms],
             "read_repeats": [round(x, 4) for x in read_ms], "n_nan": rec.n_nan, "n_inf": rec.n_inf}
    # runs that start on a 16-byte boundary (16-byte loads) against runs that start one element off it (single-element loads):
    # the same rows of the same array, two elements narrower than the memory row
    ext = (b.ims, b.ime, b.jms, b.jme, b.kms, b.kme)
    runs = {}
    for label, i0 in (("aligned", b.ims + 2), ("off_by_one", b.ims + 1)):
        box = (i0, i0 + b.idim - 3, b.kms, b.kme, b.jms, b.jme)
        ms = []
        for k in range(reps + 1):
            t0 = time.perf_counter()
            r1 = pkg.diag.field_stats(t_arr, extents=ext, box=box)[0]
            if k:
                ms.append((time.perf_counter() - t0) * 1e3)
        m = statistics.median(ms)
        runs[label] = {"first_byte_mod_16": (t_arr.data_ptr() + (i0 - b.ims) * t_arr.element_size()) % 16,
                       "row_bytes_mod_16": b.idim * t_arr.element_size() % 16, "count": r1.count, "ms": round(m, 4),
                       "GBps": round(r1.count * t_arr.element_size() / m / 1e6, 1), "repeats": [round(x, 4) for x in ms]}
    stats["row_runs"] = runs
    t = interleave(dom.step_timed, dom.set_guard, reps, sweeps)
    return stats, guard_record(f"guard domain {ni}x{nk}x{nj} f64", t, nk, L.amt_march_last_kernel().decode())


def measure_ensemble(pkg, torch, members, dims, reps, sweeps, seed=11):
    S, L = pkg.synth, pkg.load_library()
    ni, nk, nj = dims
    b = S.domain_bounds(ni, nk, nj, aligned=True).replace(ite=ni, jte=nj)
    ens = pkg.Ensemble(b, members, pkg.GridConfig(), np.float64)
    try:
        ens.fill_synthetic(seed, global_dims=dims)
        ens.sync()
        t = interleave(ens.step_timed, ens.set_guard, reps, sweeps)
        label = L.amt_march_last_kernel().decode()
    finally:
        ens.close()
    return guard_record(f"guard ensemble {members}x{ni}x{nk}x{nj} f64", t, nk, label)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=8)
    ap.add_argument("--domain", default="4096x60x4096")
    ap.add_argument("--ensemble", default="32x128x60x128")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    torch.cuda.set_device(0)
    lines = []

    def emit(r):
        lines.append(r)
        print(json.dumps(r), flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(json.dumps(x) for x in lines) + "\n")
    if args.domain:
        dims = tuple(int(x) for x in args.domain.split("x"))
        for r in measure_domain(pkg, torch, dims, args.reps, args.sweeps):
            emit(r)
        torch.cuda.empty_cache()
    if args.ensemble:
        m, *dims = (int(x) for x in args.ensemble.split("x"))
        emit(measure_ensemble(pkg, torch, m, tuple(dims), args.reps, 3 * args.sweeps))


if __name__ == "__main__":
    main()
