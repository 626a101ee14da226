#!/usr/bin/env python3
"""A/B of the cyclic boundary refresh (include/amt_advance_mu_t.h section 9) in ONE process, HIP events
through the handles' own *_step_timed, after warm-up, A and B alternating on the SAME handle:

  A  plain stepping;
  B  the same with set_cyclic(X | Y): one refresh launch in front of every sweep's launch, on the same stream.

  domain    one amt_domain_create handle (default 4096 x 60 x 4096 fp64, the resident aligned layout)
  ensemble  one amt_ensemble_create handle (default 32 members of 128 x 60 x 128 fp64)

`model` is the refresh's share of the sweep's traffic from the shapes alone: a full 128-byte line read and a full line written
per column element, the row runs as they are, over the sweep's algorithmic bytes W * NI * NJ * (11 * NK + 14) (per member).

  python profiles/cyclic_ab.py [--reps 5] [--sweeps 10] [--domain 4096x60x4096] [--ensemble 32x128x60x128] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

LINE = 128
CYCLIC_XY = 3


def model(b, ni, nk, nj, wbytes):
    """Bytes the refresh touches / algorithmic bytes of one sweep, for a window of ni x nj columns and b.kdim memory levels."""
    col_elems = 4 * b.kdim * nj + 2 * nj                 # u, u_1, t_1 (twice: both sides) and muu, msfuy
    row_elems = 4 * b.kdim * ni + 2 * ni                 # v, v_1, t_1 (twice) and muv, msfvx_inv
    touched = col_elems * 2 * LINE + row_elems * 2 * wbytes
    return touched / (wbytes * ni * nj * (11 * nk + 14))


def interleave(step_timed, set_cyclic, reps, sweeps):
    """ms per sweep of A and of B, `reps` repeats each, alternating."""
    for axes in (0, CYCLIC_XY, 0):
        set_cyclic(axes)
        step_timed(2)
    ta, tb = [], []
    for _ in range(reps):
        set_cyclic(0)
        ta.append(step_timed(sweeps) / sweeps)
        set_cyclic(CYCLIC_XY)
        tb.append(step_timed(sweeps) / sweeps)
    set_cyclic(0)
    return ta, tb


def measure_domain(pkg, torch, dims=(4096, 60, 4096), dtype=np.float64, reps=5, sweeps=10, seed=11):
    import ctypes
    from wrf_model_cuda_sample_amd import lib
    S, L = pkg.synth, pkg.load_library()
    ni, nk, nj = dims
    b = S.domain_bounds(ni, nk, nj, aligned=True).replace(ite=ni, jte=nj)
    patch = S.make_patch(b, pkg.GridConfig(), dtype=dtype, seed=seed, global_dims=dims, device="cuda:0", native_domain=True)
    torch.cuda.synchronize()
    dom = patch.owner

    def step_timed(k):
        ms = ctypes.c_float()
        lib.check(L.amt_domain_step_timed(dom.handle, k, ctypes.byref(ms)))
        return float(ms.value)
    ta, tb = interleave(step_timed, dom.set_cyclic, reps, sweeps)
    label = L.amt_march_last_kernel().decode()
    return ta, tb, model(b, ni, nk, nj, np.dtype(dtype).itemsize), label


def measure_ensemble(pkg, torch, members=32, dims=(128, 60, 128), dtype=np.float64, reps=5, sweeps=20, seed=11):
    S, L = pkg.synth, pkg.load_library()
    ni, nk, nj = dims
    b = S.domain_bounds(ni, nk, nj, aligned=True).replace(ite=ni, jte=nj)
    ens = pkg.Ensemble(b, members, pkg.GridConfig(), dtype)
    try:
        ens.fill_synthetic(seed, global_dims=dims)
        ens.sync()
        ta, tb = interleave(ens.step_timed, ens.set_cyclic, reps, sweeps)
        label = L.amt_march_last_kernel().decode()
    finally:
        ens.close()
    return ta, tb, model(b, ni, nk, nj, np.dtype(dtype).itemsize), label


def record(what, ta, tb, mdl, label):
    a, b = statistics.median(ta), statistics.median(tb)
    return {"case": what, "A_ms_per_sweep": round(a, 5), "B_ms_per_sweep": round(b, 5), "B_over_A": round(b / a, 5),
            "model": round(mdl, 6), "spread_A": round((max(ta) - min(ta)) / a, 5),
            "A_repeats": [round(x, 5) for x in ta], "B_repeats": [round(x, 5) for x in tb], "label": label}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--domain", default="4096x60x4096")
    ap.add_argument("--ensemble", default="32x128x60x128")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    torch.cuda.set_device(0)
    lines = []
    if args.domain:
        dims = tuple(int(x) for x in args.domain.split("x"))
        lines.append(record(f"domain {args.domain} f64", *measure_domain(pkg, torch, dims, reps=args.reps, sweeps=args.sweeps)))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    if args.ensemble:
        m, *dims = (int(x) for x in args.ensemble.split("x"))
        lines.append(record(f"ensemble {args.ensemble} f64", *measure_ensemble(pkg, torch, m, tuple(dims), reps=args.reps, sweeps=2 * args.sweeps)))
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
