#!/usr/bin/env python3
"""A/B of the boundary-zone update of specified / nested domains (include/amt_advance_mu_t.h section 12)
in ONE process, HIP events through the handle's own amt_domain_step_timed, after warm-up, A and B alternating on the SAME
handle:

  A  plain stepping of a `specified` domain;
  B  the same with set_spec_bdy(1): one amt_bdy_kernel launch behind every sweep's launch, on the same stream.

`model` is the update's share of the sweep's traffic from the shapes alone: the row strips as they lie (two reads and one
write per element), a full 128-byte line read per operand and a full line written per column element, over the sweep's
algorithmic bytes W * NI * NJ * (11 * NK + 14).

  python profiles/bdy_ab.py [--reps 5] [--sweeps 10] [--domain 4096x60x4096] [--out FILE]
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


def model(ni, nk, nj, wbytes):
    """Bytes the update touches / algorithmic bytes of one sweep, flags (0,1,0), tile = domain: two rows of ni cells, two
    columns of nj - 2 cells; per cell nk levels of t and one element each of mu and muts."""
    per_cell = nk + 2
    row_bytes = 2 * ni * per_cell * 3 * wbytes           # dst read, tendency read, dst written
    col_bytes = 2 * (nj - 2) * per_cell * 3 * LINE       # one line per element and access
    return (row_bytes + col_bytes) / (wbytes * ni * nj * (11 * nk + 14))


def measure(pkg, torch, dims, dtype=np.float64, reps=5, sweeps=10, seed=11):
    S, L = pkg.synth, pkg.load_library()
    ni, nk, nj = dims
    b = S.domain_bounds(ni, nk, nj, aligned=True).replace(ite=ni, jte=nj)
    patch = S.make_patch(b, pkg.GridConfig(specified=True), dtype=dtype, seed=seed, global_dims=dims, device="cuda:0", native_domain=True)
    torch.cuda.synchronize()
    dom = patch.owner
    for on in (False, True, False):
        dom.set_spec_bdy(on)
        dom.step_timed(2)
    ta, tb = [], []
    for _ in range(reps):
        dom.set_spec_bdy(False)
        ta.append(dom.step_timed(sweeps) / sweeps)
        dom.set_spec_bdy(True)
        tb.append(dom.step_timed(sweeps) / sweeps)
    dom.set_spec_bdy(False)
    return ta, tb, model(ni, nk, nj, np.dtype(dtype).itemsize), L.amt_march_last_kernel().decode()


def record(what, ta, tb, mdl, label):
    a, b = statistics.median(ta), statistics.median(tb)
    diffs = [y - x for x, y in zip(ta, tb)]
    return {"case": what, "A_ms_per_sweep": round(a, 5), "B_ms_per_sweep": round(b, 5), "B_over_A": round(b / a, 5),
            "B_minus_A_ms": round(statistics.median(diffs), 5), "B_minus_A_ms_min_max": [round(min(diffs), 5), round(max(diffs), 5)],
            "model": round(mdl, 6), "spread_A": round((max(ta) - min(ta)) / a, 5),
            "A_repeats": [round(x, 5) for x in ta], "B_repeats": [round(x, 5) for x in tb], "label": label}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--domain", default="4096x60x4096")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    torch.cuda.set_device(0)
    dims = tuple(int(x) for x in args.domain.split("x"))
    rec = record(f"domain {args.domain} f64 specified", *measure(pkg, torch, dims, reps=args.reps, sweeps=args.sweeps))
    print(json.dumps(rec), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
