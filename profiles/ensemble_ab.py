#!/usr/bin/env python3
"""A/B of the ensemble path (include/amt_advance_mu_t.h section 8) in ONE process on ONE stream, HIP events, after warm-up,
A and B alternating:

  A  M resident amt_domain handles (amt_domain_wrap over the members of a stacked state) stepped one after the other: what
     the library could do before ensembles existed -- M launches per sweep, each planned for one patch alone;
  B  one amt_ensemble over an identical stacked state: one launch per sweep, planned for the batch.

Prints one JSON line per case: median ms per member-sweep of A and B, every repeat, the ratio, the modelled ratio from the
plan functions (amt_march_rows_for / amt_march_rows_for_members, rounds * (r + 0.5)), the state size against the 256 MB
last-level cache and -- only where the M states together exceed it -- the fraction of the 8 TB/s roofline from the algorithmic
bytes W * NI * NJ * (11 * NK + 14) per member.

  python profiles/ensemble_ab.py [--reps 5] [--sweeps 20] [--quick] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import re
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CASES = [  # dtype, columns per side, levels, members
    ("f64", 128, 60, 8), ("f64", 128, 60, 32), ("f64", 256, 60, 8), ("f64", 256, 60, 32),
    ("f64", 512, 60, 8), ("f64", 512, 60, 32), ("f32", 256, 60, 8), ("f32", 256, 60, 32),
]
LLC_BYTES = 256 << 20
HBM_BYTES_PER_S = 8.0e12


def modelled(L, label_a: str, label_b: str, n: int, members: int, wbytes: int, cus: int = 256):
    """Row-times per member of A and of B from the launcher's cost model, for the tile widths the two plans really chose."""
    def tiles(label):
        m = re.search(r"<\w+, (\d+), \d+, (\d+),", label)
        vw, hl = int(m.group(1)), int(m.group(2))
        return -(-n // ((64 // hl) * vw)), hl

    def cost(cols, hl, r):
        return -(-(cols * -(-n // r)) // cus) * (r + 0.5)
    ta, hla = tiles(label_a)
    tb, hlb = tiles(label_b)
    ra = L.amt_march_rows_for(ta, n, cus, 1 << 20, wbytes, hla)
    rb = L.amt_march_rows_for_members(tb, members, n, cus, 1 << 20, wbytes, hlb)
    return cost(ta, hla, ra), cost(tb * members, hlb, rb) / members, ra, rb


def measure(pkg, torch, dtype, n, nk, members, reps=5, sweeps=20, seed=11):
    """(A ms per member-sweep per repeat, B the same, label of A, label of B)."""
    from wrf_model_cuda_sample_amd import lib
    S, L = pkg.synth, pkg.load_library()
    cfg = pkg.GridConfig()
    b = S.domain_bounds(n, nk, n, aligned=True)
    tdt = torch.float64 if np.dtype(dtype).itemsize == 8 else torch.float32
    stream = torch.cuda.Stream()
    fields = lambda arrs: (ctypes.c_void_p * len(S.FIELD_NAMES))(*[arrs[f].data_ptr() for f in S.FIELD_NAMES])
    with torch.cuda.stream(stream):
        state_a = {f: torch.empty(pkg.ensemble.stacked_shape(b, f, members), dtype=tdt, device="cuda:0") for f in S.FIELD_NAMES}
        state_b = {f: torch.empty_like(a) for f, a in state_a.items()}
        ens_a = pkg.Ensemble.wrap(state_a, b, cfg)          # only to fill A's state like B's
        ens_b = pkg.Ensemble.wrap(state_b, b, cfg)
        ens_a.fill_synthetic(seed)
        ens_b.fill_synthetic(seed)
        doms = []
        for m in range(members):
            h = ctypes.c_void_p()
            view = {f: (a if S.field_rank(f) == 1 else a[m]) for f, a in state_a.items()}
            lib.check(L.amt_domain_wrap(ctypes.byref(h), np.dtype(dtype).itemsize, *cfg.as_ints(), *b.as_tuple(), fields(view),
                                        ctypes.c_void_p(stream.cuda_stream)))
            doms.append(h)

        def run_a(k):
            for _ in range(k):
                for h in doms:
                    st = L.amt_domain_step(h, 1)
                    if st:
                        lib.check(st)

        def run_b(k):
            ens_b.step(k)

        def timed(run):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run(sweeps)
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / (sweeps * members)
        run_a(3)
        label_a = L.amt_march_last_kernel().decode()
        run_b(3)
        label_b = L.amt_march_last_kernel().decode()
        stream.synchronize()
        ta, tb = [], []
        for _ in range(reps):
            ta.append(timed(run_a))
            tb.append(timed(run_b))
        for h in doms:
            lib.check(L.amt_domain_destroy(h))
        ens_a.close()
        ens_b.close()
    return ta, tb, label_a, label_b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="the 128 x 128 cases only")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    L = pkg.load_library()
    torch.cuda.set_device(0)
    lines = []
    for dt, n, nk, members in CASES:
        if args.quick and n != 128:
            continue
        dtype = np.float64 if dt == "f64" else np.float32
        w = np.dtype(dtype).itemsize
        ta, tb, la, lb = measure(pkg, torch, dtype, n, nk, members, args.reps, args.sweeps)
        a, b = statistics.median(ta), statistics.median(tb)
        ma, mb, ra, rb = modelled(L, la, lb, n, members, w)
        alg = w * n * n * (11 * nk + 14)
        state = members * S_bytes(pkg, n, nk, w)
        rec = {"dtype": dt, "columns": n, "levels": nk, "members": members,
               "A_ms_per_member_sweep": round(a, 5), "B_ms_per_member_sweep": round(b, 5), "A_over_B": round(a / b, 3),
               "A_repeats": [round(x, 5) for x in ta], "B_repeats": [round(x, 5) for x in tb],
               "modelled_A_over_B": round(ma / mb, 3), "rows_per_block_A": ra, "rows_per_block_B": rb,
               "state_MB": round(state / 1e6, 1), "exceeds_llc": state > LLC_BYTES,
               "roofline_fraction_A": round(alg / (a * 1e-3) / HBM_BYTES_PER_S, 3) if state > LLC_BYTES else None,
               "roofline_fraction_B": round(alg / (b * 1e-3) / HBM_BYTES_PER_S, 3) if state > LLC_BYTES else None,
               "label_A": la, "label_B": lb}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in lines) + "\n")


def S_bytes(pkg, n, nk, w):
    """Bytes of ONE member's 3-D and 2-D arrays in the resident (aligned) layout."""
    b = pkg.synth.domain_bounds(n, nk, n, aligned=True)
    return w * (10 * b.jdim * b.kdim * b.idim + 12 * b.jdim * b.idim)


if __name__ == "__main__":
    main()
