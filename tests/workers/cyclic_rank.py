"""One rank of a multi-process run on ONE device with cyclic lateral boundaries (tests/test_gpu_35_cyclic_multirank.py starts
pi * pj of these): the native steppers amt_grid_* / amt_slab_* over the IPC transport with AMT_SLAB_CYCLIC_X / _Y.  Before
EVERY sweep the rank gives the exchanged fields new values (seed + sweep, as advance_uv would) and poisons with NaN every halo
row and column a sweep reads -- on all four sides where the flags say the domain wraps there, the outer sides included -- then
steps once.  It writes the cells it owns of every output to <dir>/out_<rank>_<name>.npy; the parent holds the unsplit oracle run
on the wrapped domain."""
import argparse
import ctypes
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def rank_bounds(S, dims, ri, rj, pi, pj, align, slab):
    """The patch of rank (ri, rj): tiles end at ide-1 / jde-1 (the halo column ite+1 must exist for the poison)."""
    gb = S.domain_bounds(*dims)
    gb = gb.replace(ite=gb.ide - 1, jte=gb.jde - 1)
    return S.slab_bounds(gb, rj, pj) if slab else S.patch_bounds(gb, ri, rj, pi, pj, align_elems=align)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--grid", type=int, nargs=2, required=True, metavar=("PI", "PJ"))
    ap.add_argument("--slab", action="store_true", help="amt_slab_* (PI must be 1) instead of amt_grid_*")
    ap.add_argument("--cyclic", type=int, nargs=2, required=True, metavar=("X", "Y"))
    ap.add_argument("--poison-sides", type=int, default=-1, help="-1: the sides the flags deliver; else this mask (cyclic-off runs)")
    ap.add_argument("--dir", required=True)
    ap.add_argument("--dims", type=int, nargs=3, required=True)
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--seed", type=int, default=23)
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--no-overlap", action="store_true")
    ap.add_argument("--periodic-x", action="store_true")
    ap.add_argument("--align", type=int, default=32)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    S, L = pkg.synth, pkg.load_library()
    torch.cuda.set_device(0)
    dtype = np.float64 if a.dtype == "f64" else np.float32
    dims, (pi, pj) = tuple(a.dims), a.grid
    world = pi * pj
    ri, rj = a.rank % pi, a.rank // pi
    pb = rank_bounds(S, dims, ri, rj, pi, pj, a.align, a.slab)
    cfg = pkg.GridConfig(periodic_x=a.periodic_x)
    cyclic = (bool(a.cyclic[0]), bool(a.cyclic[1]))
    uid = None
    if world > 1:
        buf = (ctypes.c_char * 128)()
        pkg.lib.check(L.amt_comm_rendezvous_file(str(Path(a.dir) / "uid").encode(), 0, a.rank, world, 90.0, buf))
        uid = bytes(buf)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev = S.make_patch(pb, cfg, dtype=dtype, seed=a.seed, global_dims=dims, device="cuda:0")
    torch.cuda.synchronize()
    kw = dict(stream=stream, overlap=not a.no_overlap, transport="ipc", cyclic=cyclic)
    if a.slab:
        st = pkg.patch.NativeSlabStepper(dev, rj, pj, uid, **kw)
    else:
        st = pkg.patch.NativeGridStepper(dev, ri, rj, pi, pj, uid, **kw)
    if a.poison_sides >= 0:
        st._halo_sides = a.poison_sides
    try:
        seen = st.comm_info()
        for sweep in range(a.sweeps):              # new u, v, t_1 ... and re-poisoned halos before EVERY sweep
            st.next_substep_inputs(a.seed, sweep)
            st.step(1)
        st.sync()
        own = (slice(pb.jts - pb.jms, pb.jte - pb.jms + 1), Ellipsis, slice(pb.its - pb.ims, pb.ite - pb.ims + 1))
        for n in S.OUTPUTS:
            np.save(Path(a.dir) / f"out_{a.rank}_{n}.npy", dev.arrays[n][own].cpu().numpy())
        print(f"rank {a.rank} = patch ({ri},{rj}) of {pi}x{pj}: i {pb.its}..{pb.ite} j {pb.jts}..{pb.jte}, cyclic {cyclic}, transport "
              f"{st.transport()}, ranks seen {seen[1]}, pull by {st.pull_mode()}, halo bytes {st.halo_bytes_per_sweep()}", flush=True)
    finally:
        st.close()


if __name__ == "__main__":
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    main()
