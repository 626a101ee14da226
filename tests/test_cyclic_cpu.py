"""Cyclic lateral boundaries without a GPU (include/amt_advance_mu_t.h section 9): properties of the numpy reference
tests/cyclic_ref.py that the GPU tests compare against, and the argument and precondition errors of the new entry points,
which are host arithmetic and are reported with or without a device."""
import ctypes

import numpy as np
import pytest

import cases
import cyclic_ref as CR

X, Y = CR.CYCLIC_X, CR.CYCLIC_Y


def _patch(pkg, dims=(12, 5, 9), dtype=np.float64, seed=7, **kw):
    b = pkg.synth.domain_bounds(*dims, **kw)
    return pkg.synth.make_patch(b, dtype=dtype, seed=seed, global_dims=dims)


def _copy(arrays):
    return {n: a.copy() for n, a in arrays.items()}


# ---------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axes", [X, Y, X | Y])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_is_idempotent(pkg, axes, dtype):
    p = _patch(pkg, dtype=dtype)
    once = CR.cyclic_fill(_copy(p.arrays), p.bounds, axes)
    twice = CR.cyclic_fill(_copy(once), p.bounds, axes)
    for n in pkg.synth.FIELD_NAMES:
        assert np.array_equal(CR.as_bits(once[n]), CR.as_bits(twice[n])), n
    assert any(not np.array_equal(CR.as_bits(once[n]), CR.as_bits(p.arrays[n])) for n in CR.MAY_CHANGE)


@pytest.mark.parametrize("axes", [X, Y, X | Y])
@pytest.mark.parametrize("aligned", [False, True])
def test_reference_writes_the_named_cells_only(pkg, axes, aligned):
    """Every cell outside the destination columns / rows keeps its bits, the four corners included; the destination cells
    hold what the definition names."""
    p = _patch(pkg, dims=(13, 4, 7), aligned=aligned)
    b = p.bounds
    got = CR.cyclic_fill(_copy(p.arrays), b, axes)
    c, r = (lambda i: i - b.ims), (lambda j: j - b.jms)
    J = slice(r(b.jds), r(b.jde - 1) + 1)
    I = slice(c(b.ids), c(b.ide - 1) + 1)
    for n in pkg.synth.FIELD_NAMES:
        before, after = p.arrays[n], got[n]
        written = np.zeros(before.shape, bool)
        if axes & X and n in CR.COLS_FROM_RIGHT:
            written[J, ..., c(b.ide)] = True
            assert np.array_equal(after[J, ..., c(b.ide)], before[J, ..., c(b.ids)]), n
        if axes & X and n in CR.COLS_FROM_LEFT:
            written[J, ..., c(b.ids - 1)] = True
            assert np.array_equal(after[J, ..., c(b.ids - 1)], before[J, ..., c(b.ide - 1)]), n
        if axes & Y and n in CR.ROWS_FROM_ABOVE:
            written[r(b.jde), ..., I] = True
            assert np.array_equal(after[r(b.jde), ..., I], before[r(b.jds), ..., I]), n
        if axes & Y and n in CR.ROWS_FROM_BELOW:
            written[r(b.jds - 1), ..., I] = True
            assert np.array_equal(after[r(b.jds - 1), ..., I], before[r(b.jde - 1), ..., I]), n
        assert np.array_equal(CR.as_bits(after)[~written], CR.as_bits(before)[~written]), f"{n}: a cell outside the named ones changed"
        assert written.any() == (n in CR.MAY_CHANGE and bool(
            (axes & X and n in CR.COLS_FROM_RIGHT + CR.COLS_FROM_LEFT) or (axes & Y and n in CR.ROWS_FROM_ABOVE + CR.ROWS_FROM_BELOW))), n
        if before.ndim >= 2:                                        # corners
            for jj in (r(b.jds - 1), r(b.jde)):
                for ii in (c(b.ids - 1), c(b.ide)):
                    assert not written[jj, ..., ii].any(), f"{n}: corner ({ii},{jj}) written"


def test_reference_follows_the_window_not_the_tile(pkg):
    """A last patch may end at ide-1 or at ide, and likewise in j: the same cells either way; with specified + periodic_x
    the column copies cover the clipped rows jds+1..jde-2 only."""
    p = _patch(pkg)
    b = p.bounds
    want = CR.cyclic_fill(_copy(p.arrays), b, X | Y)
    got = CR.cyclic_fill(_copy(p.arrays), b.replace(ite=b.ide - 1, jte=b.jde - 1), X | Y)
    for n in pkg.synth.FIELD_NAMES:
        assert np.array_equal(CR.as_bits(want[n]), CR.as_bits(got[n])), n
    clipped = CR.cyclic_fill(_copy(p.arrays), b, X, flags=(1, 1, 0))
    r = lambda j: j - b.jms
    t0, t1 = p.arrays["t_1"], clipped["t_1"]
    assert np.array_equal(t1[r(b.jds)], t0[r(b.jds)]) and np.array_equal(t1[r(b.jde - 1)], t0[r(b.jde - 1)])
    assert np.array_equal(t1[r(b.jds + 1), :, b.ide - b.ims], t0[r(b.jds + 1), :, b.ids - b.ims])


@pytest.mark.parametrize("members", [1, 2, 5])
def test_reference_treats_every_member_alone(pkg, members):
    ps = [_patch(pkg, seed=20 + m) for m in range(members)]
    b = ps[0].bounds
    S = pkg.synth
    stacked = {n: (ps[0].arrays[n].copy() if S.field_rank(n) == 1 else np.stack([p.arrays[n] for p in ps])) for n in S.FIELD_NAMES}
    CR.cyclic_fill(stacked, b, X | Y)
    for m, p in enumerate(ps):
        want = CR.cyclic_fill(_copy(p.arrays), b, X | Y)
        for n in S.FIELD_NAMES:
            got = stacked[n] if S.field_rank(n) == 1 else stacked[n][m]
            assert np.array_equal(CR.as_bits(got), CR.as_bits(want[n])), (n, m)


def test_reference_moves_bits(pkg):
    """NaN payloads and the sign of zero survive the reference's copy (the GPU test asks the same of the kernel)."""
    p = _patch(pkg)
    b = p.bounds
    bits = CR.as_bits(p.arrays["t_1"])
    bits[:, :, b.ids - b.ims] = np.uint64(0x7ff800000000beef)
    bits[:, 0, b.ids - b.ims] = np.uint64(0x8000000000000000)
    p.arrays["t_1"][...] = bits.view(np.float64)
    got = CR.cyclic_fill(_copy(p.arrays), b, X)
    J = slice(b.jds - b.jms, b.jde - b.jms)
    assert np.array_equal(CR.as_bits(got["t_1"])[J, :, b.ide - b.ims], bits[J, :, b.ids - b.ims])


# ---------------------------------------------------------------------------------------------
# argument and precondition errors of the entry points: no device needed to reach them
# ---------------------------------------------------------------------------------------------
def _fill(L, fn, axes, members, flags, b, ptrs=None):
    return getattr(L, fn)(None, axes, members, *(ptrs or [None] * 9), *flags, *b.as_tuple())


@pytest.mark.parametrize("fn", ["amt_cyclic_fill_device_f32", "amt_cyclic_fill_device_f64"])
def test_bad_arguments_are_invalid_arguments(pkg, fn):
    L = pkg.load_library()
    b = pkg.synth.domain_bounds(16, 8, 16)
    for axes in (-1, 4, 7):
        assert _fill(L, fn, axes, 1, (0, 0, 0), b) == 3, (axes, L.amt_last_error())
    for members in (0, -2):
        assert _fill(L, fn, X, members, (0, 0, 0), b) == 3, (members, L.amt_last_error())
    for name in ("amt_domain_cyclic_fill", "amt_domain_set_cyclic", "amt_ensemble_cyclic_fill", "amt_ensemble_set_cyclic"):
        assert getattr(L, name)(None, X) == 3, name
    assert L.amt_domain_cyclic(None) == 0 and L.amt_ensemble_cyclic(None) == 0


@pytest.mark.parametrize("fn", ["amt_cyclic_fill_device_f32", "amt_cyclic_fill_device_f64"])
def test_preconditions_are_reported(pkg, fn):
    L = pkg.load_library()
    b = pkg.synth.domain_bounds(16, 8, 16)
    refused = [
        ("cyclic y with specified", Y, (0, 1, 0), b),
        ("cyclic y with nested", Y, (0, 0, 1), b),
        ("cyclic y with specified and periodic_x", Y, (1, 1, 0), b),
        ("cyclic x with a clipped i window", X, (0, 1, 0), b),
        ("cyclic x with a nested, clipped i window", X, (0, 0, 1), b),
        ("memory without column ide", X, (0, 0, 0), b.replace(ime=b.ide - 1)),
        ("memory without column ids-1", X, (0, 0, 0), b.replace(ims=b.ids)),
        ("memory without row jde", Y, (0, 0, 0), b.replace(jme=b.jde - 1)),
        ("memory without row jds-1", Y, (0, 0, 0), b.replace(jms=b.jds)),
        ("a patch that does not hold the period in i", X, (0, 0, 0), b.replace(its=5)),
        ("a patch that does not hold the period in j", Y, (0, 0, 0), b.replace(jte=9)),
        ("empty memory", X, (0, 0, 0), b.replace(kme=0)),
    ]
    for what, axes, flags, bb in refused:
        assert _fill(L, fn, axes, 1, flags, bb) == 2, (what, L.amt_last_error())
        assert L.amt_last_error(), what
    # the other axis is not held to the refused axis's conditions
    assert _fill(L, fn, X, 1, (1, 1, 0), b) != 2, L.amt_last_error()
    assert _fill(L, fn, X, 1, (0, 0, 0), b.replace(jme=b.jde - 1, jte=b.jde - 1)) != 2, L.amt_last_error()


def test_no_cpu_fallback_without_a_device(pkg):
    """Well-formed host arrays on a box without a GPU: an error status, and the arrays as they were."""
    L = pkg.load_library()
    if L.amt_device_count() > 0:
        pytest.skip("a device is present")
    p = cases.make_case(pkg, "16x8x16", "none", np.float64)
    before = p.copy()
    names = ("u", "u_1", "v", "v_1", "t_1", "muu", "muv", "msfuy", "msfvx_inv")
    ptrs = [p.arrays[n].ctypes.data_as(ctypes.c_void_p) for n in names]
    st = _fill(L, "amt_cyclic_fill_device_f64", X | Y, 1, (0, 0, 0), p.bounds, ptrs)
    assert st in (1, 4), (st, L.amt_last_error())
    for n in pkg.synth.FIELD_NAMES:
        assert np.array_equal(p.arrays[n], before.arrays[n]), n
    assert _fill(L, "amt_cyclic_fill_device_f64", 0, 1, (0, 0, 0), p.bounds, ptrs) in (0, 1, 4)     # axes = 0: nothing to do
    with pytest.raises(TypeError):
        pkg.cyclic_fill(*[p.arrays[n] for n in names], p.config, *p.bounds.as_tuple())             # numpy arrays: no host path


# ---------------------------------------------------------------------------------------------
# the pure-Python steppers over gloo with cyclic=(x, y): the torus topology of amt_grid_create on CPU tensors
# ---------------------------------------------------------------------------------------------
import os                                   # noqa: E402
import socket                               # noqa: E402
import sys                                  # noqa: E402
from pathlib import Path                    # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
GLOO_SEED = 61


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_bounds(S, shape, ri, rj, pi, pj):
    gb = S.domain_bounds(*shape)
    return S.patch_bounds(gb.replace(ite=gb.ide - 1, jte=gb.jde - 1), ri, rj, pi, pj)


def _gloo_worker(rank, world, port, shape, flags, pi, pj, cyclic, slab, sweeps, out_dir):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import __graft_entry__ as g
        pkg, oracle = g.load_package(), g.load_oracle()
        S = pkg.synth
        ri, rj = rank % pi, rank // pi
        pb = _rank_bounds(S, shape, ri, rj, pi, pj)
        host = S.make_patch(pb, pkg.GridConfig(**flags), seed=GLOO_SEED, global_dims=shape)
        arrays = {k: torch.from_numpy(v) for k, v in host.arrays.items()}
        patch = S.Patch(pb, host.config, arrays, host.rdx, host.rdy, host.dts, host.epssm, shape)

        def compute(*args):
            oracle.advance_mu_t(*[a.numpy() if isinstance(a, torch.Tensor) else a for a in args])

        if slab:
            st = pkg.patch.SlabStepper(patch, rj, pj, compute, cyclic=cyclic)
        else:
            st = pkg.patch.GridStepper(patch, ri, rj, pi, pj, compute, cyclic=cyclic)
        for sweep in range(sweeps):
            S.refresh_exchanged_inputs(patch, GLOO_SEED, sweep)          # new u, v, t_1 ... every sweep
            S.poison_halos(patch, 15)                                     # all four sides, the outer ones included
            st.step()
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **{n: arrays[n].numpy() for n in S.OUTPUTS})
    finally:
        dist.destroy_process_group()


def _gloo_run(tmp_path, pkg, oracle, pi, pj, shape, flags, cyclic, slab, sweeps=3):
    """Runs the ranks; returns (per-rank outputs over the owned cells, the unsplit oracle's arrays, bounds per rank)."""
    import torch.multiprocessing as mp
    world = pi * pj
    mp.spawn(_gloo_worker, args=(world, _free_port(), shape, flags, pi, pj, cyclic, slab, sweeps, str(tmp_path)), nprocs=world, join=True)
    S = pkg.synth
    gb = S.domain_bounds(*shape)
    gb = gb.replace(ite=gb.ide - 1, jte=gb.jde - 1)
    cfg = pkg.GridConfig(**flags)
    full = S.make_patch(gb, cfg, seed=GLOO_SEED, global_dims=shape)
    axes = (X if cyclic[0] else 0) | (Y if cyclic[1] else 0)
    for sweep in range(sweeps):
        S.refresh_exchanged_inputs(full, GLOO_SEED, sweep)
        S.poison_halos(full, 15)
        if axes:
            CR.cyclic_fill(full.arrays, gb, axes, cfg.as_ints())
        oracle.advance_mu_t(*full.args())
    got, want, bounds = [], [], []
    for rank in range(world):
        b = _rank_bounds(S, shape, rank % pi, rank // pi, pi, pj)
        r = np.load(tmp_path / f"rank{rank}.npz")
        own = (slice(b.jts - b.jms, b.jte - b.jms + 1), Ellipsis, slice(b.its - b.ims, b.ite - b.ims + 1))
        glob = (slice(b.jts - gb.jms, b.jte - gb.jms + 1), Ellipsis, slice(b.its - gb.ims, b.ite - gb.ims + 1))
        got.append({n: r[n][own] for n in S.OUTPUTS})
        want.append({n: full.arrays[n][glob] for n in S.OUTPUTS})
        bounds.append(b)
    return got, want, bounds


WORLDS = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 2)]


@pytest.mark.parametrize("pi,pj", WORLDS, ids=[f"{a}x{b}" for a, b in WORLDS])
def test_python_steppers_on_a_torus_reproduce_the_unsplit_wrapped_domain(tmp_path, pkg, oracle, pi, pj):
    """GridStepper with cyclic=(True, True): self wrap where a direction has one rank, the same peer twice where it has two, the
    edge ranks as each other's neighbours beyond.  Bit-equal to the unsplit oracle on the wrapped domain, and finite."""
    shape = (13, 4, 9)
    for flags in (dict(), dict(periodic_x=True)):
        d = tmp_path / ("p" if flags else "n")
        d.mkdir()
        got, want, _ = _gloo_run(d, pkg, oracle, pi, pj, shape, flags, (True, True), slab=False)
        for rank, (g_, w_) in enumerate(zip(got, want)):
            for n in pkg.synth.OUTPUTS:
                assert np.array_equal(CR.as_bits(g_[n]), CR.as_bits(w_[n])), (pi, pj, flags, rank, n)
                lev = g_[n][:, :-1] if g_[n].ndim == 3 else g_[n]
                assert np.isfinite(lev).all(), (pi, pj, flags, rank, n)


@pytest.mark.parametrize("world,cyclic", [(1, (True, True)), (2, (False, True)), (3, (True, True)), (2, (True, False))],
                         ids=["1-xy", "2-y", "3-xy", "2-x-only"])
def test_python_slab_stepper_with_cyclic(tmp_path, pkg, oracle, world, cyclic):
    """SlabStepper: cyclic y joins slab 0 and slab world-1 (two ranks: the same peer twice), cyclic x is a self wrap of every slab.
    Sides that are NOT cyclic are poisoned as well: their window edge is NaN in the unsplit run too (number for number)."""
    shape = (11, 3, 8)
    got, want, _ = _gloo_run(tmp_path, pkg, oracle, 1, world, shape, dict(periodic_x=cyclic[0]), cyclic, slab=True)
    for rank, (g_, w_) in enumerate(zip(got, want)):
        for n in pkg.synth.OUTPUTS:
            if all(cyclic):
                assert np.array_equal(CR.as_bits(g_[n]), CR.as_bits(w_[n])), (world, cyclic, rank, n)
            else:
                assert np.array_equal(g_[n], w_[n], equal_nan=True), (world, cyclic, rank, n)


@pytest.mark.parametrize("pi,pj", WORLDS, ids=[f"{a}x{b}" for a, b in WORLDS])
def test_with_cyclic_off_the_outermost_window_cells_are_nan(tmp_path, pkg, oracle, pi, pj):
    """The same runs with cyclic off: the inputs can see a missing wrap."""
    got, want, bounds = _gloo_run(tmp_path, pkg, oracle, pi, pj, (13, 4, 9), dict(), (False, False), slab=False)
    for rank, (g_, b) in enumerate(zip(got, bounds)):
        mu, t = g_["mu"], g_["t"]
        if rank % pi == pi - 1:
            assert np.isnan(mu[:, -1]).all(), (rank, "column ide-1 reads u(ide)")
        if rank % pi == 0:
            assert np.isnan(t[:, :-1, 0]).all(), (rank, "column ids reads t_1(ids-1)")
        if rank // pi == pj - 1:
            assert np.isnan(mu[-1, :]).all(), (rank, "row jde-1 reads v(jde)")
        if rank // pi == 0:
            assert np.isnan(t[0, :-1, :]).all(), (rank, "row jds reads t_1(jds-1)")
        assert np.array_equal(mu, want[rank]["mu"], equal_nan=True), rank
