"""GPU parity on inputs without the generator's symmetries (tests/hard_inputs.py): WRF-like vertical metrics whose levels are
all distinct -- no period of 8 or 16, no mirror, fnp not 1 - fnm -- and scalars with long mantissas that change between calls
on the same arrays (dts as dts_rk of the next Runge-Kutta stage; two nested domains alternating on one host thread).  Every
path that carries the metrics or the scalars: each march instantiation forced, the column kernel and AUTO, the one-shot call
(plain, residency cache in check mode, deferred outputs, three device slots), the resident handle (amt_domain_create and
amt_domain_wrap with amt_domain_set_scalars), the slab and grid steppers in loopback and a 2 x 2 grid of processes, and one
headline-size sweep.  Bit for bit against the oracle on the same inputs."""
import ctypes
import re
import time

import numpy as np
import pytest

import hard_inputs as H
from conftest import bits_equal, slow_note
from multirank import grid_mismatches, loopback_halos_by_hand, run_grid_ranks
from test_gpu_11_shapes import SHAPES, _id

pytestmark = pytest.mark.gpu

SETS = list(H.SCALAR_SETS)
FLAGS = [dict(), dict(specified=True), dict(specified=True, periodic_x=True), dict(nested=True)]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


@pytest.fixture()
def force(pkg):
    L = pkg.load_library()
    yield lambda *a: L.amt_march_force_shape(*a)
    L.amt_march_force_shape(0, 0, 0, -1, 1, 0, 0)


def _hard_host(pkg, b, cfg, dtype, seed, gdims, sset, level_seed=None):
    p = pkg.synth.make_patch(b, cfg, dtype=dtype, seed=seed, global_dims=gdims)
    return H.apply(p, H.levels_for(p, seed if level_seed is None else level_seed), H.SCALAR_SETS[sset])


def _assert_outputs(pkg, got, want, what):
    for n in pkg.synth.OUTPUTS:
        assert bits_equal(np.asarray(got.arrays[n]), np.asarray(want.arrays[n])), f"{what}: {n} differs from the oracle"


def _levels(kpt, hl, wm):
    """Whole cell waves, one wave and a level more, one level short of three waves, and a tall count that is no multiple of 8
    (the generator's period) -- at most what (wm - 1) cell waves hold."""
    lw, cap = kpt * hl, (wm - 1) * kpt * hl
    tall = 37 if cap >= 37 else cap - (1 if cap % 8 == 0 else 0)
    return sorted({n for n in (lw, 2 * lw + 1, 3 * lw - 1, tall) if 1 <= n <= cap})


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_every_march_instantiation_on_wrf_levels(pkg, oracle, force, torch_mod, shape):
    dtype, vw, kpt, hl, xd, dma, wm = shape
    S = pkg.synth
    L = pkg.load_library()
    tc = (64 // hl) * vw
    ni = 2 * tc + tc // 2 + 3
    for n, nk in enumerate(_levels(kpt, hl, wm)):
        cfg = pkg.GridConfig(**FLAGS[n % 4])
        sset = SETS[n % len(SETS)]
        for aligned in (True, False):
            b = S.domain_bounds(ni, nk, 7, aligned=aligned)
            if not aligned and vw == 2 and not dma:
                # the register flavour with two columns per lane needs whole pairs from the first tile's column 0 to the row end
                # (test_gpu_11_shapes)
                line = 128 // np.dtype(dtype).itemsize
                for _ in range(3):
                    i0 = pkg.compute_window(cfg, b.ids, b.ide, b.jds, b.jde, b.its, b.ite, b.jts, b.jte, b.kts, b.kte)[0] - b.ims
                    col_lo = i0 if b.idim % line else i0 // line * line
                    if (b.idim - col_lo) % 2 == 0:
                        break
                    b = b.replace(ime=b.ime + 1)
            host = _hard_host(pkg, b, cfg, dtype, 300 + nk, (ni, nk, 7), sset)
            want = host.copy()
            oracle.advance_mu_t(*want.args())
            for jrows in (0, 3):
                force(vw, kpt, hl, xd, dma, jrows, wm)
                dev = host.to_device("cuda:0")
                pkg.advance_mu_t(*dev.args(), variant=pkg.VARIANT_MARCH)
                torch_mod.cuda.synchronize()
                name = L.amt_march_last_kernel().decode()
                assert f", {vw}, {kpt}, {hl}, {xd}, FULL, {'true' if dma else 'false'}, {wm}, " in name, name
                _assert_outputs(pkg, dev.to_host(), want, f"{_id(shape)} nk={nk} aligned={aligned} jrows={jrows} {sset} ({name})")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_column_kernel_on_wrf_levels(pkg, oracle, torch_mod, dtype):
    S = pkg.synth
    for n, nk in enumerate((1, 2, 9, 61, 241, 300)):
        b = S.domain_bounds(70, nk, 5, aligned=bool(n % 2))
        host = _hard_host(pkg, b, pkg.GridConfig(**FLAGS[n % 4]), dtype, 500 + nk, (70, nk, 5), SETS[n % len(SETS)])
        want = host.copy()
        oracle.advance_mu_t(*want.args())
        dev = host.to_device("cuda:0")
        pkg.advance_mu_t(*dev.args(), variant=pkg.VARIANT_COLUMN)
        torch_mod.cuda.synchronize()
        _assert_outputs(pkg, dev.to_host(), want, f"column kernel nk={nk}")


@pytest.mark.parametrize("dims,dtype,aligned", [((64, 40, 64), np.float64, False), ((64, 40, 64), np.float32, True),
                                                ((512, 60, 64), np.float64, True), ((512, 60, 64), np.float64, False)],
                         ids=["64x40x64-f64", "64x40x64-f32-aligned", "512x60x64-f64-nt", "512x60x64-f64-cached"])
def test_auto_on_wrf_levels(pkg, oracle, torch_mod, dims, dtype, aligned):
    """AUTO, the launcher's own choice; at 512 x 60 x 64 aligned rows take the non-temporal streams and WRF's unpadded rows the
    cached ones."""
    S = pkg.synth
    b = S.domain_bounds(*dims, aligned=aligned)
    host = _hard_host(pkg, b, pkg.GridConfig(specified=True), dtype, 77, dims, "rk3_dx12km")
    want = host.copy()
    oracle.advance_mu_t(*want.args())
    dev = host.to_device("cuda:0")
    pkg.advance_mu_t(*dev.args())
    torch_mod.cuda.synchronize()
    label = pkg.load_library().amt_march_last_kernel().decode()
    _assert_outputs(pkg, dev.to_host(), want, f"AUTO {dims} ({label})")
    if dims[0] == 512:
        assert (", nt>" if aligned else ", cached>") in label, label


def _oneshot_sequence(pkg, oracle, got, want, mode):
    """Sub-steps on the same host arrays: the second changes dts (the next RK stage); after amt_host_invalidate the third also
    has new metrics; then two scalar sets alternate (two domains on one host thread)."""
    seq = [("rk3_dx12km", None), ("rk2_dx3km", None), ("rk1_dx1km", 91)] + [(s, None) for s in ("nest_dx333m", "rk3_dx12km") * 2]
    for step, (sset, new_levels) in enumerate(seq):
        sc = dict(H.SCALAR_SETS["rk3_dx12km"], dts=H.SCALAR_SETS[sset]["dts"]) if step == 1 else H.SCALAR_SETS[sset]
        for p in (got, want):
            H.apply(p, H.levels_for(p, new_levels) if new_levels is not None else None, sc)
        if new_levels is not None and mode in ("cached", "deferred"):
            pkg.host_invalidate(None)                      # the cached metrics changed on the host
        pkg.advance_mu_t(*got.args())
        oracle.advance_mu_t(*want.args())
        if mode == "deferred":
            pkg.host_fetch(None)
        _assert_outputs(pkg, got, want, f"one-shot ({mode}) sub-step {step} {sset}")


@pytest.mark.parametrize("mode", ["plain", "cached", "deferred", "three-slots"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_shot_call_with_changing_scalars_and_metrics(pkg, oracle, torch_mod, dtype, mode):
    S = pkg.synth
    b = S.domain_bounds(130, 41, 31)
    got = _hard_host(pkg, b, pkg.GridConfig(nested=True), dtype, 61, (130, 41, 31), "rk3_dx12km")
    want = got.copy()
    try:
        if mode in ("cached", "deferred"):
            pkg.host_cache_enable(True, check=True)
        if mode == "deferred":
            pkg.host_defer(None, True)
        if mode == "three-slots":
            pkg.host_set_devices([0, 0, 0])
        _oneshot_sequence(pkg, oracle, got, want, mode)
    finally:
        if mode == "three-slots":
            pkg.host_set_devices(())
        if mode == "deferred":
            pkg.host_defer(None, False)
        if mode in ("cached", "deferred"):
            pkg.host_cache_enable(False, check=False)
        pkg.load_library().amt_host_release()


def _scalars_of(sset, dtype):
    r = H.rounded_scalars(H.SCALAR_SETS[sset], dtype)
    return r["rdx"], r["rdy"], r["dts"], r["epssm"]


@pytest.mark.parametrize("how", ["create", "wrap"])
@pytest.mark.parametrize("dims,dtype,aligned", [((200, 61, 24), np.float64, True), ((203, 41, 17), np.float32, False)],
                         ids=["f64-aligned", "f32-unpadded"])
def test_resident_handle_with_set_scalars_between_sweeps(pkg, oracle, torch_mod, dims, dtype, aligned, how):
    """amt_domain_create (the tensors view the handle's arrays) or amt_domain_wrap (the handle borrows torch's): the metrics
    written into its fields, amt_domain_set_scalars before each of three sweeps with another set each time."""
    from wrf_model_cuda_sample_amd import lib
    S, L = pkg.synth, pkg.load_library()
    b = S.domain_bounds(*dims, aligned=aligned)
    cfg = pkg.GridConfig(specified=True)
    dev = S.make_patch(b, cfg, dtype=dtype, seed=19, global_dims=dims, device="cuda:0", native_domain=(how == "create"))
    H.apply(dev, H.levels_for(dev, 19), H.SCALAR_SETS[SETS[0]])
    want = dev.to_host()
    torch_mod.cuda.synchronize()
    if how == "create":
        h = dev.owner.handle
    else:
        h = ctypes.c_void_p()
        fields = (ctypes.c_void_p * len(S.FIELD_NAMES))(*[dev.arrays[n].data_ptr() for n in S.FIELD_NAMES])
        lib.check(L.amt_domain_wrap(ctypes.byref(h), np.dtype(dtype).itemsize, *cfg.as_ints(), *b.as_tuple(), fields, None))
    seq = [SETS[0], SETS[2], SETS[1]]
    try:
        for sset in seq:
            lib.check(L.amt_domain_set_scalars(h, *_scalars_of(sset, dtype)))
            lib.check(L.amt_domain_step(h, 1))
        lib.check(L.amt_domain_sync(h))
    finally:
        if how == "wrap":
            lib.check(L.amt_domain_destroy(h))
    for sset in seq:
        H.apply(want, None, H.SCALAR_SETS[sset])
        oracle.advance_mu_t(*want.args())
    _assert_outputs(pkg, dev.to_host(), want, f"{how}d handle, scalars {seq}")


def _stepper_sweeps(pkg, oracle, torch_mod, st, dev, want, seed, seq, columns):
    from wrf_model_cuda_sample_amd import lib
    dtype = np.float64 if dev.arrays["t_1"].dtype == torch_mod.float64 else np.float32
    try:
        for sweep, sset in enumerate(seq):
            if sweep:
                st.next_substep_inputs(seed, sweep)
            lib.check(st.L.amt_domain_set_scalars(st._dom, *_scalars_of(sset, dtype)))
            st.step(1)
        st.sync()
    finally:
        st.close()
    S = pkg.synth
    for sweep, sset in enumerate(seq):
        if sweep:
            S.refresh_exchanged_inputs(want, seed, sweep)
        loopback_halos_by_hand(pkg, want, columns=columns)
        H.apply(want, None, H.SCALAR_SETS[sset])
        oracle.advance_mu_t(*want.args())


@pytest.mark.parametrize("transport", ["rccl", "ipc"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_slab_stepper_in_loopback(pkg, oracle, torch_mod, dtype, transport):
    """The middle slab of three, its own neighbour (amt_slab_*: the edge rows beside the exchange, the interior beside them);
    new scalars through amt_domain_set_scalars before each sweep."""
    S = pkg.synth
    gdims = (200, 41, 60)
    b = S.slab_bounds(S.domain_bounds(*gdims, aligned=True), 1, 3)
    dev = S.make_patch(b, pkg.GridConfig(), dtype=dtype, seed=23, global_dims=gdims, device="cuda:0")
    H.apply(dev, H.levels_for(dev, 23), H.SCALAR_SETS[SETS[1]])
    want = dev.to_host()
    S.poison_halos(dev, S.SIDE_BELOW | S.SIDE_ABOVE)
    torch_mod.cuda.synchronize()
    st = pkg.patch.NativeSlabStepper(dev, 0, 1, pkg.patch.NativeSlabStepper.comm_unique_id(), loopback=True, transport=transport)
    _stepper_sweeps(pkg, oracle, torch_mod, st, dev, want, 23, [SETS[1], SETS[0], SETS[3]], columns=False)
    got = dev.to_host()
    for n in S.OUTPUTS:
        assert bits_equal(got.arrays[n][1:-1], want.arrays[n][1:-1]), f"slab ({transport}): {n} differs from the oracle"


@pytest.mark.parametrize("transport", ["rccl", "ipc"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_grid_stepper_in_loopback(pkg, oracle, torch_mod, dtype, transport):
    """The middle patch of 3 x 3, its own neighbour on all four sides (amt_grid_*: packed halo columns)."""
    S = pkg.synth
    gdims = (190, 37, 45)
    pb = S.patch_bounds(S.domain_bounds(*gdims), 1, 1, 3, 3, align_elems=32)
    dev = S.make_patch(pb, pkg.GridConfig(), dtype=dtype, seed=41, global_dims=gdims, device="cuda:0")
    H.apply(dev, H.levels_for(dev, 41), H.SCALAR_SETS[SETS[2]])
    want = dev.to_host()
    S.poison_halos(dev, 15)
    torch_mod.cuda.synchronize()
    st = pkg.patch.NativeGridStepper(dev, 0, 0, 1, 1, pkg.patch.NativeGridStepper.comm_unique_id(), loopback=True,
                                     transport=transport)
    _stepper_sweeps(pkg, oracle, torch_mod, st, dev, want, 41, [SETS[2], SETS[3], SETS[0]], columns=True)
    got = dev.to_host()
    own = (slice(1, -1), Ellipsis, slice(pb.its - pb.ims, pb.ite - pb.ims + 1))
    for n in S.OUTPUTS:
        assert bits_equal(got.arrays[n][own], want.arrays[n][own]), f"grid ({transport}): {n} differs from the oracle"


def test_2x2_processes_on_wrf_levels(pkg, oracle, tmp_path):
    dims = (300, 41, 80)
    outs = run_grid_ranks(tmp_path, 2, 2, dims, sweeps=3, specified=True, hard="rk3_dx12km")
    assert all("transport ipc, ranks seen 4" in o for o in outs), outs
    bad = grid_mismatches(pkg, oracle, tmp_path, 2, 2, dims, "f64", 3, True, 32, hard="rk3_dx12km")
    assert not bad, f"(rank, array) pairs that differ from the unsplit oracle run: {bad}"


def test_headline_sweep_through_a_created_handle(pkg, oracle, torch_mod):
    """4096 x 60 x 4096 fp64 through amt_domain_create with dts = 20/3 and WRF-like metrics: the headline plan (several rounds of
    workgroups) only runs at this size.  64-row j chunks against the oracle, as test_gpu_13_fullsize does: both domain edges and
    chunks across the workgroups' j-block boundaries."""
    from test_gpu_13_fullsize import _granted_cores
    from wrf_model_cuda_sample_amd import lib
    S, L = pkg.synth, pkg.load_library()
    dims = (4096, 60, 4096)
    b = S.domain_bounds(*dims, aligned=True)
    need = 10 * b.idim * b.kdim * b.jdim * 8 * 1.05
    if torch_mod.cuda.mem_get_info(0)[0] < need:
        pytest.skip(f"needs {need / 1e9:.0f} GB of free HBM")
    cfg = pkg.GridConfig(specified=True)
    dev = S.make_patch(b, cfg, dtype=np.float64, seed=4343, device="cuda:0", native_domain=True)
    levels = H.levels_for(dev, 4343)
    H.apply(dev, levels, H.SCALAR_SETS["rk3_dx12km"])
    torch_mod.cuda.synchronize()
    h = dev.owner.handle
    lib.check(L.amt_domain_set_scalars(h, dev.rdx, dev.rdy, dev.dts, dev.epssm))
    lib.check(L.amt_domain_step(h, 1))
    lib.check(L.amt_domain_sync(h))
    label = L.amt_march_last_kernel().decode()
    m = re.search(r"jrows=(\d+)", label)
    jrows = int(m.group(1)) if m else 32
    t0 = time.time()
    rows, first_row = 64, 2
    nblk = -(-(dims[2] - 2) // jrows)
    bnd = [first_row + jrows * k for k in sorted({1, nblk // 3, (2 * nblk) // 3, nblk - 1}) if 1 <= k < nblk]
    starts = sorted({1, dims[2] - rows + 1} | {x - rows // 2 for x in bnd if x + rows // 2 <= dims[2]})
    threads = _granted_cores(rows)
    for jlo in starts:
        jhi = jlo + rows - 1
        sb = b.replace(jms=jlo - 1, jme=jhi + 1, jts=jlo, jte=jhi)
        want = S.make_patch(sb, cfg, dtype=np.float64, seed=4343, global_dims=dims, device="cuda:0").to_host()
        H.apply(want, levels, H.SCALAR_SETS["rk3_dx12km"])
        oracle.advance_mu_t_omp(*want.args(), nthreads=threads)
        for n in S.OUTPUTS:
            got = dev.arrays[n][jlo - b.jms: jhi + 1 - b.jms].cpu().numpy()
            assert bits_equal(got, want.arrays[n][1:-1]), f"rows {jlo}..{jhi}: {n} differs from the oracle ({label})"
    slow_note("headline rows on WRF-like levels against the oracle", time.time() - t0, 90)
