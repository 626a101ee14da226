"""Parity tests proper (need an MI355X): every entry point of the C-ABI against the oracle
on the same seeded inputs, bit-exact -- the kernels keep the Fortran operation order and are
built with -ffp-contract=off, so the 1e-12 relative tolerance of BASELINE.json's north_star is
met with zero error; a tolerance check is kept next to the bit check so that a failure
reports how far off it is.  At BASELINE.json's full size the oracle cannot hold the domain,
so size-independent properties are used: randomly placed j-slabs recomputed by the oracle
from regenerated inputs, tile-split invariance and variant agreement."""
import numpy as np
import pytest

import cases
from conftest import bits_equal

pytestmark = pytest.mark.gpu

REL_TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-5}   # north_star: 1e-12 rel (fp64)


def max_rel(a, b):
    """The reference's metric (advance_mu_t_driver.f90:288-300, common.cu:117-141)."""
    a = a.astype(np.float64).ravel()
    b = b.astype(np.float64).ravel()
    both = (a != 0) & (b != 0)
    m = np.maximum(np.abs(a), np.abs(b))
    rel = np.where(both, np.abs(a - b) / np.where(m == 0, 1, m), m)
    return float(rel.max()) if rel.size else 0.0


def assert_patch_equal(pkg, got, want, what):
    for n in pkg.synth.FIELD_NAMES:
        g, w = np.asarray(got.arrays[n]), np.asarray(want.arrays[n])
        if not bits_equal(g, w):
            r = max_rel(g, w)
            tol = REL_TOL[w.dtype]
            nbad = int((g != w).sum())
            raise AssertionError(f"{what}: {n} not bit-identical to the oracle "
                                 f"({nbad} elements differ, max rel err {r:.3e}, tolerance {tol:g})")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def variants(pkg):
    return [pkg.VARIANT_COLUMN, pkg.VARIANT_MARCH, pkg.VARIANT_AUTO]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("flag", sorted(cases.FLAG_COMBOS))
@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_device_call_matches_oracle(pkg, oracle, torch_mod, shape, flag, dtype):
    host = cases.make_case(pkg, shape, flag, dtype)
    want = host.copy()
    oracle.advance_mu_t(*want.args())
    for variant in variants(pkg):
        dev = host.to_device("cuda:0")
        try:
            pkg.advance_mu_t(*dev.args(), variant=variant)
        except pkg.AmtError as e:
            if variant == pkg.VARIANT_MARCH and e.status == 3:
                continue           # shape not supported by this variant (AUTO falls back)
            raise
        torch_mod.cuda.synchronize()
        assert_patch_equal(pkg, dev.to_host(), want, f"{shape}/{flag}/{np.dtype(dtype).name}/variant{variant}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape,flag", [("16x8x16", "none"), ("64x40x64", "specified"),
                                        ("130x3x7_tile", "none"), ("37x5x11_ragged", "nested")])
def test_one_shot_host_call_matches_oracle(pkg, oracle, shape, flag, dtype):
    """amt_advance_mu_t_f32/_f64: host arrays in, host arrays out (the true drop-in)."""
    p = cases.make_case(pkg, shape, flag, dtype)
    want = p.copy()
    oracle.advance_mu_t(*want.args())
    pkg.advance_mu_t(*p.args())
    assert_patch_equal(pkg, p, want, f"one-shot {shape}/{flag}")


@pytest.mark.parametrize("mode", ["default", "no-pack", "no-thread", "plain"])
@pytest.mark.parametrize("rows", [1, 5, 13, 1000])
def test_streamed_one_shot_chunks_match_oracle(pkg, oracle, monkeypatch, rows, mode):
    """The one-shot drop-in streams the window in j chunks (upload, compute and download streams,
    two device buffer sets; pageable arrays: a download thread, small arrays packed through a
    staging buffer); any chunking and any of the regimes must give the oracle's bits."""
    monkeypatch.setenv("AMT_STREAM_ROWS", str(rows))
    if mode in ("no-pack", "plain"):
        monkeypatch.setenv("AMT_STREAM_PACK", "0")
    if mode in ("no-thread", "plain"):
        monkeypatch.setenv("AMT_STREAM_THREAD", "0")
    for flag in ("none", "specified"):
        p = cases.make_case(pkg, "64x40x64", flag, np.float64)
        want = p.copy()
        oracle.advance_mu_t(*want.args())
        pkg.advance_mu_t(*p.args())
        assert_patch_equal(pkg, p, want, f"streamed one-shot rows={rows} {flag}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_shot_touches_only_window_cells_of_the_3d_outputs(pkg, oracle, monkeypatch, dtype):
    """ww, t, t_ave come back as window-only strided copies (t_ave and all but level 1 of ww are
    never uploaded): every host cell outside i_start..i_end x 1..k_end x j_start..j_end -- halo
    columns, level kte, rows outside the tile -- must keep its bit pattern, NaN canaries included."""
    monkeypatch.setenv("AMT_STREAM_ROWS", "7")
    S = pkg.synth
    b = S.domain_bounds(70, 12, 30).replace(jts=4, jte=25, its=3, ite=66)
    p = S.make_patch(b, pkg.GridConfig(specified=True), dtype=dtype, seed=19)
    win = pkg.compute_window(p.config, b.ids, b.ide, b.jds, b.jde, b.its, b.ite, b.jts, b.jte, b.kts, b.kte)
    for n in ("ww", "t", "t_ave"):
        a = p.arrays[n]
        canary = np.full(a.shape, np.nan, dtype=dtype)
        inside = np.zeros(a.shape, dtype=bool)
        i0, i1, j0, j1 = win[0], win[1], win[2], win[3]
        inside[j0 - b.jms:j1 - b.jms + 1, 1 - b.kms:b.kte - b.kms, i0 - b.ims:i1 - b.ims + 1] = True
        if n == "t_ave":
            a[...] = np.where(inside, 0, canary)               # written everywhere inside
        elif n == "ww":
            lvl1 = np.zeros(a.shape, dtype=bool)
            lvl1[:, 1 - b.kms, :] = True
            a[...] = np.where(inside & lvl1, a, np.where(inside, np.nan, canary))   # only level 1 is an input
        else:
            a[...] = np.where(inside, a, canary)
    want = p.copy()
    oracle.advance_mu_t(*want.args())
    pkg.advance_mu_t(*p.args())
    assert_patch_equal(pkg, p, want, "window-only download")
    for n in ("ww", "t", "t_ave"):
        assert np.isfinite(p.arrays[n][win[2] - b.jms:win[3] - b.jms + 1, 1 - b.kms:b.kte - b.kms,
                                       win[0] - b.ims:win[1] - b.ims + 1]).all(), n


def test_one_shot_from_concurrent_host_threads(pkg, oracle):
    """WRF calls advance_mu_t from OpenMP tile threads: four host threads, each with its own
    j-tile of the SAME host arrays, at the same time.  Each thread has its own device workspace
    (amt_host_release frees it); tiles write disjoint cells, so the union must be the oracle's
    whole-domain result."""
    import threading
    from wrf_model_cuda_sample_amd import lib
    L = pkg.load_library()
    S = pkg.synth
    b = S.domain_bounds(150, 20, 64)
    p = S.make_patch(b, pkg.GridConfig(specified=True), seed=77)
    want = p.copy()
    oracle.advance_mu_t(*want.args())
    errors = []

    def tile(jts, jte):
        try:
            pkg.advance_mu_t(*p.with_bounds(jts=jts, jte=jte).args())
            lib.check(L.amt_host_release())
        except Exception as e:                      # noqa: BLE001
            errors.append(e)

    edges = [1, 17, 33, 49, b.jde]
    threads = [threading.Thread(target=tile, args=(edges[n], edges[n + 1] - 1 if n < 3 else b.jde)) for n in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert_patch_equal(pkg, p, want, "four concurrent tile threads")


@pytest.mark.parametrize("pack", ["1", "0"], ids=["packed", "per-array"])
def test_one_shot_from_threads_on_tiles_split_in_i(pkg, oracle, monkeypatch, pack):
    """tiles that split i share their j rows.  The 2-D outputs come back as the window's
    cells only in every regime (staged scatter, or a strided copy per array when AMT_STREAM_PACK=0 /
    pinned small arrays), so a thread never rewrites a neighbour tile's freshly computed columns
    with the values it uploaded.  Repeated to give the race a chance."""
    import threading
    monkeypatch.setenv("AMT_STREAM_PACK", pack)
    S = pkg.synth
    b = S.domain_bounds(200, 12, 40)
    for rep in range(6):
        p = S.make_patch(b, pkg.GridConfig(), seed=300 + rep)
        want = p.copy()
        oracle.advance_mu_t(*want.args())
        errors = []

        def tile(its, ite):
            try:
                pkg.advance_mu_t(*p.with_bounds(its=its, ite=ite).args())
            except Exception as e:                      # noqa: BLE001
                errors.append(e)

        edges = [1, 37, 101, 150, b.ide + 1]
        threads = [threading.Thread(target=tile, args=(edges[n], edges[n + 1] - 1)) for n in range(4)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        assert_patch_equal(pkg, p, want, f"four concurrent i-tiles, rep {rep}")
    pkg.load_library().amt_host_release()


def test_streamed_one_shot_with_pinned_host_arrays(pkg, oracle):
    """amt_host_pin on the ten 3-D arrays switches the one-shot call to the chunked three-stream
    pipeline (default chunk size); results must not change."""
    import ctypes
    from wrf_model_cuda_sample_amd import lib
    L = pkg.load_library()
    S = pkg.synth
    p = S.make_patch(S.domain_bounds(700, 60, 150), pkg.GridConfig(nested=True), seed=8)   # ~43 MB per 3-D array
    want = p.copy()
    oracle.advance_mu_t_omp(*want.args(), nthreads=8)
    pinned = []
    try:
        for n in S.RANK3:
            a = p.arrays[n]
            lib.check(L.amt_host_pin(a.ctypes.data_as(ctypes.c_void_p), a.nbytes))
            pinned.append(a)
        pkg.advance_mu_t(*p.args())
    finally:
        for a in pinned:
            lib.check(L.amt_host_unpin(a.ctypes.data_as(ctypes.c_void_p)))
    assert_patch_equal(pkg, p, want, "pinned streamed one-shot")


def test_fp32_run_against_fp64_oracle_at_stated_tolerance(pkg, oracle, torch_mod):
    """BASELINE.json configs[4]: an fp32 run judged against the fp64 Fortran.  Tolerance, stated:
    per output array, max |fp32 - fp64| <= 2e-5 * max |fp64| (a few fp32 ulps of the field scale,
    accumulated over the NK-level chains); element-wise relative error is meaningless here because
    ww and t pass through zero."""
    S = pkg.synth
    b = S.domain_bounds(256, 80, 96, aligned=True)
    dev = S.make_patch(b, pkg.GridConfig(specified=True), dtype=np.float32, seed=31, device="cuda:0")
    want = S.make_patch(b, pkg.GridConfig(specified=True), dtype=np.float64, seed=31)
    pkg.advance_mu_t(*dev.args())
    torch_mod.cuda.synchronize()
    oracle.advance_mu_t_omp(*want.args(), nthreads=8)
    got = dev.to_host()
    for n in S.OUTPUTS:
        w = want.arrays[n]
        err = np.abs(got.arrays[n].astype(np.float64) - w).max()
        assert err <= 2e-5 * np.abs(w).max(), (n, err, np.abs(w).max())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nk", [1, 2, 3, 5, 6, 7, 9, 27, 35, 45, 58, 59, 61, 70])
def test_ragged_level_counts_on_the_fast_path(pkg, oracle, torch_mod, nk, dtype):
    """Level counts that do not fill the cell waves (nk % KPT != 0) on the aligned resident layout,
    i.e. through the LDS-DMA flavour with virtual levels in its last wave: the top boundary
    wdtn(kde) = 0 (:221) then falls inside a wave, and nothing beyond level nk may be stored
    (level kte and the rows around keep their bits)."""
    S = pkg.synth
    b = S.domain_bounds(200, nk, 11, aligned=True)
    host = S.make_patch(b, pkg.GridConfig(specified=True), dtype=dtype, seed=100 + nk)
    want = host.copy()
    oracle.advance_mu_t(*want.args())
    dev = host.to_device("cuda:0")
    pkg.advance_mu_t(*dev.args(), variant=pkg.VARIANT_MARCH)
    torch_mod.cuda.synchronize()
    assert_patch_equal(pkg, dev.to_host(), want, f"ragged nk={nk}")


def test_empty_and_degenerate_windows(pkg, oracle, torch_mod):
    """Windows with no column (specified on a 2-cell-wide domain), one column, one row: the call
    succeeds, matches the oracle and leaves everything else untouched."""
    S = pkg.synth
    for dims, flags in (((2, 3, 2), dict(specified=True)),        # i_start=2 > i_end=1: nothing to do
                        ((3, 2, 5), dict(nested=True)),           # exactly one column in i
                        ((9, 4, 3), dict(specified=True)),        # exactly one row in j
                        ((1, 1, 1), dict())):                     # a single cell
        b = S.domain_bounds(*dims)
        host = S.make_patch(b, pkg.GridConfig(**flags), seed=2)
        want = host.copy()
        oracle.advance_mu_t(*want.args())
        for variant in variants(pkg):
            dev = host.to_device("cuda:0")
            pkg.advance_mu_t(*dev.args(), variant=variant)
            torch_mod.cuda.synchronize()
            assert_patch_equal(pkg, dev.to_host(), want, f"degenerate {dims} {flags} variant{variant}")
        one = host.copy()
        pkg.advance_mu_t(*one.args())
        assert_patch_equal(pkg, one, want, f"degenerate one-shot {dims} {flags}")


def test_against_committed_golden_vectors(pkg, torch_mod):
    """HIP path straight against tests/golden (outputs of the reference Fortran itself)."""
    small = cases.load_small()
    keys = sorted({k.rsplit("/", 1)[0] for k in small})
    for key in keys:
        shape, flag, dtname = key.split("/")
        dev = cases.make_case(pkg, shape, flag, np.dtype(dtname)).to_device("cuda:0")
        pkg.advance_mu_t(*dev.args())
        torch_mod.cuda.synchronize()
        got = dev.to_host()
        for n in pkg.synth.OUTPUTS:
            assert bits_equal(got.arrays[n], small[f"{key}/{n}"]), f"{key}/{n}"


@pytest.mark.parametrize("aligned", [False, True])
def test_512x60x512_fp64_matches_oracle(pkg, oracle, torch_mod, aligned):
    """BASELINE.json configs[1]: 512x60x512 fp64, validate to 1e-12 rel (here: bit-exact)."""
    S = pkg.synth
    b = S.domain_bounds(512, 60, 512, aligned=aligned)
    dev = S.make_patch(b, pkg.GridConfig(), dtype=np.float64, seed=2024, device="cuda:0")
    want = dev.to_host()
    oracle.advance_mu_t_omp(*want.args(), nthreads=8)
    for variant in variants(pkg):
        d2 = dev.copy()
        try:
            pkg.advance_mu_t(*d2.args(), variant=variant)
        except pkg.AmtError as e:
            if variant == pkg.VARIANT_MARCH and e.status == 3:
                continue
            raise
        torch_mod.cuda.synchronize()
        assert_patch_equal(pkg, d2.to_host(), want, f"512x60x512 aligned={aligned} variant{variant}")


def test_repeated_sweeps_stay_identical(pkg, oracle, torch_mod):
    """ww, t, mu are INOUT: five consecutive sweeps must track the oracle bit for bit."""
    host = cases.make_case(pkg, "64x40x64", "specified", np.float64)
    dev = host.to_device("cuda:0")
    want = host.copy()
    for _ in range(5):
        oracle.advance_mu_t(*want.args())
        pkg.advance_mu_t(*dev.args())
    torch_mod.cuda.synchronize()
    assert_patch_equal(pkg, dev.to_host(), want, "5 sweeps")


def test_tile_split_invariance(pkg, torch_mod):
    """One call over the domain == the same domain swept as 3x4 (i,j) tiles (what OpenMP
    tiling in WRF and the j-slab edge/interior launches rely on)."""
    S = pkg.synth
    b = S.domain_bounds(200, 12, 90, aligned=True)
    dev = S.make_patch(b, pkg.GridConfig(specified=True), seed=4, device="cuda:0")
    whole = dev.copy()
    pkg.advance_mu_t(*whole.args())
    i_edges = [1, 64, 130, 201]
    j_edges = [1, 20, 45, 70, 91]
    for a in range(3):
        for c in range(4):
            pkg.advance_mu_t(*dev.with_bounds(its=i_edges[a], ite=i_edges[a + 1] - 1 + (a == 2),
                                              jts=j_edges[c], jte=j_edges[c + 1] - 1 + (c == 3)).args())
    torch_mod.cuda.synchronize()
    assert_patch_equal(pkg, dev.to_host(), whole.to_host(), "tiled vs whole")


def test_resident_domain_handle(pkg, oracle, torch_mod):
    """amt_domain_*: native owner of the device arrays (what a C/Fortran host uses)."""
    import ctypes
    L = pkg.load_library()
    from wrf_model_cuda_sample_amd import lib
    S = pkg.synth
    b = S.domain_bounds(96, 16, 40, aligned=True)
    cfg = pkg.GridConfig(nested=True)
    h = ctypes.c_void_p()
    lib.check(L.amt_domain_create(ctypes.byref(h), 8, *cfg.as_ints(), *b.as_tuple()))
    try:
        lib.check(L.amt_domain_fill_synthetic(h, 11, b.ims, b.kms - 1, b.jms, 98, 17, 42))
        want = S.make_patch(b, cfg, seed=11)
        got0 = {}
        for n in S.FIELD_NAMES:
            a = np.empty(b.shape(n))
            lib.check(L.amt_domain_download(h, S.FIELD_ID[n], a.ctypes.data_as(ctypes.c_void_p)))
            got0[n] = a
            assert bits_equal(a, want.arrays[n]), n
        ms = ctypes.c_float()
        lib.check(L.amt_domain_step_timed(h, 3, ctypes.byref(ms)))
        assert ms.value > 0
        for _ in range(3):
            oracle.advance_mu_t(*want.args())
        for n in S.OUTPUTS:
            a = np.empty(b.shape(n))
            lib.check(L.amt_domain_download(h, S.FIELD_ID[n], a.ctypes.data_as(ctypes.c_void_p)))
            assert bits_equal(a, want.arrays[n]), n
        # upload round trip
        lib.check(L.amt_domain_upload(h, S.FIELD_ID["t"], got0["t"].ctypes.data_as(ctypes.c_void_p)))
        a = np.empty(b.shape("t"))
        lib.check(L.amt_domain_download(h, S.FIELD_ID["t"], a.ctypes.data_as(ctypes.c_void_p)))
        assert bits_equal(a, got0["t"])
    finally:
        lib.check(L.amt_domain_destroy(h))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_launch_beside_others_plans_two_rounds_and_the_same_bits(pkg, oracle, torch_mod, dtype):
    """AMT_LAUNCH_BESIDE_OTHERS (what the slab stepper's interior launch carries while the halo exchange runs): a launch that
    would be ONE round of workgroups on its own is planned in at least two, so that another stream's kernels get compute units
    at a round boundary; the results are the same bits."""
    import re
    torch = torch_mod
    S = pkg.synth
    L = pkg.load_library()
    cols = 64 if dtype == np.float64 else 128                       # columns per tile of the shapes chosen here
    b = S.domain_bounds(16 * cols, 20, 512)                         # 16 tiles x 512 rows: 256 blocks of 32 rows = one round
    host = S.make_patch(b, pkg.GridConfig(), dtype=dtype, seed=31)
    want = host.copy()
    oracle.advance_mu_t(*want.args())
    labels = {}
    for flag in (0, pkg.LAUNCH_BESIDE_OTHERS):
        dev = host.to_device("cuda:0")
        pkg.advance_mu_t(*dev.args(), variant=pkg.VARIANT_MARCH | flag)
        torch.cuda.synchronize()
        labels[flag] = L.amt_march_last_kernel().decode()
        assert_patch_equal(pkg, dev.to_host(), want, f"variant flag {flag:#x} ({labels[flag]})")
    rows = {f: int(re.search(r"jrows=(\d+)", lab).group(1)) for f, lab in labels.items()}
    ntile = -(-(b.ite - b.its + 1) // cols)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nj = b.jte - b.jts + 1
    blocks = {f: ntile * -(-nj // r) for f, r in rows.items()}
    if blocks[0] <= cus:                                            # the plain launch is one round on this device
        assert blocks[pkg.LAUNCH_BESIDE_OTHERS] > cus, (labels, blocks)
        assert rows[pkg.LAUNCH_BESIDE_OTHERS] < rows[0], labels


def test_placement_tuning_keeps_the_contents_and_a_working_handle(pkg, oracle, torch_mod):
    """amt_domain_tune_placement: the handle's arrays are re-allocated a few times and the fastest set kept -- every array
    must hold afterwards what it held before (inputs AND the in/out state the timed sweeps advanced), and the next
    sweep must be the oracle's."""
    import ctypes
    from wrf_model_cuda_sample_amd import lib
    L = pkg.load_library()
    S = pkg.synth
    b = S.domain_bounds(130, 20, 24, aligned=True)
    cfg = pkg.GridConfig(specified=True)
    h = ctypes.c_void_p()
    lib.check(L.amt_domain_create(ctypes.byref(h), 8, *cfg.as_ints(), *b.as_tuple()))
    try:
        lib.check(L.amt_domain_fill_synthetic(h, 5, b.ims, b.kms - 1, b.jms, 132, 21, 26))
        lib.check(L.amt_domain_sync(h))
        want = S.make_patch(b, cfg, dtype=np.float64, seed=5)
        before = {}
        for n in S.FIELD_NAMES:
            a = np.empty(b.shape(n), dtype=np.float64)
            lib.check(L.amt_domain_download(h, S.FIELD_ID[n], a.ctypes.data_as(ctypes.c_void_p)))
            before[n] = a
            assert bits_equal(a, want.arrays[n]), n
        ms = (ctypes.c_float * 4)()
        lib.check(L.amt_domain_tune_placement(h, 4, ms))
        assert ms[0] > 0 and all(m >= 0 for m in ms)
        for n in S.FIELD_NAMES:
            a = np.empty(b.shape(n), dtype=np.float64)
            lib.check(L.amt_domain_download(h, S.FIELD_ID[n], a.ctypes.data_as(ctypes.c_void_p)))
            assert bits_equal(a, before[n]), f"{n} changed by the tuning"
        lib.check(L.amt_domain_step(h, 1))
        lib.check(L.amt_domain_sync(h))
        oracle.advance_mu_t(*want.args())
        for n in S.OUTPUTS:
            a = np.empty(b.shape(n), dtype=np.float64)
            lib.check(L.amt_domain_download(h, S.FIELD_ID[n], a.ctypes.data_as(ctypes.c_void_p)))
            assert bits_equal(a, want.arrays[n]), n
    finally:
        lib.check(L.amt_domain_destroy(h))


def test_slab_stepper_single_rank_on_gpu(pkg, torch_mod):
    """world = 1 through the SlabStepper == a direct call (the N=1 bench path)."""
    S = pkg.synth
    b = S.slab_bounds(S.domain_bounds(128, 10, 50, aligned=True), 0, 1)
    dev = S.make_patch(b, seed=3, global_dims=(128, 10, 50), device="cuda:0")
    ref = dev.copy()
    pkg.patch.SlabStepper(dev, 0, 1, pkg.advance_mu_t).step()
    pkg.advance_mu_t(*ref.args())
    torch_mod.cuda.synchronize()
    assert_patch_equal(pkg, dev.to_host(), ref.to_host(), "stepper world=1")


@pytest.mark.parametrize("world,overlap", [(2, True), (3, True), (4, False)])
def test_slab_steppers_on_one_gpu_reproduce_the_unsplit_domain(pkg, torch_mod, world, overlap):
    """The N > 1 sweep logic on a real GPU: `world` slabs of one domain, each with its own
    SlabStepper (comm stream, interior launch overlapped with the exchange, edge rows after it),
    all in this process; the RCCL send/recv is replaced by device-to-device copies of the same
    rows.  Halo rows start as NaN, so only a correct exchange + ordering gives the unsplit result."""
    import torch
    S = pkg.synth
    dims = (200, 20, 61)
    g = S.domain_bounds(*dims, aligned=True)
    cfg = pkg.GridConfig(specified=True)
    whole = S.make_patch(g, cfg, seed=5, device="cuda:0")
    slabs = []
    for r in range(world):
        sb = S.slab_bounds(g, r, world)
        pt = S.make_patch(sb, cfg, seed=5, global_dims=dims, device="cuda:0")
        for name in S.HALO_FROM_ABOVE:
            if r < world - 1:
                pt.arrays[name][-1].fill_(float("nan"))
        if r > 0:
            pt.arrays["t_1"][0].fill_(float("nan"))
        slabs.append(pt)

    def transport(st):
        a = st.patch.arrays
        if st.above is not None:
            up = slabs[st.above].arrays
            for name in S.HALO_FROM_ABOVE:
                a[name][-1].copy_(up[name][1], non_blocking=True)
        if st.below is not None:
            a["t_1"][0].copy_(slabs[st.below].arrays["t_1"][-2], non_blocking=True)

    steppers = [pkg.patch.SlabStepper(slabs[r], r, world, pkg.advance_mu_t, overlap=overlap, transport=transport)
                for r in range(world)]
    for _ in range(3):
        pkg.advance_mu_t(*whole.args())
        for st in steppers:
            st.step()
    torch.cuda.synchronize()
    ref = whole.to_host()
    for r in range(world):
        b = slabs[r].bounds
        got = slabs[r].to_host()
        for n in S.OUTPUTS:
            assert bits_equal(got.arrays[n][1:-1], ref.arrays[n][b.jts - g.jms: b.jte - g.jms + 1]), (r, n)


def test_full_size_slab_properties(pkg, oracle, torch_mod):
    """BASELINE.json configs[2] shape in i and k (4096 x 60) on as many rows as fit quickly:
    the oracle recomputes randomly placed 3-row j-slabs from regenerated inputs."""
    S = pkg.synth
    ni, nk, nj = 4096, 60, 96
    b = S.domain_bounds(ni, nk, nj, aligned=True)
    dev = S.make_patch(b, seed=9, dtype=np.float64, device="cuda:0")
    pkg.advance_mu_t(*dev.args())
    torch_mod.cuda.synchronize()
    rng = np.random.default_rng(1)
    for jlo in [1, nj - 2] + [int(x) for x in rng.integers(2, nj - 3, 3)]:
        sb = b.replace(jms=jlo - 1, jme=jlo + 3, jts=jlo, jte=jlo + 2)
        want = S.make_patch(sb, seed=9, global_dims=(ni, nk, nj))
        oracle.advance_mu_t_omp(*want.args(), nthreads=3)
        for n in S.OUTPUTS:
            got = dev.arrays[n][jlo - b.jms: jlo + 3 - b.jms].cpu().numpy()
            assert bits_equal(got, want.arrays[n][1:4]), (jlo, n)


@pytest.mark.parametrize("dims,dtype", [((4096, 60, 1024), np.float64), ((4096, 60, 4096), np.float64),
                                        ((8192, 80, 2048), np.float32), ((8192, 80, 8192), np.float32)],
                         ids=["quarter-f64", "configs2-4096x60x4096-f64", "configs4-quarter-8192x80-f32",
                              "configs4-8192x80x8192-f32"])
def test_large_domain_checksums_agree_across_kernels(pkg, oracle, torch_mod, dims, dtype):
    """Every cell of a large domain -- a quarter of BASELINE.json configs[2] (21 GB), configs[2]
    itself (4096 x 60 x 4096 fp64, 82 GB resident), a quarter of configs[4] and configs[4] itself
    (8192 x 80 x 8192 fp32, 219 GB resident; there the fp32 result is also held against the fp64 oracle
    at the stated tolerance):
    the production kernel in one launch, the same kernel swept as seven ragged j tiles (other block
    sizes, other prologues) and the simple column kernel must leave bit-identical outputs -- compared
    through wrap-around integer checksums of the raw bit patterns -- and a few slabs are anchored to
    the oracle."""
    import torch
    S = pkg.synth
    b = S.domain_bounds(*dims, aligned=True)
    need = 10 * b.idim * b.kdim * b.jdim * np.dtype(dtype).itemsize * 1.1
    if torch.cuda.mem_get_info(0)[0] < need:
        pytest.skip(f"needs {need / 1e9:.0f} GB of free HBM")
    ibits = torch.int64 if dtype == np.float64 else torch.int32

    def run(variant, tiles):
        dev = S.make_patch(b, pkg.GridConfig(specified=True), dtype=dtype, seed=77, device="cuda:0")
        edges = np.linspace(1, dims[2] + 1, tiles + 1).astype(int)
        for a, c in zip(edges[:-1], edges[1:]):
            pkg.advance_mu_t(*dev.with_bounds(jts=int(a), jte=int(c) - 1 + (c == edges[-1])).args(), variant=variant)
        torch.cuda.synchronize()
        sums = {n: int(dev.arrays[n].view(ibits).sum(dtype=torch.int64).item()) for n in S.OUTPUTS}
        return dev, sums

    dev, auto = run(pkg.VARIANT_AUTO, 1)
    # anchor: three slabs against the oracle
    for jlo in (2, dims[2] // 2 - 1, dims[2] - 3):
        sb = b.replace(jms=jlo - 1, jme=jlo + 3, jts=jlo, jte=jlo + 2)
        want = S.make_patch(sb, pkg.GridConfig(specified=True), dtype=dtype, seed=77, global_dims=dims)
        oracle.advance_mu_t_omp(*want.args(), nthreads=3)
        for n in S.OUTPUTS:
            got = dev.arrays[n][jlo - b.jms: jlo + 3 - b.jms].cpu().numpy()
            assert bits_equal(got, want.arrays[n][1:4]), (jlo, n)
        if dtype == np.float32:
            # BASELINE.json configs[4]: the fp32 run against the fp64 Fortran, per output array
            # max|fp32 - fp64| <= 2e-5 * max|fp64|  (FP32_VS_FP64_TOL below)
            w64 = S.make_patch(sb, pkg.GridConfig(specified=True), dtype=np.float64, seed=77, global_dims=dims)
            oracle.advance_mu_t_omp(*w64.args(), nthreads=3)
            for n in S.OUTPUTS:
                got = dev.arrays[n][jlo - b.jms: jlo + 3 - b.jms].cpu().numpy().astype(np.float64)
                ref = w64.arrays[n][1:4]
                assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max(), (jlo, n)
    del dev
    torch.cuda.empty_cache()
    dev, tiled = run(pkg.VARIANT_MARCH, 7)        # ragged j tiles: other block sizes, other prologues
    assert tiled == auto
    del dev
    torch.cuda.empty_cache()
    dev, column = run(pkg.VARIANT_COLUMN, 1)
    assert column == auto
    del dev
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nk", [61, 76, 80, 88, 100, 120, 128, 133, 176, 200, 264, 300])
def test_many_levels_match_oracle(pkg, oracle, torch_mod, nk, dtype):
    """Level counts beyond the 60 of BASELINE.json (61..90 ran spilling kernels, beyond
    that the column kernel): whatever the launcher picks -- level groups of 2 or 4 per wave, 12- or
    16-wave builds, the column kernel past 264 levels -- against the oracle, aligned (LDS-DMA) and
    unaligned (register flavour) layouts; the column kernel alone as well (its LDS column passes
    64 KB at 129 levels in fp64)."""
    S = pkg.synth
    L = pkg.load_library()
    for aligned in (True, False):
        b = S.domain_bounds(150, nk, 5, aligned=aligned)
        host = S.make_patch(b, pkg.GridConfig(specified=True), dtype=dtype, seed=nk, global_dims=(150, nk, 5))
        want = host.copy()
        oracle.advance_mu_t(*want.args())
        for variant in (pkg.VARIANT_AUTO, pkg.VARIANT_COLUMN):
            dev = host.to_device("cuda:0")
            pkg.advance_mu_t(*dev.args(), variant=variant)
            torch_mod.cuda.synchronize()
            assert_patch_equal(pkg, dev.to_host(), want, f"nk={nk} aligned={aligned} variant={variant} "
                                                         f"({L.amt_march_last_kernel().decode()})")


def test_level_count_beyond_lds_is_refused(pkg, torch_mod):
    S = pkg.synth
    b = S.domain_bounds(64, 330, 3, aligned=True)
    dev = S.make_patch(b, pkg.GridConfig(), dtype=np.float64, seed=1, device="cuda:0")
    with pytest.raises(pkg.AmtError) as e:
        pkg.advance_mu_t(*dev.args())
    assert e.value.status == 2
    torch_mod.cuda.synchronize()
