"""GPU parity on special values (tests/special_values.py): exact and negative zeros, subnormals, overflow to Inf and Inf - Inf,
planted NaN / Inf / zero divisors and NaN in every cell the Fortran does not read.  Every path: each march instantiation forced,
both flavours of the column kernel and AUTO, the one-shot host call (plain, residency cache in check mode, deferred outputs,
three device slots), the resident handle, the ensemble launch and the non-finite guard on values the kernels computed.

Compared with the oracle on the same inputs: NaN at the same cells, every other cell of the window equal as bits (+-Inf, +-0,
subnormals), every cell outside the window and every array the routine only reads untouched, bit for bit
(special_values.same_up_to_nan_payload).  tests/test_special_values_cpu.py anchors the oracle on the reference
Fortran and holds the footprint table of the single plants."""
import numpy as np
import pytest

import diag_ref as R
import hard_inputs as H
import special_values as SV
from conftest import bits_equal
from test_gpu_11_shapes import SHAPES, _id
from test_gpu_24_diag import _Domain, _report_tuple

pytestmark = pytest.mark.gpu

FLAGS = [dict(), dict(specified=True), dict(specified=True, periodic_x=True), dict(nested=True)]
DTYPES = [np.float64, np.float32]
FIELD_ENUM = {"ww": 0, "mu": 6, "t": 13}                      # enum amt_field


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


def _base(pkg, b, cfg, dtype, seed, gdims):
    """WRF-like metrics and the rk3 scalars (dts = 20/3) under every regime, as special_values.base_case."""
    p = pkg.synth.make_patch(b, cfg, dtype=dtype, seed=seed, global_dims=gdims)
    return H.apply(p, H.levels_for(p, seed), H.SCALAR_SETS["rk3_dx12km"])


def _oracle(oracle, before, sweeps=1):
    want = before.copy()
    for _ in range(sweeps):
        oracle.advance_mu_t(*want.args())
    return want


def _assert_same(pkg, got, want, before, what):
    """got: the arrays after the call (numpy); want: the oracle's; before: the inputs."""
    for n in pkg.synth.FIELD_NAMES:
        g = np.asarray(got[n])
        if n in pkg.synth.OUTPUTS:
            assert SV.same_up_to_nan_payload(g, want.arrays[n]), \
                f"{what}: {n} differs from the oracle; first (index, got, want, cells): {SV.first_difference(g, want.arrays[n])}"
            assert SV.outside_window_bits_equal(before, n, g, before.arrays[n]), f"{what}: {n} changed outside the window"
        else:
            assert bits_equal(g, before.arrays[n]), f"{what}: the input {n} was written"


def _device_run(pkg, torch, before, variant):
    dev = before.to_device("cuda:0")
    pkg.advance_mu_t(*dev.args(), variant=variant)
    torch.cuda.synchronize()
    return dev.to_host().arrays


# ---------------------------------------------------------------------------------------------
# every march instantiation
# ---------------------------------------------------------------------------------------------
MARCH_REGIMES = ("signed_zeros", "denormal", "planted_composite", "unread_poison")


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_every_march_instantiation(pkg, oracle, force, torch_mod, shape):
    dtype, vw, kpt, hl, xd, dma, wm = shape
    S, L = pkg.synth, pkg.load_library()
    tc = (64 // hl) * vw
    ni, nj = 2 * tc + tc // 2 + 3, 7
    nk = min(2 * kpt * hl + 1, (wm - 1) * kpt * hl)
    for n, regime in enumerate(MARCH_REGIMES):
        cfg = pkg.GridConfig(**FLAGS[n % 4])
        aligned = n % 2 == 0
        b = S.domain_bounds(ni, nk, nj, aligned=aligned)
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
        before = _base(pkg, b, cfg, dtype, 700 + nk, (ni, nk, nj))
        w0 = SV.window(before)[0]
        # the last column of a tile, the first of the next (the tile's halo column), and the same at the second boundary
        kw = dict(columns=(w0 + tc - 1, w0 + tc, w0 + 2 * tc - 1, w0 + 2 * tc)) if regime == "planted_composite" else {}
        SV.apply(before, regime, SV.SEED, **kw)
        want = _oracle(oracle, before)
        for jrows in (0, 3):
            force(vw, kpt, hl, xd, dma, jrows, wm)
            got = _device_run(pkg, torch_mod, before, pkg.VARIANT_MARCH)
            name = L.amt_march_last_kernel().decode()
            assert f", {vw}, {kpt}, {hl}, {xd}, FULL, {'true' if dma else 'false'}, {wm}, " in name, name
            _assert_same(pkg, got, want, before, f"{_id(shape)} nk={nk} aligned={aligned} jrows={jrows} {regime} ({name})")


# ---------------------------------------------------------------------------------------------
# the column kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", SV.REGIMES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_column_kernel_and_auto(pkg, oracle, torch_mod, monkeypatch, dtype, regime):
    """The LDS flavour at 9 levels, RECOMPUTE at 61, and the launcher's own choice (AUTO) at both."""
    S = pkg.synth
    for n, (nk, recompute) in enumerate(((9, "0"), (61, "1"))):
        b = S.domain_bounds(37, nk, 11, aligned=bool(n % 2))
        cfg = pkg.GridConfig(**FLAGS[(n + SV.REGIMES.index(regime)) % 4])
        before = SV.apply(_base(pkg, b, cfg, dtype, 800 + nk, (37, nk, 11)), regime, SV.SEED)
        want = _oracle(oracle, before)
        monkeypatch.setenv("AMT_COLUMN_RECOMPUTE", recompute)
        got = _device_run(pkg, torch_mod, before, pkg.VARIANT_COLUMN)
        _assert_same(pkg, got, want, before, f"column kernel nk={nk} recompute={recompute} {regime}")
        monkeypatch.delenv("AMT_COLUMN_RECOMPUTE")
        got = _device_run(pkg, torch_mod, before, pkg.VARIANT_AUTO)
        label = pkg.load_library().amt_march_last_kernel().decode()
        _assert_same(pkg, got, want, before, f"AUTO nk={nk} {regime} ({label})")


@pytest.mark.parametrize("dtype", DTYPES)
def test_column_kernel_on_every_single_plant(pkg, oracle, torch_mod, dtype):
    """One field at a time on 37x5x11_ragged: a NaN, +Inf, -Inf (0.0 for the divisors) in an interior cell, in the first and
    last window column and row, and in each halo cell the stencil reads.  The oracle's footprint of each is the table of
    tests/test_special_values_cpu.py."""
    import torch
    base = SV.base_case(pkg, SV.PLANT_SHAPE, "none", dtype)
    dev = base.to_device("cuda:0")
    keep = {n: dev.arrays[n].clone() for n in pkg.synth.FIELD_NAMES}
    for field, value, where in SV.single_plants():
        before = SV.planted(base.copy(), field, value, where)
        want = _oracle(oracle, before)
        for n in pkg.synth.OUTPUTS + (field,):
            dev.arrays[n].copy_(torch.from_numpy(before.arrays[n]))
        pkg.advance_mu_t(*dev.args(), variant=pkg.VARIANT_COLUMN)
        got = {n: dev.arrays[n].cpu().numpy() for n in pkg.synth.FIELD_NAMES}
        _assert_same(pkg, got, want, before, f"column kernel, {field} = {value} at {where} {SV.site(before, field, where)}")
        dev.arrays[field].copy_(keep[field])


# ---------------------------------------------------------------------------------------------
# the one-shot host call
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "cached", "deferred", "three-slots"])
@pytest.mark.parametrize("regime", ["signed_zeros", "overflow", "planted_composite"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_shot_call(pkg, oracle, torch_mod, dtype, regime, mode):
    """Two calls on the same host arrays.  A NaN or Inf the routine computes is a legitimate output: the check mode of the
    residency cache must neither refuse it nor take it for (or replace it by) one of its canaries; cells of the host arrays
    outside the window keep their bits."""
    S = pkg.synth
    b = S.domain_bounds(37, 41, 11)
    before = SV.apply(_base(pkg, b, pkg.GridConfig(nested=True), dtype, 61, (37, 41, 11)), regime, SV.SEED)
    got = before.copy()
    try:
        if mode in ("cached", "deferred"):
            pkg.host_cache_enable(True, check=True)
        if mode == "deferred":
            pkg.host_defer(None, True)
        if mode == "three-slots":
            pkg.host_set_devices([0, 0, 0])
        for sweep in (1, 2):
            pkg.advance_mu_t(*got.args())
            if mode == "deferred":
                pkg.host_fetch(None)
            want = _oracle(oracle, before, sweeps=sweep)
            _assert_same(pkg, got.arrays, want, before, f"one-shot ({mode}) {regime} call {sweep}")
    finally:
        if mode == "three-slots":
            pkg.host_set_devices(())
        if mode == "deferred":
            pkg.host_defer(None, False)
        if mode in ("cached", "deferred"):
            pkg.host_cache_enable(False, check=False)
        pkg.load_library().amt_host_release()


# ---------------------------------------------------------------------------------------------
# the resident handle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["rest", "signed_zeros", "denormal"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_resident_handle_three_sweeps(pkg, oracle, torch_mod, dtype, regime):
    S = pkg.synth
    aligned = dtype is np.float64
    b = S.domain_bounds(70, 13, 9, aligned=aligned)
    before = SV.apply(_base(pkg, b, pkg.GridConfig(specified=True), dtype, 19, (70, 13, 9)), regime, SV.SEED)
    want = _oracle(oracle, before, sweeps=3)
    dm = _Domain(pkg, before)
    dm.dom.step(3)
    dm.dom.sync()
    got = {n: dm.download(n) for n in S.FIELD_NAMES}
    _assert_same(pkg, got, want, before, f"amt_domain_create, three sweeps of {regime}")
    if regime == "rest":
        for n in ("ww", "t", "mu"):
            assert not np.ascontiguousarray(got[n][SV.window_index(before, n)]).view(np.uint8).any(), f"{n}: a run at rest holds something but +0.0"


# ---------------------------------------------------------------------------------------------
# the ensemble
# ---------------------------------------------------------------------------------------------
ENSEMBLE_REGIMES = ("rest", "denormal", "overflow", "planted_composite", "signed_zeros")
FINITE_MEMBERS = (0, 1, 4)


def _ensemble_members(pkg, dtype, regimes, seed):
    S = pkg.synth
    b = S.domain_bounds(70, 13, 9, aligned=True)
    ps = []
    for m, regime in enumerate(regimes):
        p = SV.apply(_base(pkg, b, pkg.GridConfig(), dtype, seed, (70, 13, 9)), regime, SV.SEED + m)
        p.dts = abs(p.dts)                                      # the scalars are the ensemble's, not a member's
        ps.append(p)
    for p in ps[1:]:
        for n in S.RANK1:
            p.arrays[n] = ps[0].arrays[n]
    return b, ps


@pytest.mark.parametrize("variant", ["march", "column"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_ensemble_of_five_regimes(pkg, oracle, torch_mod, dtype, variant):
    """One launch per sweep, two sweeps; member 2 overflows, member 3 carries the planted NaN / Inf."""
    S = pkg.synth
    v = pkg.VARIANT_MARCH if variant == "march" else pkg.VARIANT_COLUMN
    b, ps = _ensemble_members(pkg, dtype, ENSEMBLE_REGIMES, 33)
    ens = pkg.Ensemble(b, len(ps), ps[0].config, dtype)
    try:
        for m, p in enumerate(ps):
            ens.upload_patch(m, p)
        ens.set_variant(v)
        ens.step(1)
        ens.step(1)
        ens.sync()
        got = [ens.download_patch(m) for m in range(len(ps))]
    finally:
        ens.close()
    for m, p in enumerate(ps):
        what = f"member {m} ({ENSEMBLE_REGIMES[m]}, {variant})"
        _assert_same(pkg, got[m], _oracle(oracle, p, sweeps=2), p, what)
        dev = p.to_device("cuda:0")
        for _ in range(2):
            pkg.advance_mu_t(*dev.args(), variant=v)
        torch_mod.cuda.synchronize()
        alone = dev.to_host().arrays
        for n in S.OUTPUTS:
            assert SV.same_up_to_nan_payload(got[m][n], alone[n]), f"{what}: {n} differs from the single-patch call on that member"
        if m in FINITE_MEMBERS:
            for n in S.OUTPUTS:
                assert np.isfinite(got[m][n]).all(), f"{what}: {n} is not finite: a neighbour's NaN or Inf leaked in"
        else:
            assert any(not np.isfinite(got[m][n]).all() for n in S.OUTPUTS), what


# ---------------------------------------------------------------------------------------------
# the guard on non-finite values the kernels computed
# ---------------------------------------------------------------------------------------------
def _first_finding(oracle, patches, sweeps):
    """(sweep, field, member, offset, n_nonfinite) of the first finding on the oracle's state: earliest sweep, then lowest
    member, then ww before t before mu (include/amt_advance_mu_t.h section 10); None when every sweep stays finite."""
    state = [p.copy() for p in patches]
    b = patches[0].bounds
    ext = (b.ims, b.ime, b.jms, b.jme, b.kms, b.kme)
    i0, i1, j0, j1, k0, k1 = SV.window(patches[0])
    for sweep in range(1, sweeps + 1):
        for p in state:
            oracle.advance_mu_t(*p.args())
        for m, p in enumerate(state):
            for n in ("ww", "t", "mu"):
                s = R.stats(p.arrays[n], ext, (i0, i1, k0, k1, j0, j1))
                if s["n_nan"] + s["n_inf"]:
                    return (sweep, FIELD_ENUM[n], m, s["first_nonfinite"], s["n_nan"] + s["n_inf"])
    return None


def test_guard_finds_the_first_overflow_of_a_domain(pkg, oracle, torch_mod):
    b = pkg.synth.domain_bounds(37, 13, 11)
    before = SV.apply(_base(pkg, b, pkg.GridConfig(), np.float32, 5, (37, 13, 11)), "overflow", SV.SEED)
    assert all(np.isfinite(a).all() for a in before.arrays.values())
    want = _first_finding(oracle, [before], 3)
    assert want is not None and want[0] == 1
    dm = _Domain(pkg, before)
    dm.dom.set_guard(1)
    assert dm.L.amt_domain_step(dm.handle, 3) == 0
    r = dm.dom.guard_report()
    print(f"  guard: {r!r}, the oracle's state gives {want}")
    assert _report_tuple(r) == want and r.sweeps_checked == 3
    with pytest.raises(pkg.AmtError) as e:
        dm.dom.sync()
    assert e.value.status == 7
    got = {n: dm.download(n) for n in pkg.synth.FIELD_NAMES}
    _assert_same(pkg, got, _oracle(oracle, before, sweeps=3), before, "the guarded domain after three sweeps")


def test_guard_finds_the_bad_member_of_an_ensemble(pkg, oracle, torch_mod):
    regimes = ("rest", "denormal", "overflow", "signed_zeros")
    b, ps = _ensemble_members(pkg, np.float32, regimes, 44)
    want = _first_finding(oracle, ps, 3)
    assert want is not None and want[2] == 2, want
    ens = pkg.Ensemble(b, len(ps), ps[0].config, np.float32)
    try:
        for m, p in enumerate(ps):
            ens.upload_patch(m, p)
        ens.set_guard(1)
        assert ens.L.amt_ensemble_step(ens.handle, 3) == 0
        r = ens.guard_report()
        print(f"  guard: {r!r}, the oracle's state gives {want}")
        assert _report_tuple(r) == want and r.sweeps_checked == 3
        ens.set_guard(0)
        ens.sync()
        for m in (0, 1, 3):
            for n in ("ww", "t", "mu"):
                assert np.isfinite(ens.download_member(n, m)).all(), f"member {m}: {n} is not finite"
    finally:
        ens.close()
