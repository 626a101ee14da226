"""The Fortran binding module held to the oracle through a Fortran program that USES it (tests/fortran/amt_binding_host.f90):
ensembles, cyclic refresh, the boundary zone, statistics / compare / guard, the host-owned halo exchange, the pointer-level
device calls and the one-shot call's control calls -- the interfaces no driver reaches.  The host fills its inputs with
amt_synth_fill_host / amt_*_fill_synthetic, this file with synth.make_patch of the same seed (tests/test_synth.py holds the two
identical); the host writes whole arrays and text records, this file compares every one of them: by bits against the oracle
and the numpy references (tests/cyclic_ref.py, tests/specbdy_ref.py, tests/diag_ref.py); only the statistics' `sum` is held to
math.fsum within diag_ref.sum_bound, the bound tests/test_gpu_24_diag.py uses.

Shapes: 70x13x9 fp64 and 133x9x7 fp32 on unpadded rows (ims:ime = 0:ni+1; the fp32 row is 135 long), 64x12x8 fp64 padded.  The
four scalars are not representable in fp32, so a REAL kind that is wrong anywhere on the way changes bits.  One host process at
a time, each with a timeout; a host that ends on a signal fails its test with its output shown."""
import ctypes
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch  # noqa: F401  -- before the HIP library initialises: both must share one HIP runtime (lib.py)

import cyclic_ref as CR
import diag_ref as DR
import specbdy_ref as SB
from conftest import bits_equal

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
HOST_DIR = ROOT / "tests" / "fortran"
SEED = 4321
MEMBERS = 3
SCALARS = (1.1e-3, 1.3e-3, 1.7, 0.1)                       # rdx, rdy, dts, epssm: none of them an fp32 number
F64, F32, F64_PADDED = (8, (70, 13, 9), False), (4, (133, 9, 7), False), (8, (64, 12, 8), True)
IDS = ["f64-70x13x9", "f32-133x9x7", "f64-64x12x8-padded"]
T, MU, FT = 13, 6, 16


@pytest.fixture(scope="module")
def host(pkg):
    r = subprocess.run(["make", "-C", str(HOST_DIR), "all"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"no Fortran toolchain: {r.stderr[-300:]}")
    return {4: HOST_DIR / "amt_binding_host_f32", 8: HOST_DIR / "amt_binding_host_f64"}


# ---------------------------------------------------------------------------------------------------------------------
# running the host, reading what it wrote
# ---------------------------------------------------------------------------------------------------------------------
def _scalars(itemsize):
    """The four scalars as this precision holds them (fp32: rounded once), as Python floats."""
    return tuple(float(np.float32(x)) if itemsize == 4 else x for x in SCALARS)


def _run_host(host, cmd, out, itemsize, b, cfg, dims, *, variant=0, extra=(), env=None):
    fmt = "%.17g" if itemsize == 8 else "%.9g"                  # both round-trip
    args = [str(host[itemsize]), cmd, str(out), str(MEMBERS), str(variant), *map(str, cfg.as_ints()), *map(str, b.as_tuple()),
            *map(str, dims), str(SEED), *[fmt % x for x in _scalars(itemsize)], *map(str, extra)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode >= 0, f"the host ended on signal {-r.returncode}:\n{r.stdout}\n{r.stderr}"
    assert r.returncode == 0, f"{' '.join(args)}\n{r.stdout}\n{r.stderr}"
    recs = [line.split() for line in (Path(out) / "records.txt").read_text().splitlines()]
    assert recs[0] == ["real_bytes", str(itemsize)] and recs[-1] == ["done"], recs
    return recs


def _dtype(itemsize):
    return np.float64 if itemsize == 8 else np.float32


def _patch(pkg, b, cfg, itemsize, dims, seed):
    p = pkg.synth.make_patch(b, cfg, dtype=_dtype(itemsize), seed=seed, global_dims=dims)
    p.rdx, p.rdy, p.dts, p.epssm = _scalars(itemsize)
    return p


def _members(pkg, b, cfg, itemsize, dims):
    return [_patch(pkg, b, cfg, itemsize, dims, SEED + m) for m in range(MEMBERS)]


def _load(pkg, out, stage, b, itemsize, members=None):
    """name -> array of one stage: (jdim, kdim, idim) / (jdim, idim) / (kdim,), member-stacked with `members`."""
    S, got = pkg.synth, {}
    for n in S.FIELD_NAMES:
        shape = b.shape(n) if members is None or S.field_rank(n) == 1 else (members, *b.shape(n))
        a = np.fromfile(Path(out) / f"{stage}_{n}.bin", dtype=_dtype(itemsize))
        assert a.size == int(np.prod(shape)), (stage, n, a.size, shape)
        got[n] = a.reshape(shape)
    return got


def _stack(pkg, patches):
    S = pkg.synth
    return {n: (patches[0].arrays[n].copy() if S.field_rank(n) == 1 else np.stack([p.arrays[n] for p in patches])) for n in S.FIELD_NAMES}


def _assert_all_fields(pkg, got, want, what):
    for n in pkg.synth.FIELD_NAMES:
        assert bits_equal(got[n], want[n]), f"{what}: {n} differs"


def _assert_members(pkg, got, patches, what):
    """Every field of every member, whole arrays: outputs against the oracle's, inputs unchanged."""
    S = pkg.synth
    for n in S.FIELD_NAMES:
        for m, p in enumerate(patches):
            g = got[n] if S.field_rank(n) == 1 else got[n][m]
            assert bits_equal(g, p.arrays[n]), f"{what}: {n} of member {m} differs"


def _value(recs, key):
    rows = [r for r in recs if r[0] == key]
    assert len(rows) == 1, (key, rows)
    return rows[0][1:]


def _f64(bits):
    return struct.unpack("<d", struct.pack("<q", int(bits)))[0]


def _cell(b, i, k, j):
    return (j - b.jms, k - b.kms, i - b.ims)


# ---------------------------------------------------------------------------------------------------------------------
# ensemble
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,flag", [(F64, "none"), (F32, "specified"), (F64_PADDED, "nested")], ids=IDS)
def test_ensemble_interfaces(pkg, oracle, host, tmp_path, case, flag):
    """Three members in Fortran 4-D / 3-D arrays: upload_member, two sweeps of amt_ensemble_step, a third through
    amt_advance_mu_t_ensemble_device_* on the handle's pointers and stream, a fourth through amt_ensemble_wrap over them; the
    single patch through amt_advance_mu_t_device_* and amt_domain_wrap.  Every field of every member against the oracle on that
    member alone; a device-filled second handle compares equal (n_diff = 0 per member and field)."""
    import cases
    itemsize, dims, aligned = case
    S, L = pkg.synth, pkg.load_library()
    cfg = pkg.GridConfig(**cases.FLAG_COMBOS[flag])
    b = S.domain_bounds(*dims, aligned=aligned)
    recs = _run_host(host, "ensemble", tmp_path, itemsize, b, cfg, dims)
    ps = _members(pkg, b, cfg, itemsize, dims)
    single = ps[0].copy()
    single.rdx, single.rdy, single.dts, single.epssm = _scalars(itemsize)
    assert _value(recs, "members") == [str(MEMBERS)]
    rows = [r for r in recs if r[0] == "ecompare"]
    assert len(rows) == MEMBERS * 22
    for _k, name, region, m, count, n_diff, first_diff, mad in rows:
        assert (int(region), int(count)) == (1, int(np.prod(b.shape(name)))), (name, m)
        assert (int(n_diff), int(first_diff), _f64(mad)) == (0, -1, 0.0), f"{name} of member {m}: uploaded and device-filled differ"
    for stage, sweeps in (("step2", 2), ("dev3", 1), ("wrap4", 1)):
        for p in ps:
            for _ in range(sweeps):
                oracle.advance_mu_t(*p.args())
        _assert_members(pkg, _load(pkg, tmp_path, stage, b, itemsize, MEMBERS), ps, f"{stage} ({flag})")
    for stage in ("one1", "one2"):
        oracle.advance_mu_t(*single.args())
        _assert_all_fields(pkg, _load(pkg, tmp_path, stage, b, itemsize), single.arrays, f"{stage} ({flag})")
    assert tuple(map(int, _value(recs, "window"))) == pkg.compute_window(cfg, b.ids, b.ide, b.jds, b.jde, b.its, b.ite, b.jts,
                                                                         b.jte, b.kts, b.kte)
    ntile = (b.ite - b.its) // 16 + 1
    assert int(_value(recs, "rows_for_members")[0]) == L.amt_march_rows_for_members(ntile, MEMBERS, b.jte - b.jts + 1, 256, 1000000, itemsize, 1) > 0
    assert int(_value(recs, "rows_for")[0]) == L.amt_march_rows_for(ntile, b.jte - b.jts + 1, 256, 1000000, itemsize, 1) > 0
    assert int(_value(recs, "placement")[0]) == 0               # a state this small is not sampled


# ---------------------------------------------------------------------------------------------------------------------
# cyclic
# ---------------------------------------------------------------------------------------------------------------------
def _plant_payload(arrays, b, itemsize):
    """A NaN with a payload into every cell a refresh writes or leaves (whole columns ide, ids-1 and rows jde, jds-1, corners
    included), in every member -- what the host's plant_cyclic_destinations does."""
    bits = np.array([0x7ff800000000beef], np.uint64).view(np.float64)[0] if itemsize == 8 else np.array([0x7fc0beef], np.uint32).view(np.float32)[0]
    c, r = (lambda i: i - b.ims), (lambda j: j - b.jms)
    for n in CR.COLS_FROM_RIGHT:
        arrays[n][..., c(b.ide)] = bits
    arrays["t_1"][..., c(b.ids - 1)] = bits
    for n in CR.ROWS_FROM_ABOVE:
        if n in CR.RANK3:
            arrays[n][..., r(b.jde), :, :] = bits
        else:
            arrays[n][..., r(b.jde), :] = bits
    arrays["t_1"][..., r(b.jds - 1), :, :] = bits


def _finite_window(pkg, arrays, b, flags, what):
    i0, i1, j0, j1 = CR.window(flags, b)
    for n in pkg.synth.OUTPUTS:
        a = arrays[n]
        v = a[..., j0 - b.jms:j1 - b.jms + 1, 0:b.kte - b.kms, i0 - b.ims:i1 - b.ims + 1] if a.ndim - (a.ndim > 3) == 3 and n in pkg.synth.RANK3 \
            else a[..., j0 - b.jms:j1 - b.jms + 1, i0 - b.ims:i1 - b.ims + 1]
        assert np.isfinite(v).all(), f"{what}: {n} is not finite over the whole window"


@pytest.mark.parametrize("case,flags,last_at_ide", [(F64, (0, 0, 0), True), (F32, (1, 0, 0), False)], ids=["f64-none", "f32-periodic_x"])
def test_cyclic_interfaces(pkg, oracle, host, tmp_path, case, flags, last_at_ide):
    """amt_domain_cyclic_fill alone, amt_cyclic_fill_device_* on the handle's pointers, amt_domain_set_cyclic(X+Y) read back and
    two sweeps, and the ensemble twins: against cyclic_ref, and the oracle on arrays cyclic_ref has wrapped before each sweep."""
    itemsize, dims, aligned = case
    S = pkg.synth
    cfg = pkg.GridConfig(periodic_x=bool(flags[0]))
    b = S.domain_bounds(*dims, aligned=aligned)
    if not last_at_ide:
        b = b.replace(ite=b.ide - 1, jte=b.jde - 1)
    recs = _run_host(host, "cyclic", tmp_path, itemsize, b, cfg, dims)
    axes = CR.CYCLIC_X | CR.CYCLIC_Y
    assert [_value(recs, k) for k in ("cyclic_after_fill", "cyclic_set", "ecyclic_after_fill", "ecyclic_set")] == [["0"], [str(axes)]] * 2
    ps = _members(pkg, b, cfg, itemsize, dims)
    for p in ps:
        _plant_payload(p.arrays, b, itemsize)
    # the single domain holds member 0
    filled = CR.cyclic_fill({n: a.copy() for n, a in ps[0].arrays.items()}, b, axes, flags)
    c, r = b.ide - b.ims, b.jde - b.jms
    assert np.isnan(filled["t_1"][r, :, c]).all() and not np.isnan(filled["u"][1:-1, :, c]).any()      # corners keep the payload
    for stage in ("fill", "ptr"):
        _assert_all_fields(pkg, _load(pkg, tmp_path, stage, b, itemsize), filled, f"{stage} {flags}")
    stacked = CR.cyclic_fill(_stack(pkg, ps), b, axes, flags)
    for stage in ("efill", "eptr"):
        _assert_all_fields(pkg, _load(pkg, tmp_path, stage, b, itemsize, MEMBERS), stacked, f"{stage} {flags}")
    for p in ps:
        for _ in range(2):
            CR.cyclic_fill(p.arrays, b, axes, flags)
            oracle.advance_mu_t(*p.args())
    _assert_all_fields(pkg, _load(pkg, tmp_path, "step", b, itemsize), ps[0].arrays, f"step {flags}")
    got = _load(pkg, tmp_path, "estep", b, itemsize, MEMBERS)
    _assert_members(pkg, got, ps, f"estep {flags}")
    _finite_window(pkg, got, b, flags, f"estep {flags}")


# ---------------------------------------------------------------------------------------------------------------------
# boundary zone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,flags", [(F64, (0, 1, 0)), (F32, (0, 0, 1))], ids=["f64-specified", "f32-nested"])
def test_boundary_zone_interfaces(pkg, oracle, host, tmp_path, case, flags):
    """amt_domain_spec_bdy_update alone, amt_spec_bdy_update_device_f64 / _f32 on the handle's pointers (dts = 1.7 is no fp32
    number: a wrong REAL kind changes the zone's bits), amt_domain_set_spec_bdy(1) read back and two sweeps, the ensemble twins:
    against specbdy_ref, and the oracle plus specbdy_ref per sweep."""
    itemsize, dims, aligned = case
    S = pkg.synth
    cfg = pkg.GridConfig(specified=bool(flags[1]), nested=bool(flags[2]))
    b = S.domain_bounds(*dims, aligned=aligned)
    recs = _run_host(host, "specbdy", tmp_path, itemsize, b, cfg, dims)
    assert [_value(recs, k) for k in ("spec_bdy_after_update", "spec_bdy_set", "espec_bdy_after_update", "espec_bdy_set")] == [["0"], ["1"]] * 2
    ps = _members(pkg, b, cfg, itemsize, dims)
    dts = ps[0].dts
    assert SB.zone_mask(flags, b).sum() == 2 * (dims[0] + dims[2]) - 4
    updated = SB.spec_bdy_update({n: a.copy() for n, a in ps[0].arrays.items()}, b, flags, dts)
    assert not bits_equal(updated["t"], ps[0].arrays["t"])
    for stage in ("upd", "ptr"):
        _assert_all_fields(pkg, _load(pkg, tmp_path, stage, b, itemsize), updated, f"{stage} {flags}")
    stacked = SB.spec_bdy_update(_stack(pkg, ps), b, flags, dts)
    for stage in ("eupd", "eptr"):
        _assert_all_fields(pkg, _load(pkg, tmp_path, stage, b, itemsize, MEMBERS), stacked, f"{stage} {flags}")
    for p in ps:
        for _ in range(2):
            oracle.advance_mu_t(*p.args())
            SB.spec_bdy_update(p.arrays, b, flags, dts)
    _assert_all_fields(pkg, _load(pkg, tmp_path, "step", b, itemsize), ps[0].arrays, f"step {flags}")
    _assert_members(pkg, _load(pkg, tmp_path, "estep", b, itemsize, MEMBERS), ps, f"estep {flags}")


# ---------------------------------------------------------------------------------------------------------------------
# statistics, compare, guard
# ---------------------------------------------------------------------------------------------------------------------
def _plant_specials(p):
    """What the host's plant_specials does, in every member alike."""
    b, a = p.bounds, p.arrays
    a["t"][_cell(b, b.its + 2, b.kts + 2, b.jts + 1)] = np.nan
    a["t"][_cell(b, b.its + 4, b.kts + 1, b.jts + 2)] = np.inf
    a["t"][_cell(b, b.its + 1, b.kts + 3, b.jts + 3)] = -np.inf
    a["t"][_cell(b, b.its + 3, b.kts + 2, b.jts + 2)] = -0.0
    a["mu"][b.jts + 2 - b.jms, b.its + 2 - b.ims] = np.nan
    a["mu"][b.jts + 1 - b.jms, b.its + 5 - b.ims] = -np.inf
    a["mu"][b.jts + 3 - b.jms, b.its + 3 - b.ims] = np.inf
    a["mu"][b.jts + 3 - b.jms, b.its + 1 - b.ims] = -0.0


def _plant_differences(p):
    b, a = p.bounds, p.arrays
    dt = a["t"].dtype.type
    a["t"][_cell(b, b.its + 3, b.kts + 2, b.jts + 2)] = 0.0
    a["t"][_cell(b, b.its + 6, b.kts + 1, b.jts + 1)] += dt(0.5)
    a["t"][_cell(b, b.its + 2, b.kts + 2, b.jts + 1)] = 1.0
    a["mu"][b.jts + 3 - b.jms, b.its + 1 - b.ims] = 0.0
    a["mu"][b.jts + 2 - b.jms, b.its + 4 - b.ims] -= dt(1.25)
    a["mu"][b.jts + 1 - b.jms, b.its + 6 - b.ims] *= dt(-1.0)


def _check_stats_row(row, want, what):
    count, n_nan, n_inf, first, mn, mx, mabs, total = row
    got = dict(count=int(count), n_nan=int(n_nan), n_inf=int(n_inf), first_nonfinite=int(first), min=_f64(mn), max=_f64(mx),
               max_abs=_f64(mabs), sum=_f64(total))
    print(f"  {what}: got {got}")
    for k in ("count", "n_nan", "n_inf", "first_nonfinite", "min", "max", "max_abs"):
        assert got[k] == want[k], f"{what}: {k} = {got[k]!r}, the reference has {want[k]!r}"
    bound = DR.sum_bound(want["count"], want["abs_sum"])
    err = abs(got["sum"] - want["sum"])
    print(f"  {what}: |sum - fsum| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{what}: sum {got['sum']!r} vs fsum {want['sum']!r}: off by {err:.3e} > {bound:.3e}"


def _check_diff_row(row, want, what):
    count, n_diff, first, mad = row
    got = dict(count=int(count), n_diff=int(n_diff), first_diff=int(first), max_abs_diff=_f64(mad))
    assert got == want, f"{what}: {got}, the reference has {want}"


def _predict_guard(pkg, oracle, patches, every, sweeps):
    """(sweeps_checked, sweep, field, member, offset, n_nonfinite) from oracle sweeps: the first finding is the earliest checked
    sweep, then the lowest member, then ww before t before mu, then the smallest offset; counted over the compute window."""
    b, cfg = patches[0].bounds, patches[0].config
    i0, i1, j0, j1, k0, k1 = pkg.compute_window(cfg, b.ids, b.ide, b.jds, b.jde, b.its, b.ite, b.jts, b.jte, b.kts, b.kte)
    ext = (b.ims, b.ime, b.jms, b.jme, b.kms, b.kme)
    finding = None
    for s in range(1, sweeps + 1):
        for p in patches:
            oracle.advance_mu_t(*p.args())
        if s % every or finding:
            continue
        for m, p in enumerate(patches):
            for name, fid in (("ww", 0), ("t", T), ("mu", MU)):
                st = DR.stats(p.arrays[name], ext, (i0, i1, k0, k1, j0, j1))
                if st["n_nan"] + st["n_inf"] and finding is None:
                    finding = (s, fid, m, st["first_nonfinite"], st["n_nan"] + st["n_inf"])
    return (sweeps // every, *(finding or (0, 0, 0, 0, 0)))


@pytest.mark.parametrize("case", [F64, F32], ids=IDS[:2])
def test_statistics_compare_and_guard_interfaces(pkg, oracle, host, tmp_path, case):
    """amt_domain_field_stats / amt_ensemble_field_stats on t and mu over both regions, amt_stats_device_* and
    amt_compare_device_* with a box strictly inside the extents and members = 2, amt_domain_compare of two handles that differ in
    three planted cells per field, on a state with NaN, +Inf, -Inf and -0.0 planted: every member of the records equals diag_ref
    (sum: within diag_ref.sum_bound of math.fsum).  The guard on a domain (every 2, four sweeps, one NaN in ft) and on an ensemble
    (every 1, two sweeps, the NaN in member 1 only): amt_*_sync returns AMT_ERR_NONFINITE and the report is the oracle's."""
    itemsize, dims, aligned = case
    S = pkg.synth
    cfg = pkg.GridConfig()
    b = S.domain_bounds(*dims, aligned=aligned)
    recs = _run_host(host, "diag", tmp_path, itemsize, b, cfg, dims)
    ps = _members(pkg, b, cfg, itemsize, dims)
    for p in ps:
        _plant_specials(p)
    ext = (b.ims, b.ime, b.jms, b.jme, b.kms, b.kme)
    i0, i1, j0, j1, k0, k1 = pkg.compute_window(cfg, b.ids, b.ide, b.jds, b.jde, b.its, b.ite, b.jts, b.jte, b.kts, b.kte)
    boxes = {0: (i0, i1, k0, k1, j0, j1), 1: (b.ims, b.ime, b.kms, b.kme, b.jms, b.jme),
             9: (b.ims + 1, b.ime - 1, b.kms + 1, b.kme - 1, b.jms + 1, b.jme - 1)}
    seen = 0
    for row in recs:
        if row[0] in ("dstats", "estats", "pstats"):
            name, region, m = row[1], int(row[2]), int(row[3])
            want = DR.stats(ps[m].arrays[name], ext, boxes[region])
            assert want["n_nan"] == 1 and want["n_inf"] == 2, (name, region)          # the box holds the planted cells
            _check_stats_row(row[4:], want, f"{row[0]} {name} region {region} member {m}")
            seen += 1
    assert seen == 2 * 2 * (1 + MEMBERS) + 2 * 2
    qs = [p.copy() for p in ps]
    for q in qs:
        _plant_differences(q)
    seen = 0
    for row in recs:
        if row[0] in ("dcompare", "pcompare"):
            name, region, m = row[1], int(row[2]), int(row[3])
            want = DR.diff(ps[m].arrays[name], qs[m].arrays[name], ext, boxes[region])
            assert want["n_diff"] == 3 and want["max_abs_diff"] > 0, (name, region, want)
            _check_diff_row(row[4:], want, f"{row[0]} {name} region {region} member {m}")
            seen += 1
    assert seen == 2 * 2 + 2 * 2
    # the guard
    assert tuple(map(int, _value(recs, "dguard_off"))) == (0, 0, 0, 0, 0, 0, 0)
    one = _members(pkg, b, cfg, itemsize, dims)[:1]
    one[0].arrays["ft"][_cell(b, b.its + 3, b.kts + 2, b.jts + 2)] = np.nan
    want = _predict_guard(pkg, oracle, one, 2, 4)
    assert want == (2, 2, T, 0, int(np.ravel_multi_index(_cell(b, b.its + 3, b.kts + 2, b.jts + 2), b.shape("t"))), 1)
    assert tuple(map(int, _value(recs, "dguard"))) == (7, *want)
    msg = " ".join(_value(recs, "dguard_message"))
    assert "sweep 2" in msg and "field t" in msg and f"({b.its + 3},{b.kts + 2},{b.jts + 2})" in msg, msg
    ens = _members(pkg, b, cfg, itemsize, dims)
    ens[1].arrays["ft"][_cell(b, b.its + 3, b.kts + 2, b.jts + 2)] = np.nan
    want = _predict_guard(pkg, oracle, ens, 1, 2)
    assert want[:4] == (2, 1, T, 1) and want[5] == 1
    assert tuple(map(int, _value(recs, "eguard"))) == (7, *want)


# ---------------------------------------------------------------------------------------------------------------------
# host-owned halos
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,pi,pj", [(F64, 2, 1), (F32, 1, 2)], ids=["f64-grid-2x1", "f32-slab-1x2"])
def test_host_owned_halo_interfaces(pkg, oracle, host, tmp_path, case, pi, pj):
    """Both ranks in one Fortran process; the loop of INTEGRATION.md section 8 with the two MPI calls replaced by c_f_pointer and
    an array copy: two sweeps with new exchanged inputs and poisoned halos, every owned cell of every output against the
    unsplit oracle run; then _halo_pack / _halo_unpack once: the halos hold the neighbour's new values, corners stay poisoned."""
    import os
    from multirank import oracle_sweeps
    from wrf_model_cuda_sample_amd import lib
    itemsize, dims, _aligned = case
    S, P, L = pkg.synth, pkg.patch, pkg.load_library()
    cfg = pkg.GridConfig()
    gb = S.domain_bounds(*dims)
    env = dict(os.environ, AMT_SLAB_TRANSPORT="ipc")           # amt_comm_unique_id then needs no RCCL; external handles ignore it
    recs = _run_host(host, "halo", tmp_path, itemsize, gb, cfg, dims, extra=(pi, pj), env=env)
    assert [r[1:] for r in recs if r[0] == "transport"] == [["external"]] * 2
    assert _value(recs, "transport_1x1") == ["none"] and _value(recs, "transport_slab_1") == ["none"]
    assert _value(recs, "grid_exchange_1x1") == ["0"] and _value(recs, "slab_exchange_1") == ["0"]
    assert len(_value(recs, "launch_nonce")) == 1
    full = _patch(pkg, gb, cfg, itemsize, dims, SEED)
    oracle_sweeps(pkg, oracle, full, SEED, 2)
    for r in range(2):
        ri, rj = r % pi, r // pi
        b = S.patch_bounds(gb, ri, rj, pi, pj)
        out, n = (lib.HaloMessage * 4)(), ctypes.c_int(-1)
        assert L.amt_halo_plan(itemsize, *cfg.as_ints(), *b.as_tuple(), ri, rj, pi, pj, 64, out, 4, ctypes.byref(n)) == 0
        want = [(r, m.side, m.peer, m.send_bytes, m.recv_bytes, 1, 1) for m in out[:n.value]]
        assert [tuple(map(int, x[1:])) for x in recs if x[0] == "message" and int(x[1]) == r] == want and len(want) == 1
        sides = sum(m[1] for m in want)
        got = _load(pkg, tmp_path, f"r{r}step", b, itemsize)
        J, I = slice(b.jts - b.jms, b.jte - b.jms + 1), slice(b.its - b.ims, b.ite - b.ims + 1)
        GJ, GI = slice(b.jts - gb.jms, b.jte - gb.jms + 1), slice(b.its - gb.ims, b.ite - gb.ims + 1)
        for name in S.OUTPUTS:
            assert bits_equal(got[name][J, ..., I], full.arrays[name][GJ, ..., GI]), f"rank {r}: {name} differs from the unsplit run"
            assert np.isfinite(got[name][J, ..., I][..., :b.kte - b.kms, :] if name in S.RANK3 else got[name][J, I]).all(), (r, name)
        # pack / unpack alone: the inputs of seed + 2, poisoned halos, then what the neighbour sent
        packed = _load(pkg, tmp_path, f"r{r}pack", b, itemsize)
        for name in S.OUTPUTS:
            assert bits_equal(packed[name], got[name]), f"rank {r}: {name} changed without a sweep"
        fresh = _patch(pkg, b, cfg, itemsize, dims, SEED)
        S.refresh_exchanged_inputs(fresh, SEED, 2)
        want_in = fresh.copy()
        S.poison_halos(want_in, sides)
        f, w = fresh.arrays, want_in.arrays
        if sides & S.SIDE_ABOVE:
            for name in S.HALO_FROM_ABOVE:
                w[name][b.jte + 1 - b.jms, ..., I] = f[name][b.jte + 1 - b.jms, ..., I]
        if sides & S.SIDE_BELOW:
            w["t_1"][b.jts - 1 - b.jms, :, I] = f["t_1"][b.jts - 1 - b.jms, :, I]
        if sides & S.SIDE_RIGHT:
            for name in S.HALO_FROM_RIGHT:
                w[name][J, ..., b.ite + 1 - b.ims] = f[name][J, ..., b.ite + 1 - b.ims]
        if sides & S.SIDE_LEFT:
            w["t_1"][J, :, b.its - 1 - b.ims] = f["t_1"][J, :, b.its - 1 - b.ims]
        for name in S.EXCHANGED_INPUTS:
            assert np.isnan(w[name]).any() == (name in ("t_1",) + (S.HALO_FROM_ABOVE if sides & S.SIDE_ABOVE else ())
                                               + (S.HALO_FROM_RIGHT if sides & S.SIDE_RIGHT else ())), name
            assert packed[name].dtype == w[name].dtype and np.array_equal(packed[name], w[name], equal_nan=True), \
                f"rank {r}: {name} after pack, carry, unpack"
        if r == 0:                                             # one plain sweep of rank 0's patch as it stands (amt_grid_step, 1 x 1)
            alone = S.Patch(b, cfg, {k: v.copy() for k, v in packed.items()}, *_scalars(itemsize), tuple(dims))
            oracle.advance_mu_t(*alone.args())
            grid = _load(pkg, tmp_path, "r0grid", b, itemsize)
            for name in S.OUTPUTS:
                assert bits_equal(grid[name], alone.arrays[name]), f"amt_grid_step on a grid of one patch: {name} differs"


# ---------------------------------------------------------------------------------------------------------------------
# the one-shot call's control calls
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,flag", [(F64, "specified_periodic_x"), (F32, "none")], ids=IDS[:2])
def test_one_shot_control_interfaces(pkg, oracle, host, tmp_path, case, flag):
    """Two one-shot calls on host arrays with one device slot named (amt_host_set_devices / amt_host_devices), the residency
    cache in its checking mode and invalidated between the calls, then amt_host_release: the oracle's bits in all 26 arrays."""
    import cases
    itemsize, dims, aligned = case
    cfg = pkg.GridConfig(**cases.FLAG_COMBOS[flag])
    b = pkg.synth.domain_bounds(*dims, aligned=aligned)
    recs = _run_host(host, "oneshot", tmp_path, itemsize, b, cfg, dims)
    assert _value(recs, "host_devices") == ["1", "0"]
    want = _patch(pkg, b, cfg, itemsize, dims, SEED)
    for _ in range(2):
        oracle.advance_mu_t(*want.args())
    _assert_all_fields(pkg, _load(pkg, tmp_path, "host2", b, itemsize), want.arrays, f"one-shot ({flag})")
