"""Parity on PACKED state (tests/packed_state.py): all arrays of a call are views of ONE pool, each at an element offset of its
own, bracketed by guard bands of NaNs that carry their pool index.  Over the rotations of a layout every array takes every
phase ``base % 16``; the pairs whose two addresses decide one access width (t/ft, mu/mu_tend, muts/mu_tend, t_1/t, the two
operands of a compare, a halo copy's source and destination) never share one.  The pool goes to the device as ONE tensor, comes
back as ONE tensor and is compared WHOLE, as bytes, with the initial pool into which the oracle (or the numpy reference of the
call) has written its results: outputs, inputs that must stay, unread levels and every guard byte are one assertion, and a
result that depended on an out-of-array read is NaN.  tests/test_packed_state_cpu.py shows that this comparison fails on
planted defects.

a: march wave shapes forced, one per memory path;  b: the launcher's choice and the column kernel;  c: ensembles in one launch;
d: the stand-alone device calls (boundary-zone update, cyclic refresh, compare, statistics, moments);  e: resident handles wrapped
over the pool with cyclic refresh, boundary-zone update and non-finite guard armed TOGETHER;  f: the one-shot host call on a
host pool.  Page-locking packed host arrays (amt_host_pin) is out of scope: neighbouring arrays share pages.

No wall-clock assertion anywhere."""
import ctypes

import numpy as np
import pytest

import cases
import cyclic_ref as CR
import diag_ref as D
import moments_ref as R
import packed_state as PS
import specbdy_ref as SB

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
DTYPES = [F64, F32]
FLAGS = list(cases.FLAG_COMBOS.values())          # none, specified, specified + periodic_x, nested
X, Y = CR.CYCLIC_X, CR.CYCLIC_Y
BELOW, ABOVE, LEFT, RIGHT = 1, 2, 4, 8

# Cases of this file that failed before a fix in the library: (bounds in the order of synth.INT_NAMES, flags, dtype, rotation,
# kernel label).  None so far: every case passed on the library as it was.
REGRESSIONS = []


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


def _per(dtype):
    return 16 // np.dtype(dtype).itemsize


def _rotations(dtype, ends_only=False):
    per = _per(dtype)
    return (0, per - 1) if ends_only else tuple(range(per))


def _inputs(S, b, cfg, dtype, members, seed, gdims=None):
    """(one host patch per member, name -> array as the pool holds it: member-stacked where members > 1)."""
    ps = [S.make_patch(b, cfg, dtype=dtype, seed=seed + 10 * m, global_dims=gdims) for m in range(members)]
    if members == 1:
        return ps, ps[0].arrays
    return ps, {n: (ps[0].arrays[n] if S.field_rank(n) == 1 else np.stack([p.arrays[n] for p in ps])) for n in S.FIELD_NAMES}


def _member(S, p0, arrays, m, members):
    """Member m's patch over (views of) member-stacked arrays."""
    one = arrays if members == 1 else {n: (a if S.field_rank(n) == 1 else a[m]) for n, a in arrays.items()}
    return S.Patch(p0.bounds, p0.config, one, p0.rdx, p0.rdy, p0.dts, p0.epssm, p0.global_dims)


def _upload(torch, pool):
    dpool = torch.from_numpy(pool).to("cuda:0")
    assert dpool.data_ptr() % 128 == 0                                  # the phases are those of the layout
    return dpool


def _assert_pool(dpool, want, lay, what):
    got = dpool.cpu().numpy() if hasattr(dpool, "cpu") else dpool
    d = PS.diff(got, want, lay)
    assert d is None, f"{what}: the pool differs from the expected one: {d}"


def _label(pkg):
    return pkg.load_library().amt_march_last_kernel().decode()


def _sweep_case(pkg, oracle, b, cfg, dtype, rotation, seed, members=1, gdims=None):
    """(first member's host patch, layout, initial pool, expected pool after ONE sweep of every member)."""
    S = pkg.synth
    ps, arrays = _inputs(S, b, cfg, dtype, members, seed, gdims)
    lay = PS.layout(b, dtype, members, rotation)
    pool = PS.place(arrays, lay)
    want = PS.clone(pool)
    wv = PS.views(want, lay, b, members)
    for m in range(members):
        oracle.advance_mu_t(*_member(S, ps[0], wv, m, members).args())
    return ps[0], lay, pool, want


# ---------------------------------------------------------------------------------------------
# a: forced march shapes, one per memory path
# ---------------------------------------------------------------------------------------------
# (dtype, vw, kpt, hl, xd, dma, max waves) -- of AMT_MARCH_SHAPES (tests/test_gpu_11_shapes.py runs all of them on separate arrays)
MARCH = [(F64, 1, 4, 1, 0, 1, 16), (F64, 1, 2, 1, 3, 1, 16), (F64, 1, 4, 1, 0, 0, 16), (F64, 1, 4, 4, 0, 1, 16),
         (F32, 1, 4, 1, 0, 1, 16), (F32, 2, 4, 1, 1, 1, 16), (F32, 2, 4, 1, 0, 0, 16), (F32, 2, 6, 4, 0, 1, 12)]


def _march_id(s):
    return f"{np.dtype(s[0]).name}-vw{s[1]}-kpt{s[2]}-hl{s[3]}-xd{s[4]}-{'dma' if s[5] else 'reg'}-w{s[6]}"


@pytest.mark.parametrize("shape", MARCH, ids=_march_id)
def test_forced_march_shape_on_packed_state(pkg, oracle, torch_mod, force, shape):
    """Three tiles with the last partly filled, seven rows; a level count that fills the cell waves and a ragged one; padded rows
    and an odd row length; the launcher's rows per workgroup and three; every rotation; the four flag sets in turn.  A shape
    the launcher refuses (status 3) fails the test: the level counts are feasible."""
    torch = torch_mod
    dtype, vw, kpt, hl, xd, dma, wm = shape
    S = pkg.synth
    lw, tc = kpt * hl, (64 // hl) * vw
    ni = 2 * tc + tc // 2 + 3
    case = 0
    for nk in (3 * lw, 2 * lw + 1):
        for aligned in (True, False):
            cfg = pkg.GridConfig(**FLAGS[case % 4])
            case += 1
            b = S.domain_bounds(ni, nk, 7, aligned=aligned)
            if not aligned and vw == 2 and not dma:
                # register flavour with two columns per lane: whole pairs from the first tile's column 0 to the row end, the
                # rule tests/test_gpu_11_shapes.py applies to its bounds
                def col_lo(bb):
                    line = 128 // np.dtype(dtype).itemsize
                    i0 = pkg.compute_window(cfg, bb.ids, bb.ide, bb.jds, bb.jde, bb.its, bb.ite, bb.jts, bb.jte, bb.kts, bb.kte)[0] - bb.ims
                    return i0 if bb.idim % line else i0 // line * line
                for _ in range(3):
                    if (b.idim - col_lo(b)) % 2 == 0:
                        break
                    b = b.replace(ime=b.ime + 1)
            for rotation in _rotations(dtype):
                p0, lay, pool, want = _sweep_case(pkg, oracle, b, cfg, dtype, rotation, 100 + nk, gdims=(ni, nk, 7))
                for jrows in (0, 3):
                    force(vw, kpt, hl, xd, dma, jrows, wm)
                    dpool = _upload(torch, pool)
                    pkg.advance_mu_t(*_member(S, p0, PS.views(dpool, lay, b), 0, 1).args(), variant=pkg.VARIANT_MARCH)
                    torch.cuda.synchronize()
                    name = _label(pkg)
                    what = f"{_march_id(shape)} nk={nk} aligned={aligned} flags={cfg} rotation={rotation} jrows={jrows} ({name})"
                    assert f", {vw}, {kpt}, {hl}, {xd}, FULL, {'true' if dma else 'false'}, {wm}, " in name, what
                    assert (", nt>" if (b.idim * np.dtype(dtype).itemsize) % 128 == 0 else ", cached>") in name, what
                    _assert_pool(dpool, want, lay, what)
    assert case == 4


# ---------------------------------------------------------------------------------------------
# b: the launcher's own choice, and the column kernel
# ---------------------------------------------------------------------------------------------
# (dims, aligned, tile override)
LAUNCHER = [((130, 13, 9), False, None), ((100, 20, 18), True, None), ((37, 40, 5), False, None), ((37, 20, 5), False, None),
            ((20, 241, 3), False, None), ((130, 3, 7), False, dict(its=60, ite=70, jts=3, jte=5))]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("dims,aligned,tile", LAUNCHER, ids=["130x13x9", "100x20x18-padded", "37x40x5", "37x20x5", "20x241x3-tall", "130x3x7-tile"])
def test_auto_and_column_on_packed_state(pkg, oracle, torch_mod, dims, aligned, tile, dtype):
    """VARIANT_AUTO and VARIANT_COLUMN: 40 levels are above the fp64 column kernel's 32-level rule (it recomputes), 20 take its
    LDS column, 241 fp64 levels are beyond the march kernel (AUTO falls back to the column kernel); one interior tile call."""
    torch = torch_mod
    S = pkg.synth
    b = S.domain_bounds(*dims, aligned=aligned)
    if tile:
        b = b.replace(**tile)
    n = LAUNCHER.index((dims, aligned, tile))
    for rotation in _rotations(dtype):
        cfg = pkg.GridConfig(**FLAGS[(n + rotation) % 4])
        p0, lay, pool, want = _sweep_case(pkg, oracle, b, cfg, dtype, rotation, 500 + n, gdims=dims)
        for variant in (pkg.VARIANT_AUTO, pkg.VARIANT_COLUMN):
            dpool = _upload(torch, pool)
            pkg.advance_mu_t(*_member(S, p0, PS.views(dpool, lay, b), 0, 1).args(), variant=variant)
            torch.cuda.synchronize()
            label = _label(pkg)
            what = f"{dims} {np.dtype(dtype).name} flags={cfg} rotation={rotation} variant={variant} ({label})"
            column = variant == pkg.VARIANT_COLUMN or dims[1] > (240 if dtype == F64 else 264)
            assert ("amt_column_kernel" in label) == column and ("amt_march_kernel<" in label) != column, what
            _assert_pool(dpool, want, lay, what)


# ---------------------------------------------------------------------------------------------
# c: ensembles in one launch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("members,dims,aligned", [(3, (67, 9, 5), False), (2, (128, 12, 6), True)], ids=["3x67x9x5", "2x128x12x6-padded"])
def test_ensemble_call_on_packed_state(pkg, oracle, torch_mod, members, dims, aligned, dtype):
    """advance_mu_t_ensemble on member-stacked views.  69 x 10 x 7 elements per member: the member stride is no multiple of 16
    bytes in either dtype.  Every member bit-equal to the oracle on that member; the halo rows between the members and the
    guards keep their bytes (the whole pool is compared)."""
    torch = torch_mod
    S = pkg.synth
    b = S.domain_bounds(*dims, aligned=aligned)
    if not aligned:
        assert (b.idim * b.kdim * b.jdim * 4) % 16 and (b.idim * b.jdim * 8) % 16
    for rotation in _rotations(dtype):
        cfg = pkg.GridConfig(**FLAGS[(members + rotation) % 4])
        p0, lay, pool, want = _sweep_case(pkg, oracle, b, cfg, dtype, rotation, 4000, members=members, gdims=dims)
        for variant in (pkg.VARIANT_MARCH, pkg.VARIANT_COLUMN):
            dpool = _upload(torch, pool)
            a = PS.views(dpool, lay, b, members)
            assert tuple(a["t"].shape) == (members, b.jdim, b.kdim, b.idim)
            pkg.advance_mu_t_ensemble(*S.Patch(b, cfg, a, p0.rdx, p0.rdy, p0.dts, p0.epssm).args(), variant=variant)
            torch.cuda.synchronize()
            label = _label(pkg)
            what = f"{members} x {dims} {np.dtype(dtype).name} flags={cfg} rotation={rotation} variant={variant} ({label})"
            assert ("amt_march_kernel<" if variant == pkg.VARIANT_MARCH else "amt_column_kernel<") in label, what
            assert f"members={members}" in label or variant == pkg.VARIANT_COLUMN, what
            _assert_pool(dpool, want, lay, what)


# ---------------------------------------------------------------------------------------------
# d: stand-alone device calls whose access width depends on two addresses
# ---------------------------------------------------------------------------------------------
NAMES5 = ("t", "ft", "mu", "muts", "mu_tend")
NAMES9 = ("u", "u_1", "v", "v_1", "t_1", "muu", "muv", "msfuy", "msfvx_inv")
MOVER_SHAPES = [37, 40]


def _mover_bounds(S, idim):
    """The two memory shapes of tests/test_gpu_19b_mover_alignment.py: 37 x 5 x 11, and 40 x 5 x 11 with ims = -3."""
    b = S.domain_bounds(35, 4, 9) if idim == 37 else S.domain_bounds(32, 4, 9).replace(ims=-3, ime=36)
    assert (b.idim, b.kdim, b.jdim) == (idim, 5, 11)
    return b


def _subset_case(pkg, b, dtype, members, rotation, names, seed):
    """(layout, pool) of the arrays `names` alone, member-stacked where members > 1."""
    _ps, arrays = _inputs(pkg.synth, b, pkg.GridConfig(), dtype, members, seed)
    lay = PS.layout(b, dtype, members, rotation, names=names)
    return lay, PS.place({n: arrays[n] for n in names}, lay)


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("idim", MOVER_SHAPES, ids=["37x5x11", "40x5x11-ims-3"])
def test_spec_bdy_update_on_packed_state(pkg, torch_mod, idim, dtype, members):
    """t and ft, mu / muts and mu_tend on different phases in every rotation: the kernel's mixed branch (one operand on a
    16-byte boundary, the other not).  Flags (0,1,0): four strips; (1,1,0): two."""
    torch = torch_mod
    S = pkg.synth
    b = _mover_bounds(S, idim)
    dts = S.DTS
    for rotation in _rotations(dtype):
        lay, pool = _subset_case(pkg, b, dtype, members, rotation, NAMES5, 41)
        assert lay.phase_bytes("t") != lay.phase_bytes("ft") and lay.phase_bytes("mu") != lay.phase_bytes("mu_tend") != lay.phase_bytes("muts")
        for flags in ((0, 1, 0), (1, 1, 0)):
            zone = SB.zone_mask(flags, b)
            if flags == (0, 1, 0):
                i0, i1, j0, j1 = SB.window(flags, b)
                assert zone[j0 - 1 - b.jms].any() and zone[j1 + 1 - b.jms].any() and zone[j0 - b.jms, i0 - 1 - b.ims] and zone[j0 - b.jms, i1 + 1 - b.ims]
            want = PS.clone(pool)
            SB.spec_bdy_update(PS.views(want, lay, None, members), b, flags, dts)
            assert set(PS.diff(want, pool, lay)["counts"]) == {"t", "mu", "muts"}
            dpool = _upload(torch, pool)
            dv = PS.views(dpool, lay, None, members)
            cfg = pkg.GridConfig(periodic_x=bool(flags[0]), specified=bool(flags[1]), nested=bool(flags[2]))
            pkg.spec_bdy_update(*[dv[n] for n in NAMES5], dts, cfg, *b.as_tuple(), members=members)
            torch.cuda.synchronize()
            _assert_pool(dpool, want, lay, f"spec_bdy_update {idim} {np.dtype(dtype).name} members={members} flags={flags} rotation={rotation}")


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("idim", MOVER_SHAPES, ids=["37x5x11", "40x5x11-ims-3"])
def test_cyclic_fill_on_packed_state(pkg, torch_mod, idim, dtype, members):
    torch = torch_mod
    S = pkg.synth
    b = _mover_bounds(S, idim)
    cfg = pkg.GridConfig()
    for rotation in _rotations(dtype):
        lay, pool = _subset_case(pkg, b, dtype, members, rotation, NAMES9, 43)
        for axes in (X, Y, X | Y):
            want = PS.clone(pool)
            CR.cyclic_fill(PS.views(want, lay, None, members), b, axes)
            assert PS.diff(want, pool, lay) is not None
            dpool = _upload(torch, pool)
            dv = PS.views(dpool, lay, None, members)
            pkg.cyclic_fill(*[dv[n] for n in NAMES9], cfg, *b.as_tuple(), axes=axes, members=members)
            torch.cuda.synchronize()
            _assert_pool(dpool, want, lay, f"cyclic_fill {idim} {np.dtype(dtype).name} members={members} axes={axes} rotation={rotation}")


def _record(rec):
    return bytes(rec)


def _diag_operands(S, b, dtype, members, seed):
    """A member-stacked 3-D field and a copy of it."""
    ps = [S.make_patch(b, dtype=dtype, seed=seed + m) for m in range(members)]
    return np.stack([p.arrays["t"] for p in ps])


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("idim", MOVER_SHAPES, ids=["37x5x11", "40x5x11-ims-3"])
def test_compare_and_field_stats_on_packed_state(pkg, torch_mod, idim, dtype, members):
    """diag.compare with its two operands on different phases and diag.field_stats: the records of the same operands in
    separate, aligned tensors, byte for byte (and the reference's counts); nothing in the pool changes.  One bit differs in the
    last element of a run and one in the first element of a run's last chunk (a short chunk where the run is no whole number
    of 16-byte chunks), in every member."""
    torch = torch_mod
    S = pkg.synth
    b = _mover_bounds(S, idim)
    per = _per(dtype)
    u = PS._uint(dtype)
    a = _diag_operands(S, b, dtype, members, 70)
    ext = (0, b.idim - 1, 0, b.jdim - 1, 0, b.kdim - 1)
    boxes = {"memory": (0, b.idim - 1, 0, b.kdim - 1, 0, b.jdim - 1), "odd": (1, b.idim - 2, 1, b.kdim - 1, 1, b.jdim - 2)}
    for bname, box in boxes.items():
        ni = box[1] - box[0] + 1
        other = a.copy()
        other.view(u)[:, box[4] + 1, box[2], box[1]] ^= u(1)                                     # the last element of a run
        other.view(u)[:, box[5], box[3], box[0] + (ni - 1) // per * per] ^= u(4)                  # the first element of a run's last chunk
        sep_a, sep_b = torch.from_numpy(a).to("cuda:0"), torch.from_numpy(other).to("cuda:0")
        assert sep_a.data_ptr() % 16 == 0 and sep_b.data_ptr() % 16 == 0
        want_diff = pkg.diag.compare(sep_a, sep_b, stacked=True, extents=ext, box=box)
        want_stats = pkg.diag.field_stats(sep_b, stacked=True, extents=ext, box=box)
        for m in range(members):
            ref = D.diff(a[m], other[m], ext, box)
            assert (want_diff[m].count, want_diff[m].n_diff, want_diff[m].first_diff) == (ref["count"], 2, ref["first_diff"])
        for rotation in _rotations(dtype):
            lay = PS.layout(b, dtype, members, rotation, names={"a": a.shape, "b": a.shape})
            assert lay.phase_bytes("a") != lay.phase_bytes("b")
            pool = PS.place({"a": a, "b": other}, lay)
            dpool = _upload(torch, pool)
            dv = PS.views(dpool, lay)
            got_diff = pkg.diag.compare(dv["a"], dv["b"], stacked=True, extents=ext, box=box)
            got_stats = pkg.diag.field_stats(dv["b"], stacked=True, extents=ext, box=box)
            what = f"{idim} {np.dtype(dtype).name} members={members} box={bname} rotation={rotation}"
            for m in range(members):
                assert _record(got_diff[m]) == _record(want_diff[m]), f"compare, {what}, member {m}: {got_diff[m]} != {want_diff[m]}"
                assert _record(got_stats[m]) == _record(want_stats[m]), f"field_stats, {what}, member {m}: {got_stats[m]} != {want_stats[m]}"
            _assert_pool(dpool, pool, lay, what)


def _sentinel(dtype):
    """A quiet NaN with a payload no arithmetic produces."""
    if np.dtype(dtype).itemsize == 8:
        return np.array([0x7FF8_0000_00C0_FFEE], dtype=np.uint64).view(np.float64)[0]
    return np.array([0x7FC0_BEEF], dtype=np.uint32).view(np.float32)[0]


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("idim", MOVER_SHAPES, ids=["37x5x11", "40x5x11-ims-3"])
def test_moments_on_packed_state(pkg, torch_mod, idim, dtype, members):
    """diag.moments with the input and the four outputs in one pool, neighbours on different phases, against moments_ref.  The
    outputs hold a sentinel NaN before the call and must show exactly those bits outside the box."""
    torch = torch_mod
    S = pkg.synth
    b = _mover_bounds(S, idim)
    a = _diag_operands(S, b, dtype, members, 90)
    ext = (0, b.idim - 1, 0, b.jdim - 1, 0, b.kdim - 1)
    one = a.shape[1:]
    before = np.full(one, _sentinel(dtype), dtype=dtype)
    for bname, box in {"memory": (0, b.idim - 1, 0, b.kdim - 1, 0, b.jdim - 1), "odd": (1, b.idim - 2, 1, b.kdim - 1, 1, b.jdim - 2)}.items():
        ref = R.moments(a, ext, box)
        idx = R.member_index(a, ext, box)
        assert all(np.isfinite(ref[n]).all() for n in R.NAMES)
        for rotation in _rotations(dtype):
            lay = PS.layout(b, dtype, members, rotation, names=dict(a=a.shape, mean=one, var=one, lo=one, hi=one))
            assert len({lay.phase_bytes(n) for n in lay.names}) == min(_per(dtype), 5)
            pool = PS.place(dict(a=a, mean=before, var=before, lo=before, hi=before), lay)
            want = PS.place(dict(a=a, **{n: R.expected(before, ref[n], idx) for n in R.NAMES}), lay)
            dpool = _upload(torch, pool)
            dv = PS.views(dpool, lay)
            got = pkg.diag.moments(dv["a"], extents=ext, box=box, want=R.NAMES, out={n: dv[n] for n in R.NAMES})
            torch.cuda.synchronize()
            assert all(got[n] is dv[n] for n in R.NAMES)
            _assert_pool(dpool, want, lay, f"moments {idim} {np.dtype(dtype).name} members={members} box={bname} rotation={rotation}")


# ---------------------------------------------------------------------------------------------
# e: handles over the pool; cyclic refresh + sweep + boundary-zone update + guard on one handle
# ---------------------------------------------------------------------------------------------
def _poison(arrays, b, sides):
    """NaN into the cells the stencil reads across `sides` of the DOMAIN: whole columns ide / ids-1 and rows jde / jds-1, corners
    included; numpy arrays or torch tensors, member-stacked or not."""
    c, r = (lambda i: i - b.ims), (lambda j: j - b.jms)
    if sides & RIGHT:
        for n in CR.COLS_FROM_RIGHT:
            arrays[n][..., c(b.ide)] = np.nan
    if sides & LEFT:
        arrays["t_1"][..., c(b.ids - 1)] = np.nan
    if sides & ABOVE:
        for n in CR.ROWS_FROM_ABOVE:
            if n in CR.RANK3:
                arrays[n][..., r(b.jde), :, :] = np.nan
            else:
                arrays[n][..., r(b.jde), :] = np.nan
    if sides & BELOW:
        arrays["t_1"][..., r(b.jds - 1), :, :] = np.nan


def _exchanged_mask(S):
    m = 0
    for n in S.EXCHANGED_INPUTS:
        m |= 1 << S.FIELD_ID[n]
    return m


def _step_packed(pkg, oracle, torch, kind, dims, aligned, dtype, rotation, flags, axes, spec, sweeps=3, seed=900):
    """Three sweeps of a handle wrapped over pool views on a side stream, the exchanged inputs refilled (seed + sweep) and the
    halos of the cyclic sides re-poisoned in front of each.  Returns (pool from the device, expected pool, layout, bounds, the
    guard's report, what).  Expected per sweep, on the host pool: the refill, the poison, cyclic_ref, the oracle, specbdy_ref."""
    from wrf_model_cuda_sample_amd import lib
    S, L = pkg.synth, pkg.load_library()
    members = 3 if kind == "ensemble" else 1
    cfg = pkg.GridConfig(periodic_x=bool(flags[0]), specified=bool(flags[1]), nested=bool(flags[2]))
    b = S.domain_bounds(*dims, aligned=aligned)
    ps, arrays = _inputs(S, b, cfg, dtype, members, seed, dims)
    lay = PS.layout(b, dtype, members, rotation)
    pool = PS.place(arrays, lay)
    sides = (LEFT | RIGHT if axes & X else 0) | (BELOW | ABOVE if axes & Y else 0)
    p0 = ps[0]
    seeds = [seed + 10 * m for m in range(members)]

    # the expected pool
    want = PS.clone(pool)
    wv = PS.views(want, lay, b, members)
    for s in range(sweeps):
        for m in range(members):
            S.refresh_exchanged_inputs(_member(S, p0, wv, m, members), seeds[m], s)
        _poison(wv, b, sides)
        CR.cyclic_fill(wv, b, axes, flags)
        for m in range(members):
            oracle.advance_mu_t(*_member(S, p0, wv, m, members).args())
        if spec:
            SB.spec_bdy_update(wv, b, flags, p0.dts)

    # the device
    dpool = _upload(torch, pool)
    dv = PS.views(dpool, lay, b, members)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    if kind == "ensemble":
        ens = pkg.Ensemble.wrap(dv, b, cfg, stream=stream)
        try:
            assert ens.stream == stream.cuda_stream and ens.field_ptr("t") == dv["t"].data_ptr()
            ens.set_scalars(p0.rdx, p0.rdy, p0.dts, p0.epssm)
            ens.set_cyclic(axes)
            if spec:
                ens.set_spec_bdy(True)
            ens.set_guard(1)
            for s in range(sweeps):
                for m in range(members):           # (there is no amt_ensemble_fill_fields: the generator writes through the views)
                    S.refresh_exchanged_inputs(_member(S, p0, dv, m, members), seeds[m], s, stream=stream)
                ens.sync()
                _poison(dv, b, sides)
                torch.cuda.synchronize()
                ens.step(1)
                ens.sync()
            report = ens.guard_report()
        finally:
            ens.close()
    else:
        h = ctypes.c_void_p()
        fields = (ctypes.c_void_p * len(S.FIELD_NAMES))(*[dv[n].data_ptr() for n in S.FIELD_NAMES])
        lib.check(L.amt_domain_wrap(ctypes.byref(h), np.dtype(dtype).itemsize, *cfg.as_ints(), *b.as_tuple(), fields, ctypes.c_void_p(stream.cuda_stream)))
        try:
            assert int(L.amt_domain_stream(h) or 0) == stream.cuda_stream
            lib.check(L.amt_domain_set_scalars(h, p0.rdx, p0.rdy, p0.dts, p0.epssm))
            lib.check(L.amt_domain_set_cyclic(h, axes))
            if spec:
                lib.check(L.amt_domain_set_spec_bdy(h, 1))
            lib.check(L.amt_domain_set_guard(h, 1))
            for s in range(sweeps):
                lib.check(L.amt_domain_fill_fields(h, ctypes.c_uint64(_exchanged_mask(S)), ctypes.c_uint64(seed + s),
                                                   b.ims, b.kms - 1, b.jms, dims[0] + 2, dims[1] + 1, dims[2] + 2))
                lib.check(L.amt_domain_sync(h))
                _poison(dv, b, sides)
                torch.cuda.synchronize()
                lib.check(L.amt_domain_step(h, 1))
                lib.check(L.amt_domain_sync(h))
            report = lib.GuardReport()
            lib.check(L.amt_domain_guard_report(h, ctypes.byref(report)))
        finally:
            L.amt_domain_destroy(h)
    what = f"{kind} {dims} {np.dtype(dtype).name} flags={flags} axes={axes} spec_bdy={spec} rotation={rotation} ({_label(pkg)})"
    return dpool.cpu().numpy(), want, lay, b, report, what


@pytest.mark.parametrize("kind", ["domain", "ensemble"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("dims,aligned", [((130, 13, 9), False), ((100, 20, 18), True)], ids=["130x13x9", "100x20x18-padded"])
def test_cyclic_refresh_sweep_zone_update_and_guard_on_one_handle(pkg, oracle, torch_mod, dims, aligned, dtype, kind):
    """amt_domain_wrap / amt_ensemble_wrap (3 members) over pool views with set_cyclic(CYCLIC_X), set_spec_bdy(1) and set_guard(1)
    armed TOGETHER on flags (1,1,0), a channel: per sweep the refresh, the sweep, the boundary-zone update, the guard.  The whole
    pool equals the host's; the guard has checked three sweeps and found nothing; the same run with spec_bdy off differs in
    exactly the zone cells of t, mu and muts that the reference update moves -- the update was enqueued behind the sweep.
    Then flags (0,0,0) with cyclic x|y and the guard (`specified` admits no cyclic y)."""
    flags = (1, 1, 0)
    for rotation in _rotations(dtype, ends_only=True):
        got, want, lay, b, report, what = _step_packed(pkg, oracle, torch_mod, kind, dims, aligned, dtype, rotation, flags, X, True)
        _assert_pool(got, want, lay, what)
        assert report.sweep == 0 and report.n_nonfinite == 0 and report.sweeps_checked == 3, (what, report)
        off, want_off, _lay, _b, report_off, what_off = _step_packed(pkg, oracle, torch_mod, kind, dims, aligned, dtype, rotation, flags, X, False)
        _assert_pool(off, want_off, lay, what_off)
        assert report_off.sweep == 0 and report_off.sweeps_checked == 3, (what_off, report_off)
        d = PS.diff(got, off, lay)
        assert d is not None and set(d["counts"]) == {"t", "mu", "muts"}, (what, d)
        zone = SB.zone_mask(flags, b)
        u = PS._uint(dtype)
        gv, ov, wv, wov = (PS.views(p, lay) for p in (got, off, want, want_off))
        for n in ("t", "mu", "muts"):
            moved = gv[n].view(u) != ov[n].view(u)
            z = zone if n != "t" else np.broadcast_to(zone[:, None, :], (b.jdim, b.kdim, b.idim)).copy()
            if n == "t":
                z[:, b.kte - b.kms:, :] = False                            # levels kts .. kte-1
            assert moved.any() and not (moved & ~np.broadcast_to(z, moved.shape)).any(), f"{what}: {n} moved outside the zone"
            assert np.array_equal(moved, wv[n].view(u) != wov[n].view(u)), f"{what}: {n} did not move where the reference update moves it"
        got, want, lay, b, report, what = _step_packed(pkg, oracle, torch_mod, kind, dims, aligned, dtype, rotation, (0, 0, 0), X | Y, False)
        _assert_pool(got, want, lay, what)
        assert report.sweep == 0 and report.sweeps_checked == 3, (what, report)


# ---------------------------------------------------------------------------------------------
# f: the one-shot host call on a host pool
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("dims", [(130, 13, 9), (37, 5, 11)], ids=["130x13x9", "37x5x11"])
def test_one_shot_host_call_on_a_host_pool(pkg, oracle, torch_mod, dims, dtype):
    """numpy views of one numpy pool through amt_advance_mu_t_f32/_f64: plain; the residency cache with its check mode, two
    sub-steps; cache and deferred outputs, two sub-steps, then the fetch.  The whole host pool is compared."""
    S = pkg.synth
    b = S.domain_bounds(*dims)
    for n, rotation in enumerate(_rotations(dtype, ends_only=True)):
        cfg = pkg.GridConfig(**FLAGS[(n + dims[2]) % 4])
        p0, lay, pool, once = _sweep_case(pkg, oracle, b, cfg, dtype, rotation, 1200, gdims=dims)
        twice = PS.clone(once)
        oracle.advance_mu_t(*_member(S, p0, PS.views(twice, lay, b), 0, 1).args())
        what = f"{dims} {np.dtype(dtype).name} flags={cfg} rotation={rotation}"

        host = PS.clone(pool)
        pkg.advance_mu_t(*_member(S, p0, PS.views(host, lay, b), 0, 1).args())
        _assert_pool(host, once, lay, "one-shot, " + what)

        host = PS.clone(pool)
        args = _member(S, p0, PS.views(host, lay, b), 0, 1).args()
        pkg.host_cache_enable(True, check=True)
        try:
            pkg.advance_mu_t(*args)
            pkg.advance_mu_t(*args)
        finally:
            pkg.host_cache_enable(False)
        _assert_pool(host, twice, lay, "cached one-shot, second sub-step, " + what)

        host = PS.clone(pool)
        args = _member(S, p0, PS.views(host, lay, b), 0, 1).args()
        pkg.host_cache_enable(True, check=True)
        pkg.host_defer(None, True)
        try:
            pkg.advance_mu_t(*args)
            pkg.advance_mu_t(*args)
            pkg.host_fetch(None)
        finally:
            pkg.host_defer(None, False)
            pkg.host_cache_enable(False, check=False)
        _assert_pool(host, twice, lay, "deferred one-shot, second sub-step, " + what)
