"""The acoustic loop's momentum update advance_uv on the GPU (include/amt_advance_mu_t.h section 17):
the pointer-level call against tests/uv_ref.py.  Every array of a call is compared WHOLE and as bytes, outputs and inputs,
which catches a write outside the ranges; the arrays hold NaN with distinct payloads in every cell the contract neither reads
nor writes, so a stray read shows as a NaN in u or v.  A NaN the arithmetic made equals any NaN
(tests/special_values.py), everything else its bits."""
import itertools

import numpy as np
import pytest

import packed_state as PS
import uv_ref as R
from special_values import same_up_to_nan_payload

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
SCALARS = dict(rdx=1.0e-3, rdy=1.25e-3, dts=2.0, cf1=1.5, cf2=-0.75, cf3=0.25, emdiv=0.01)
GROUP = 8                              # AMT_UV_GROUP of csrc/amt_uv_kernel.h: the levels of one group
# every flag set amt_compute_window admits: (periodic_x, specified, nested)
FLAGS = [(0, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 0)]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def _flags(f):
    return dict(periodic_x=bool(f[0]), specified=bool(f[1]), nested=bool(f[2]))


def _bounds(pkg, tile, ni, nk, nj, kms=0):
    """A tile of ni x nj columns and kde = nk levels.  whole: the tile is the domain (ite == ide, jte == jde: the u part
    reaches column ide, the v part row jde); interior: no clipping, the neighbours at its-1 and jts-1 are halo cells."""
    B = pkg.synth.Bounds
    if tile == "whole":
        return B(ids=1, ide=ni, jds=1, jde=nj, kde=nk, ims=0, ime=ni + 1, jms=0, jme=nj + 1, kms=kms, kme=nk + 1,
                 its=1, ite=ni, jts=1, jte=nj, kts=1, kte=nk)
    return B(ids=1, ide=ni + 20, jds=1, jde=nj + 12, kde=nk, ims=3, ime=ni + 7, jms=2, jme=nj + 5, kms=kms, kme=nk + 1,
             its=5, ite=ni + 4, jts=4, jte=nj + 3, kts=1, kte=nk)


def _to_device(torch, arrays):
    return {n: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for n, a in arrays.items()}


def _call(pkg, dev, b, nh, flags, members=1, stream=None):
    f = _flags(flags)
    pkg.advance_uv(nh, *[dev[n] for n in R.NAMES], *[SCALARS[k] for k in ("rdx", "rdy", "dts", "cf1", "cf2", "cf3", "emdiv")],
                   f["periodic_x"], f["specified"], f["nested"], *b.as_tuple(), members=members, stream=stream)


def _check(dev, want, what):
    for name, w in want.items():
        got = dev[name].cpu().numpy()
        assert same_up_to_nan_payload(got, w) if name in R.OUT_3D else got.tobytes() == w.tobytes(), (what, name)


def _one_call(pkg, torch, b, dtype, nh, flags, seed, members=1):
    want = R.make_state(b, dtype, seed, nh, members, **_flags(flags))
    dev = _to_device(torch, want)
    _call(pkg, dev, b, nh, flags, members)
    torch.cuda.synchronize()
    R.advance_uv(want, b, nh, **SCALARS, **_flags(flags))
    _check(dev, want, (nh, flags, b.as_tuple()))
    for name in R.OUT_3D:                                          # the reference read no poison: the cells are finite, the rest NaN
        cells = np.broadcast_to(R.cell_mask(b, name, **_flags(flags)), want[name].shape)
        assert np.isfinite(want[name][cells]).all() and np.isnan(want[name][~cells]).all()
    return want


@pytest.mark.parametrize("nh", [1, 0], ids=["nonhydrostatic", "hydrostatic"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_small_tiles(pkg, torch_mod, dtype, nh):
    """Rows shorter than a 16-byte chunk, tails of one to three elements, whole chunks; one and three rows; kde 2 and 3
    (hydrostatic only), 4, 5 and, for the level groups, G + 1, G + 2 and 2G; crossed with every flag set and with the
    whole-domain and the interior tile.  On the whole-domain tile the clipped flag sets leave both parts, one part alone (the u
    part without the v part and the reverse) or no cell at all: every one of them is a case, the empty ones must change nothing."""
    seed, parts = 0, set()
    for kde in ((2, 3) if not nh else ()) + (4, 5, GROUP + 1, GROUP + 2, 2 * GROUP):
        for ni, nj in itertools.product((1, 2, 3, 4, 5, 7, 8, 9), (1, 3)):
            for tile in ("whole", "interior"):
                for flags in FLAGS:
                    seed += 1
                    b = _bounds(pkg, tile, ni, kde, nj)
                    parts.add(tuple(bool(R.cell_mask(b, name, **_flags(flags)).any()) for name in R.OUT_3D))
                    _one_call(pkg, torch_mod, b, dtype, nh, flags, seed)
    assert parts == {(True, True), (True, False), (False, True), (False, False)}


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "p%ds%dn%d" % f)
@pytest.mark.parametrize("tile", ["whole", "interior"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_every_flag_set_on_a_tile_of_several_chunks(pkg, torch_mod, dtype, tile, flags):
    """13 x 9 columns, 6 levels, memory levels below kts (kms = -2): every flag set on both tiles, both modes."""
    for nh in (0, 1):
        _one_call(pkg, torch_mod, _bounds(pkg, tile, 13, 6, 9, kms=-2), dtype, nh, flags, seed=11)


@pytest.mark.parametrize("nh", [1, 0], ids=["nonhydrostatic", "hydrostatic"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_rows_of_sixteen_elements_take_the_wide_path(pkg, torch_mod, dtype, nh):
    """Memory rows of 16 and 32 elements (a multiple of 16 bytes) whose tile starts on and off a boundary: with torch's
    aligned allocations every array has one phase, so whole chunks move as 16-byte accesses where the run starts on one."""
    B = pkg.synth.Bounds
    for ims, ime, its in ((0, 15, 4), (0, 15, 3), (1, 32, 5), (-3, 28, 1)):
        b = B(ids=-20, ide=60, jds=-5, jde=20, kde=5, ims=ims, ime=ime, jms=0, jme=5, kms=1, kme=5,
              its=its, ite=ime - 1, jts=1, jte=4, kts=1, kte=5)
        _one_call(pkg, torch_mod, b, dtype, nh, (0, 0, 0), seed=ims + 9)


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_every_phase_of_every_array_in_packed_pools(pkg, torch_mod, dtype, members):
    """The 24 arrays back to back in ONE pool (tests/packed_state.py), every array at every 16-byte phase over the rotations,
    in two orders, on a tile with odd row lengths (15 elements) and memory levels below kts (kms = -2); with three members the
    member strides are off 16 bytes as well.  Both forms on the same pool; whole pools are compared: outputs, inputs and guard
    bands.  A second pool has rows of 16 elements and every array on one phase: the 16-byte path where the phase is 0."""
    torch = torch_mod
    per = 16 // np.dtype(dtype).itemsize
    B = pkg.synth.Bounds
    odd = B(ids=1, ide=13, jds=1, jde=9, kde=5, ims=0, ime=14, jms=0, jme=10, kms=-2, kme=6, its=1, ite=13, jts=1, jte=9, kts=1, kte=5)
    padded = B(ids=-9, ide=40, jds=1, jde=9, kde=5, ims=1, ime=16, jms=0, jme=4, kms=0, kme=6, its=2, ite=16, jts=1, jte=3, kts=1, kte=5)
    flags = (0, 0, 0)
    for b, orders in ((odd, (R.NAMES, R.NAMES[::-1])), (padded, (R.NAMES,))):
        seen = {name: set() for name in R.NAMES}
        for order in orders:
            shapes = {name: R.shape(b, name, members) for name in order}
            for rotation in range(per):
                lay = PS.layout(b, dtype, members=members, rotation=rotation, names=shapes)
                if b is padded:                                    # one phase for all: the rotation's
                    at = 0
                    for name in lay.names:
                        base = at + lay.guard
                        lay[name] = base + (rotation - base) % per
                        at = lay.end(name)
                    lay.length = at + lay.guard
                for nh in (1, 0):
                    want_pool = PS.place(R.make_state(b, dtype, 40 + rotation, nh, members, **_flags(flags)), lay)
                    dev_pool = torch.from_numpy(want_pool).to("cuda:0")
                    assert dev_pool.data_ptr() % 128 == 0
                    dev, want = PS.views(dev_pool, lay), PS.views(want_pool, lay)
                    _call(pkg, dev, b, nh, flags, members)
                    torch.cuda.synchronize()
                    R.advance_uv(want, b, nh, **SCALARS, **_flags(flags))
                    bad = PS.diff(dev_pool.cpu().numpy(), want_pool, lay)
                    assert bad is None, (rotation, nh, bad)
                for name in R.NAMES:
                    seen[name].add(lay.phase_bytes(name))
        assert all(len(v) == per for v in seen.values()), seen


@pytest.mark.parametrize("nh", [1, 0], ids=["nonhydrostatic", "hydrostatic"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_long_rows_and_more_units_than_waves(pkg, torch_mod, dtype, nh):
    """A row of three wave segments with a short tail, ni = 2 * 64 * (16 / sizeof T) + 3; and nj = 4100 rows of three columns
    with kde = 4: more units than the launch's 1024 blocks of four waves hold, so waves take a second unit."""
    per = 16 // np.dtype(dtype).itemsize
    _one_call(pkg, torch_mod, _bounds(pkg, "interior", 2 * 64 * per + 3, 4, 2), dtype, nh, (0, 0, 0), seed=3)
    _one_call(pkg, torch_mod, _bounds(pkg, "whole", 3, 4, 4100), dtype, nh, (0, 1, 0), seed=4)


@pytest.mark.parametrize("nh", [1, 0], ids=["nonhydrostatic", "hydrostatic"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_three_members_equal_three_single_calls(pkg, torch_mod, dtype, nh):
    """Member strides off 16 bytes (11 x 7 x 9 = 693 elements, 99 for the 2-D arrays): one launch over three members
    against the reference on the stack, and against the single call on each member alone."""
    torch = torch_mod
    b = _bounds(pkg, "interior", 6, 5, 5)
    assert (b.idim * b.kdim * b.jdim) % 2 == 1 and (b.idim * b.jdim) % 2 == 1
    flags = (0, 1, 0)
    want = _one_call(pkg, torch, b, dtype, nh, flags, seed=21, members=3)
    start = R.make_state(b, dtype, 21, nh, 3, **_flags(flags))
    for m in range(3):
        one = {n: (a if R.RANK[n] == 1 else a[m]).copy() for n, a in start.items()}
        dev = _to_device(torch, one)
        _call(pkg, dev, b, nh, flags)
        torch.cuda.synchronize()
        for name in R.OUT_3D:
            assert same_up_to_nan_payload(dev[name].cpu().numpy(), want[name][m]), (m, name)


def test_refusals_leave_the_device_arrays_alone(pkg, torch_mod):
    """non_hydrostatic with kde < 4, and a tile whose neighbour column lies outside memory: AMT_ERR_PRECONDITION, nothing
    enqueued, every array as it was."""
    torch = torch_mod
    for b, nh, text in ((_bounds(pkg, "interior", 5, 3, 3), 1, "kde = 3"),
                        (_bounds(pkg, "interior", 5, 5, 3).replace(ims=5), 0, "the cells read, 4:")):
        want = R.make_state(b, F64, 1, 0, poison=False)
        dev = _to_device(torch, want)
        with pytest.raises(pkg.AmtError) as e:
            _call(pkg, dev, b, nh, (0, 0, 0))
        assert e.value.status == 2 and text in str(e.value), str(e.value)
        torch.cuda.synchronize()
        for name, w in want.items():
            assert dev[name].cpu().numpy().tobytes() == w.tobytes(), name
