"""The long-row list of the pressure diagnosis (tests/prho_long_rows.py) without a GPU: the list has every feature the kernel's
control flow distinguishes at least twice in both types, the layouts are what they claim to be, and the reference alone, run
over every shape on the poisoned state the GPU test uses, leaves p and al finite on every cell of the range and NaN outside."""
import time
from pathlib import Path

import numpy as np
import pytest

import prho_long_rows as LR
import prho_ref as R
import test_gpu_41_p_rho as T41

TYPES = pytest.mark.parametrize("dtype", LR.DTYPES, ids=["f64", "f32"])


def test_the_constants_are_the_kernels():
    """The lines the constants restate are in the sources."""
    csrc = Path(__file__).resolve().parent.parent / "wrf-model-cuda-sample_amd" / "csrc"
    kernel, launcher = (csrc / "amt_p_rho_kernel.h").read_text(), (csrc / "amt_p_rho.hip").read_text()
    assert f"constexpr unsigned kSeg = {LR.SEG_CHUNKS} * kPer;" in kernel
    assert f"constexpr int kPer = {LR.CHUNK_BYTES} / (int)sizeof(T);" in kernel
    assert f"#define AMT_P_RHO_GROUP {LR.GROUP}\n" in kernel and LR.GROUP == T41.GROUP
    assert f"long blocks = (units + {LR.WAVES_PER_BLOCK - 1}) / {LR.WAVES_PER_BLOCK};" in launcher and f"dim3({64 * LR.WAVES_PER_BLOCK})" in launcher
    assert f"if (blocks > {LR.MAX_BLOCKS}) blocks = {LR.MAX_BLOCKS};" in launcher


@TYPES
def test_every_feature_occurs_at_least_twice(dtype):
    cases = LR.all_cases(dtype)
    count = {f: 0 for f in LR.FEATURES}
    for c in cases:
        for f, has in LR.features(c).items():
            count[f] += bool(has)
    assert all(n >= 2 for n in count.values()), count
    # and what the issue states of the three shapes with more than 4096 units
    S = LR.seg(dtype)
    one, three, third = [LR.Case("units", dtype, *shape, 1, 2, 1, "a") for shape in LR.unit_shapes(dtype)]
    assert LR.measures(one) == dict(segs=1, units=8197, most=3, carry=False, idle=False, full_wide=False, groups=1)
    assert LR.measures(three) == dict(segs=3, units=4200, most=2, carry=True, idle=True, full_wide=True, groups=1)
    assert LR.measures(third)["units"] == 8400 and LR.measures(third)["most"] == 3 and LR.measures(third)["carry"]
    assert three.ni == 2 * S + 5 and LR.launcher_blocks(three) == LR.MAX_BLOCKS
    # lengths on both sides of one and of two segments, a short chunk behind a full segment, whole segments only
    assert {LR.measures(c)["segs"] for c in cases} == {1, 2, 3}
    assert any(c.ni % S == 0 and c.ni > S for c in cases) and any(c.ni % LR.per(dtype) for c in cases)


@TYPES
def test_the_layouts_are_what_they_claim(pkg, dtype):
    P = LR.per(dtype)
    for c in LR.all_cases(dtype):
        b = LR.bounds(pkg, c)
        assert (b.ite - b.its + 1, b.kte - b.kts, b.jte - b.jts + 1) == (c.ni, c.nk, c.nj)
        assert b.ite < b.ide - 1 and b.jte < b.jde - 1 and b.ims < b.its and b.ite < b.ime      # nothing clipped, poison on both sides
        assert (b.idim, b.its - b.ims) == LR.row_geometry(c)
        first3 = ((b.jts - b.jms) * b.kdim + (b.kts - b.kms)) * b.idim + (b.its - b.ims)
        if c.layout == "a":
            assert b.idim % P == 0 and first3 % P == 0 and LR.wide_rows(c)
        elif c.layout == "b":
            assert b.idim % P == 0 and first3 % P == 1 and not LR.wide_rows(c)
        else:
            assert b.idim % P != 0 and not LR.wide_rows(c)
    assert max(int(np.prod(R.shape(LR.bounds(pkg, c), "t", c.members))) for c in LR.all_cases(dtype)) < 6.5e6


@TYPES
def test_the_reference_alone_is_finite_on_the_range_and_nan_outside(pkg, dtype):
    spent = 0.0
    for seed, c in enumerate(LR.all_cases(dtype)):
        b = LR.bounds(pkg, c)
        a = T41._state(b, c.dtype, 100 + seed, c.mode, c.step, c.members, LR.nan_patterns)
        t0 = time.perf_counter()
        R.p_rho(a, b, c.mode, c.step, T41.T0, T41.SMDIV)
        spent += time.perf_counter() - t0
        cells = np.broadcast_to(R.cell_mask(b, "t"), a["p"].shape)
        for name in ("p", "al"):
            assert np.isfinite(a[name][cells]).all() and np.isnan(a[name][~cells]).all(), (c, name)
    print(f"  {LR.dtype_name(dtype)}: the reference over the list: {spent:.2f} s")


def test_the_poison_is_the_original_where_that_is_defined():
    for dtype in LR.DTYPES:
        for tag in (0, 5, 12):
            assert T41.bits_equal(LR.nan_patterns((7, 5, 11), dtype, tag), T41.T38._nan_patterns((7, 5, 11), dtype, tag))
        big = LR.nan_patterns(((1 << 22) + 100,), dtype, 12)
        assert np.isnan(big).all() and ((R.as_bits(big) & 0x3FFFFF) != 0).all()
