"""Properties of tests/hard_inputs.py that keep it free of the generator's symmetries (CPU only): every level of a column is
distinct, so no level repeats at k+8 or k+16 (the level counts of one march wave); fnp is not fl(1 - fnm); rdnw is 1/dnw in the
array's precision; no dts of SCALAR_SETS is a short dyadic number; the scalars reach a patch rounded to its precision."""
import numpy as np
import pytest

import hard_inputs as H

NKS = (2, 3, 8, 9, 17, 33, 40, 41, 60, 61, 241, 300)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nk", NKS)
def test_every_level_of_a_column_is_its_own(dtype, nk):
    t = np.dtype(dtype).type
    L = H.wrf_levels(nk, dtype, seed=7)
    dnw, rdnw = L["dnw"][:nk], L["rdnw"][:nk]                 # memory level 1 is index 0 (kms = 1)
    fnm, fnp = L["fnm"][1:nk], L["fnp"][1:nk]
    assert all(a.dtype == np.dtype(dtype) and a.shape == (nk + 1,) for a in L.values())
    assert len(set(dnw.tolist())) == nk and len(set(fnm.tolist())) == nk - 1 and len(set(fnp.tolist())) == nk - 1
    for name, col in (("dnw", dnw), ("rdnw", rdnw), ("fnm", fnm), ("fnp", fnp)):
        for d in (8, 16):
            assert not np.any(col[d:] == col[:-d]), f"{name}: a level equals the one {d} above it"
        assert not (len(col) > 2 and np.array_equal(col, col[::-1])), f"{name} is mirror-symmetric"
    assert np.array_equal(rdnw, (t(1) / dnw).astype(dtype))
    assert (dnw < 0).all() and abs(float(dnw.astype(np.float64).sum()) + 1.0) < 1e-5      # eta from 1 at the ground to 0 at the top
    if nk > 2:
        differs = fnp != (t(1) - fnm)
        assert differs.mean() > 0.75, f"fnp == 1 - fnm on {int((~differs).sum())} of {nk - 1} levels"
    # the levels the routine never reads (dnw, rdnw at kde; fnm, fnp at 1 and kde) hold finite values no read level has
    for name, unread, read in (("dnw", [nk], dnw), ("rdnw", [nk], rdnw), ("fnm", [0, nk], fnm), ("fnp", [0, nk], fnp)):
        v = L[name][unread]
        assert np.isfinite(v).all() and not np.isin(v, read).any(), name


def test_levels_are_seeded_and_follow_the_memory_extent():
    a = H.wrf_levels(40, np.float64, seed=3)
    b = H.wrf_levels(40, np.float64, seed=3, kms=-2, kme=44)
    c = H.wrf_levels(40, np.float64, seed=4)
    for n in H.RANK1:
        lo = 1 if n in ("fnm", "fnp") else 0                  # the levels the routine reads: 1..40 (fnm, fnp: 2..40)
        assert np.array_equal(a[n][lo:40], b[n][3 + lo:43]) and b[n].shape == (47,)
        assert len(set(b[n].tolist())) == 47, f"{n}: unread memory levels must be distinct"
    assert not np.array_equal(a["dnw"], c["dnw"])
    with pytest.raises(ValueError):
        H.wrf_levels(40, np.float64, seed=3, kme=40)


def test_scalar_sets_are_not_short_dyadic_numbers():
    assert len(H.SCALAR_SETS) >= 4
    dx_eq_dy = [k for k, s in H.SCALAR_SETS.items() if s["rdx"] == s["rdy"]]
    assert len(dx_eq_dy) == 1
    assert {0.1} < {s["epssm"] for s in H.SCALAR_SETS.values()} - {1.0}
    for name, s in H.SCALAR_SETS.items():
        for dtype in (np.float32, np.float64):
            r = H.rounded_scalars(s, dtype)
            assert H.significant_bits(r["dts"]) >= 20, (name, dtype)
            assert H.significant_bits(r["rdx"]) >= 20 and H.significant_bits(r["rdy"]) >= 20, (name, dtype)
    assert H.significant_bits(2.0) == 1 and H.significant_bits(0.1) > 50


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_apply_writes_the_metrics_and_the_rounded_scalars(pkg, dtype):
    S = pkg.synth
    b = S.domain_bounds(9, 12, 5).replace(kms=-1, kme=15)
    p = S.make_patch(b, pkg.GridConfig(), dtype=dtype, seed=1, global_dims=(9, 12, 5))
    before = {n: a.copy() for n, a in p.arrays.items()}
    L = H.levels_for(p, 5)
    H.apply(p, L, H.SCALAR_SETS["rk3_dx12km"])
    for n in S.FIELD_NAMES:
        if n in H.RANK1:
            assert np.array_equal(p.arrays[n], L[n]) and not np.array_equal(p.arrays[n], before[n])
        else:
            assert np.array_equal(p.arrays[n], before[n]), n
    t = np.dtype(dtype).type
    assert p.dts == float(t(20.0 / 3.0)) and p.rdx == float(t(1.0 / 12000.0)) and p.epssm == float(t(0.1))
    q = p.copy()
    assert (q.rdx, q.rdy, q.dts, q.epssm) == (p.rdx, p.rdy, p.dts, p.epssm)
