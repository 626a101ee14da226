"""Specified / nested lateral boundaries without a GPU (include/amt_advance_mu_t.h section 12): the
numpy reference tests/specbdy_ref.py that the GPU tests compare against -- its zone is the tile minus the compute window, and
where its formulas coincide with the routine's they give the oracle's bits --, and the argument and precondition errors of
the pointer-level call, which are host arithmetic and are reported with or without a device."""
import ctypes

import numpy as np
import pytest

import cases
import specbdy_ref as SB

FLAG_SETS = [(0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1)]


def _tiles(b):
    """name -> bounds: the whole domain, the four corner tiles, the four edge tiles, an interior tile of a domain with at
    least 6 cells per side; the whole domain only for a smaller one."""
    out = {"whole": b}
    ni, nj = b.ide - b.ids, b.jde - b.jds
    if ni < 6 or nj < 6:
        return out
    ilo, imid, ihi = (b.ids, b.ids + 1), (b.ids + 2, b.ide - 3), (b.ide - 2, b.ide)
    jlo, jmid, jhi = (b.jds, b.jds + 1), (b.jds + 2, b.jde - 3), (b.jde - 2, b.jde)
    cols = dict(left=ilo, mid=imid, right=ihi)
    rows = dict(lower=jlo, mid=jmid, upper=jhi)
    for rn, (j0, j1) in rows.items():
        for cn, (i0, i1) in cols.items():
            out[f"{rn}-{cn}"] = b.replace(its=i0, ite=i1, jts=j0, jte=j1)
    return out


# ---------------------------------------------------------------------------------------------
# 1: zone and window partition the tile
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAG_SETS, ids=["".join(map(str, f)) for f in FLAG_SETS])
def test_zone_and_window_partition_the_tile(pkg, flags):
    S = pkg.synth
    seen = set()
    domains = [(12, 3, 9)] + [(ni, 2, nj) for ni in (1, 2, 3) for nj in (1, 2, 3)] + [(2, 2, 9), (12, 2, 2), (3, 2, 8)]
    for dims in domains:
        for name, b in _tiles(S.domain_bounds(*dims)).items():
            tile, win, zone = SB.tile_mask(b), SB.window_mask(flags, b), SB.zone_mask(flags, b)
            assert not (zone & win).any(), (dims, name)
            assert np.array_equal(zone | win, tile), (dims, name)
            assert not (win & ~tile).any(), (dims, name)
            i0, i1, j0, j1 = SB.window(flags, b)
            # the window as the library states it (amt_compute_window), where one can be built
            got = pkg.compute_window(pkg.GridConfig(bool(flags[0]), bool(flags[1]), bool(flags[2])), b.ids, b.ide, b.jds, b.jde,
                                     b.its, b.ite, b.jts, b.jte, b.kts, b.kte)
            assert got[:4] == (i0, i1, j0, j1), (dims, name)
            ni, nj = dims[0], dims[2]
            if name == "mid-mid":
                assert not zone.any(), "an interior tile has an empty zone"
                seen.add("interior")
            elif name == "whole" and (nj < 3 or (ni < 3 and not flags[0])):
                assert np.array_equal(zone, tile) and not win.any(), (dims, "window empty: every cell is zone")
                seen.add("empty-window")
            elif name == "whole":
                want = 2 * ni + (0 if flags[0] else 2 * (nj - 2))
                assert int(zone.sum()) == want, (dims, flags, int(zone.sum()), want)
                seen.add("ring")
            elif name in ("lower-left", "lower-right", "upper-left", "upper-right"):
                # a 2 x 2 (3 x 3 at the upper / right end: ite = ide is no mass point) corner tile: one row plus one column cell
                w = int(tile.sum()) ** 0.5
                assert int(zone.sum()) == (w if flags[0] else 2 * w - 1), (dims, name, flags)
                seen.add("corner")
            elif name in ("lower-mid", "upper-mid"):
                assert int(zone.sum()) == tile.shape[1] - 2 - 4 and zone.any(axis=1).sum() == 1, (dims, name)
                seen.add("row-edge")
            elif name in ("mid-left", "mid-right"):
                assert int(zone.sum()) == (0 if flags[0] else tile.shape[0] - 2 - 4), (dims, name)
                seen.add("column-edge")
    assert seen == {"interior", "empty-window", "ring", "corner", "row-edge", "column-edge"}, seen


def test_the_reference_touches_the_zone_only_and_each_cell_once(pkg):
    """All 26 arrays compared whole: t, mu, muts change in the zone (levels kts..kte-1) and nowhere else, by exactly one step."""
    S = pkg.synth
    for dtype in (np.float64, np.float32):
        for flags in FLAG_SETS:
            for aligned in (False, True):
                p = S.make_patch(S.domain_bounds(13, 4, 7, aligned=aligned), dtype=dtype, seed=3)
                b = p.bounds
                got = SB.spec_bdy_update({n: a.copy() for n, a in p.arrays.items()}, b, flags, p.dts)
                zone = SB.zone_mask(flags, b)
                s = np.dtype(dtype).type(p.dts)
                for n in S.FIELD_NAMES:
                    before, after = p.arrays[n], got[n]
                    if n not in SB.MAY_CHANGE:
                        assert np.array_equal(SB.as_bits(after), SB.as_bits(before)), n
                        continue
                    z = np.broadcast_to(zone[:, None, :], before.shape).copy() if before.ndim == 3 else zone
                    if before.ndim == 3:
                        z[:, b.kte - b.kms:, :] = False                     # level kte and above
                    tend = p.arrays["ft" if n == "t" else "mu_tend"]
                    assert np.array_equal(SB.as_bits(after)[~z], SB.as_bits(before)[~z]), n
                    assert np.array_equal(after[z], before[z] + s * tend[z]), n
                    assert (after[z] != before[z]).any(), n


@pytest.mark.parametrize("members", [1, 3])
def test_the_reference_treats_every_member_alone(pkg, members):
    S = pkg.synth
    ps = [S.make_patch(S.domain_bounds(12, 5, 9), dtype=np.float32, seed=20 + m) for m in range(members)]
    b = ps[0].bounds
    stacked = {n: (ps[0].arrays[n].copy() if S.field_rank(n) == 1 else np.stack([p.arrays[n] for p in ps])) for n in S.FIELD_NAMES}
    SB.spec_bdy_update(stacked, b, (0, 1, 0), ps[0].dts)
    for m, p in enumerate(ps):
        want = SB.spec_bdy_update({n: a.copy() for n, a in p.arrays.items()}, b, (0, 1, 0), p.dts)
        for n in S.FIELD_NAMES:
            got = stacked[n] if S.field_rank(n) == 1 else stacked[n][m]
            assert np.array_equal(SB.as_bits(got), SB.as_bits(want[n])), (n, m)


# ---------------------------------------------------------------------------------------------
# 2: argument and precondition errors of the pointer-level call: no device needed to reach them
# ---------------------------------------------------------------------------------------------
NAMES5 = ("t", "ft", "mu", "muts", "mu_tend")


def _update(L, fn, members, flags, b, ptrs, dts=2.0):
    return getattr(L, fn)(None, members, *ptrs, dts, *flags, *b.as_tuple())


@pytest.mark.parametrize("dtype,fn", [(np.float32, "amt_spec_bdy_update_device_f32"), (np.float64, "amt_spec_bdy_update_device_f64")],
                         ids=["f32", "f64"])
def test_errors_are_reported_without_a_device_and_touch_nothing(pkg, dtype, fn):
    L = pkg.load_library()
    p = cases.make_case(pkg, "16x8x16", "specified", dtype)
    b = p.bounds
    before = p.copy()
    ptrs = [p.arrays[n].ctypes.data_as(ctypes.c_void_p) for n in NAMES5]
    refused = [
        ("neither specified nor nested", 2, 1, (0, 0, 0), b, ptrs),
        ("periodic_x alone", 2, 1, (1, 0, 0), b, ptrs),
        ("a tile left of memory", 2, 1, (0, 1, 0), b.replace(ims=b.its + 1), ptrs),
        ("a tile right of memory", 2, 1, (0, 1, 0), b.replace(ime=b.ide - 2), ptrs),
        ("a tile below memory", 2, 1, (0, 0, 1), b.replace(jms=b.jts + 1), ptrs),
        ("a tile above memory", 2, 1, (0, 1, 0), b.replace(jme=b.jde - 2), ptrs),
        ("levels above memory", 2, 1, (0, 1, 0), b.replace(kme=b.kte - 2), ptrs),
        ("empty memory", 2, 1, (0, 1, 0), b.replace(kme=0), ptrs),
        ("no member", 3, 0, (0, 1, 0), b, ptrs),
        ("a negative member count", 3, -2, (0, 1, 0), b, ptrs),
    ] + [(f"{n} is NULL", 3, 1, (0, 1, 0), b, ptrs[:k] + [None] + ptrs[k + 1:]) for k, n in enumerate(NAMES5)]
    for what, status, members, flags, bb, pp in refused:
        assert _update(L, fn, members, flags, bb, pp) == status, (what, L.amt_last_error())
        assert L.amt_last_error(), what
    for n in pkg.synth.FIELD_NAMES:                                 # the refused calls touched nothing
        assert np.array_equal(SB.as_bits(p.arrays[n]), SB.as_bits(before.arrays[n])), n
    for name in ("amt_domain_spec_bdy_update", "amt_ensemble_spec_bdy_update"):
        assert getattr(L, name)(None) == 3, name
    for name in ("amt_domain_set_spec_bdy", "amt_ensemble_set_spec_bdy"):
        assert getattr(L, name)(None, 1) == 3, name
    assert L.amt_domain_spec_bdy(None) == 0 and L.amt_ensemble_spec_bdy(None) == 0
    # an interior tile: an empty zone is AMT_OK and needs no device either
    inner = b.replace(its=b.ids + 2, ite=b.ide - 3, jts=b.jds + 2, jte=b.jde - 3)
    assert _update(L, fn, 1, (0, 1, 0), inner, ptrs) == 0, L.amt_last_error()
    assert _update(L, fn, 1, (1, 0, 1), b.replace(jts=b.jds + 1, jte=b.jde - 2), ptrs) == 0, L.amt_last_error()
    # a well-formed call: no CPU fallback, an error status without a device
    if L.amt_device_count() == 0:
        assert _update(L, fn, 1, (0, 1, 0), b, ptrs) in (1, 4), L.amt_last_error()
        with pytest.raises(TypeError):
            pkg.spec_bdy_update(*[p.arrays[n] for n in NAMES5], p.dts, p.config, *b.as_tuple())      # numpy arrays: no host path
        for n in pkg.synth.FIELD_NAMES:
            assert np.array_equal(SB.as_bits(p.arrays[n]), SB.as_bits(before.arrays[n])), n


# ---------------------------------------------------------------------------------------------
# 3: the anchor to the reference Fortran
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_where_the_formulas_coincide_the_reference_gives_the_oracles_bits(pkg, oracle, dtype):
    """With u = v = u_1 = v_1 = 0, t_1 = 0 and msfty = 1 the routine itself computes the zone's formulas
    (module_small_step_em.f90): :142-147 give dvdxi = 0 and dmdt = 0, so :153 is mu + dts*mu_tend; :212 is t + (1*dts)*ft;
    :227 gives wdtn = ww*0 = 0 and :237-246 subtract dts*1*(msftx*0 + rdnw*0) = 0 from a non-zero t.  The zeros may be of
    either sign; every one of them is added to or subtracted from a non-zero number, or (dmdt + mu_tend) to a non-zero
    mu_tend, so no sign of zero reaches a result.  So the oracle with flags (0,0,0) -- unclipped -- must hold, in the cells
    that form the zone under `specified`, bit for bit what the numpy reference's zone update under `specified` makes of the
    same inputs.  muts is not anchored: :155 is mut + mu, another rounding."""
    p = cases.make_case(pkg, "16x8x16", "none", dtype)
    for n in ("u", "v", "u_1", "v_1", "t_1"):
        p.arrays[n][...] = 0
    p.arrays["msfty"][...] = 1
    b = p.bounds
    assert (p.arrays["ft"] != 0).all() and (p.arrays["mu_tend"] != 0).all() and (p.arrays["mu"] != 0).all() and (p.arrays["t"] != 0).all()
    want = SB.spec_bdy_update({n: a.copy() for n, a in p.arrays.items()}, b, (0, 1, 0), p.dts)
    ran = p.copy()
    oracle.advance_mu_t(*ran.with_bounds().args())
    zone = SB.zone_mask((0, 1, 0), b)
    assert int(zone.sum()) == 2 * 16 + 2 * 14
    K = slice(b.kts - b.kms, b.kte - 1 - b.kms + 1)
    jj, ii = np.nonzero(zone)
    assert np.array_equal(SB.as_bits(ran.arrays["mu"][jj, ii]), SB.as_bits(want["mu"][jj, ii]))
    assert np.array_equal(SB.as_bits(ran.arrays["t"][jj, K, ii]), SB.as_bits(want["t"][jj, K, ii]))
    assert not np.array_equal(want["mu"][jj, ii], p.arrays["mu"][jj, ii]) and not np.array_equal(want["t"][jj, K, ii], p.arrays["t"][jj, K, ii])
    # outside the zone the reference changed nothing, the oracle everything
    assert np.array_equal(SB.as_bits(want["mu"][~zone]), SB.as_bits(p.arrays["mu"][~zone]))
    if oracle.have_ref(np.dtype(dtype).itemsize):                  # the reference Fortran itself, where it has been built
        ref = p.copy()
        oracle.ref_advance_mu_t(*ref.args())
        assert np.array_equal(SB.as_bits(ref.arrays["mu"][jj, ii]), SB.as_bits(want["mu"][jj, ii]))
        assert np.array_equal(SB.as_bits(ref.arrays["t"][jj, K, ii]), SB.as_bits(want["t"][jj, K, ii]))
