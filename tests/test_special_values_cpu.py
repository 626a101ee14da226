"""The oracle, the reference Fortran and the build's Fortran CPU path on special values (tests/special_values.py): exact and
negative zeros, subnormals, overflow, planted NaN / Inf / zero divisors and NaN in every cell the routine does not read.
Anchored on tests/golden/special_values_digests.json -- the outputs of the reference Fortran itself, every NaN mapped to one bit
pattern (cases.digest_canonical_nan) -- and on the reference live where oracle/_ref exists.  CPU only.

The conditions below are asserted on the ORACLE's outputs, so that no regime is empty and no comparison of the GPU tests
(tests/test_gpu_17b_special_values.py) is hollow.

Footprint of ONE plant at (i, k, j) of the window (37x5x11_ragged, k_end = 5), from the oracle; NaN, +Inf and -Inf give the same
cells; a column or row outside the window drops out (first_column, first_row, the halo places).  `*` = levels 1..k_end of t and
2..k_end of ww (through dmdt: every level of the column), 2-D = mu, muave, muts, mudf.

    field               columns (di, dj)              non-finite outputs
    u u_1 muu msfuy     (-1, 0) (0, 0)                ww *, t *, 2-D          msfuy = +-Inf: finite everywhere (x / Inf = 0)
    v v_1 muv msfvx_inv (0, -1) (0, 0)                ww *, t *, 2-D
    mu_tend msftx msfty (0, 0)                        ww *, t *, 2-D          msftx = 0: finite (a factor, not a divisor)
    msfty = 0           (0, 0)                        ww *, t *               (x / 0 in ww only; mu and its kin stay finite)
    ww   (level 1)      (0, 0)                        ww 1..k_end, t 1..k_end
    ww_1                (0, 0)                        ww k, t k-1..k
    t                   (0, 0)                        t k, t_ave k
    ft                  (0, 0)                        t k
    t_1                 (0, 0)                        t k-1..k+1 (wdtn(k), wdtn(k+1))
                        (-1, 0) (1, 0) (0, -1) (0, 1) t k
    mu                  (0, 0)                        mu, muave, muts
    mut                 (0, 0)                        muts                    mut = 0: nothing (muts = 0 + mu); mut enters only muts
"""
import json
from pathlib import Path

import numpy as np
import pytest

import cases
import special_values as SV
from conftest import bits_equal

DIGESTS = json.loads((Path(__file__).resolve().parent / "golden" / "special_values_digests.json").read_text())
REGIME_KEYS = SV.regime_keys()
# read by the Fortran at that cell, yet every output stays finite: x / (+-Inf) = +-0, 0 * x = 0, 0 + mu
FINITE_PLANTS = {("msfuy", "+inf"), ("msfuy", "-inf"), ("msftx", "zero"), ("mut", "zero")}
NAN_CAP = 0.25


def test_the_digest_file_covers_every_case():
    assert sorted(DIGESTS) == sorted(REGIME_KEYS + SV.plant_keys())
    assert len(REGIME_KEYS) == 3 * 4 * 2 * len(SV.REGIMES)


def test_window_is_the_librarys(pkg):
    for key in REGIME_KEYS[::len(SV.REGIMES)]:
        p = SV.special_case(pkg, key.rsplit("/", 1)[0] + "/rest")
        b = p.bounds
        assert SV.window(p) == tuple(pkg.compute_window(p.config, b.ids, b.ide, b.jds, b.jde, b.its, b.ite, b.jts, b.jte, b.kts, b.kte))


def _digests(pkg, p):
    return {n: cases.digest_canonical_nan(p.arrays[n]) for n in pkg.synth.OUTPUTS}


def _plant_digest(pkg, p):
    return cases.digest(np.concatenate([SV.canonical_nan(p.arrays[n]).view(np.uint8).ravel() for n in pkg.synth.OUTPUTS]))


def _win(p, n):
    return p.arrays[n][SV.window_index(p, n)]


def _nonfinite_share(p):
    return {n: float(np.isnan(_win(p, n)).mean()) for n in SV.OUTPUTS}


@pytest.fixture(scope="module")
def oracle_runs(pkg, oracle):
    """key -> (patch before, patch after the oracle), computed once for the tests below."""
    runs = {}

    def get(key):
        if key not in runs:
            before = SV.special_case(pkg, key)
            after = before.copy()
            oracle.advance_mu_t(*after.args())
            runs[key] = (before, after)
        return runs[key]
    return get


@pytest.mark.parametrize("key", REGIME_KEYS)
def test_oracle_matches_reference_digests(pkg, oracle_runs, key):
    before, p = oracle_runs(key)
    rec = DIGESTS[key]
    assert list(p.bounds.as_tuple()) == rec["bounds"] and [p.rdx, p.rdy, p.dts, p.epssm] == rec["scalars"]
    assert _digests(pkg, p) == rec["outputs"], f"{key}: differs from the reference Fortran"


@pytest.mark.parametrize("key", REGIME_KEYS)
def test_fortran_cpu_path_matches_reference_digests(pkg, oracle, key):
    p = SV.special_case(pkg, key)
    oracle.fortran_advance_mu_t(*p.args(), nthreads=3)
    assert _digests(pkg, p) == DIGESTS[key]["outputs"], f"{key}: differs from the reference Fortran"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_single_plants_match_reference_digests(pkg, oracle, oracle_runs, dtype):
    for key in (k for k in SV.plant_keys() if k.split("/")[2] == np.dtype(dtype).name):
        _, p = oracle_runs(key)
        assert _plant_digest(pkg, p) == DIGESTS[key]["outputs"], f"oracle, {key}: differs from the reference Fortran"
        q = SV.special_case(pkg, key)
        oracle.fortran_advance_mu_t(*q.args(), nthreads=2)
        assert _plant_digest(pkg, q) == DIGESTS[key]["outputs"], f"Fortran CPU path, {key}: differs from the reference Fortran"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_oracle_matches_live_reference(pkg, oracle, oracle_runs, dtype):
    if not oracle.have_ref(np.dtype(dtype).itemsize):
        pytest.skip("oracle/_ref is built only where the reference sources exist")
    for key in (k for k in REGIME_KEYS + SV.plant_keys() if k.split("/")[2] == np.dtype(dtype).name):
        before, p = oracle_runs(key)
        q = before.copy()
        oracle.ref_advance_mu_t(*q.args())
        for n in pkg.synth.FIELD_NAMES:
            assert SV.same_up_to_nan_payload(p.arrays[n], q.arrays[n]), (key, n, SV.first_difference(p.arrays[n], q.arrays[n]))
            if n not in pkg.synth.OUTPUTS:
                assert bits_equal(q.arrays[n], before.arrays[n]), (key, n)
            else:
                assert SV.outside_window_bits_equal(q, n, q.arrays[n], before.arrays[n]), (key, n)
                assert SV.outside_window_bits_equal(p, n, p.arrays[n], before.arrays[n]), (key, n)


# ---------------------------------------------------------------------------------------------
# no regime is empty
# ---------------------------------------------------------------------------------------------
def _keys(regime):
    return [k for k in REGIME_KEYS if k.endswith("/" + regime)]


def test_rest_stays_at_rest(oracle_runs):
    for key in _keys("rest"):
        _, p = oracle_runs(key)
        for n in ("ww", "t", "mu", "mudf", "muave", "t_ave"):
            w = _win(p, n)
            assert (w == 0).all() and not np.signbit(w).any(), f"{key}: {n} is not +0.0 throughout"


def test_signed_zeros_reach_every_advanced_field(oracle_runs):
    for key in _keys("signed_zeros"):
        _, p = oracle_runs(key)
        for n in ("ww", "mu", "t"):
            w = _win(p, n)
            zero = w == 0
            assert (zero & np.signbit(w)).any() and (zero & ~np.signbit(w)).any(), f"{key}: {n} lacks a -0.0 or a +0.0"


def test_denormal_outputs_are_subnormal(oracle_runs):
    for key in _keys("denormal"):
        _, p = oracle_runs(key)
        for n in ("ww", "t"):
            w = _win(p, n)
            sub = (np.abs(w) < np.finfo(w.dtype).tiny) & (w != 0)
            assert sub.mean() >= 0.01 and (w == 0).mean() <= 0.5, f"{key}: {n}: {sub.mean():.3f} subnormal, {(w == 0).mean():.3f} zero"
            assert np.isfinite(w).all()


def test_overflow_makes_both_infinities_and_nan_from_finite_inputs(oracle_runs):
    for key in _keys("overflow"):
        before, p = oracle_runs(key)
        assert all(np.isfinite(a).all() for a in before.arrays.values()), f"{key}: an input is not finite"
        outs = [_win(p, n) for n in SV.OUTPUTS]
        assert any((w == np.inf).any() for w in outs) and any((w == -np.inf).any() for w in outs), key
        assert any(np.isnan(w).any() for w in outs), key
        share = _nonfinite_share(p)
        assert max(share.values()) <= NAN_CAP, f"{key}: NaN share {share}"


def test_composite_plants_are_apart_and_leave_most_cells_comparable(oracle_runs):
    for key in _keys("planted_composite"):
        before, p = oracle_runs(key)
        sites = SV.composite_sites(before, SV.SEED)
        assert len(sites) >= 3, key
        i1 = SV.window(before)[1]
        assert any(i == i1 + 1 for _, _, (i, _k, _j) in sites), f"{key}: no plant in the halo column"
        for a, (_, _, (ia, _ka, ja)) in enumerate(sites):
            for _, _, (ib, _kb, jb) in sites[a + 1:]:
                assert abs(ia - ib) >= 4 or abs(ja - jb) >= 2, (key, sites)
        share = _nonfinite_share(p)
        assert max(share.values()) <= NAN_CAP, f"{key}: NaN share {share}"
        assert any(not np.isfinite(_win(p, n)).all() for n in SV.OUTPUTS), key


def test_unread_poison_changes_no_output_bit(pkg, oracle, oracle_runs):
    """What defines `unread`: NaN (two bit patterns) in every cell outside special_values.read_mask -- halos beyond the
    stencil's, corners, i_start - 1 of the u family, j_start - 1 of the v family, levels outside 1..kde - 1, ww above level 1,
    the INTENT(OUT) arrays -- and the oracle's window is bit-equal to its window on the clean patch."""
    for key in _keys("unread_poison"):
        before, p = oracle_runs(key)
        clean = SV.base_case(pkg, *key.split("/")[:2], np.dtype(key.split("/")[2]))
        poisoned = sum(int(np.isnan(before.arrays[n]).sum()) for n in before.arrays)
        assert poisoned > 0
        for n in ("u", "v", "t_1", "ww", "t_ave", "dnw", "fnm"):
            assert np.isnan(before.arrays[n]).any(), f"{key}: nothing of {n} is poisoned"
        bits = before.arrays["t_1"][np.isnan(before.arrays["t_1"])].view(np.uint64 if p.arrays["t"].itemsize == 8 else np.uint32)
        assert len(set(bits.tolist())) == 2, "two NaN bit patterns"
        oracle.advance_mu_t(*clean.args())
        for n in SV.OUTPUTS:
            assert bits_equal(_win(p, n), _win(clean, n)), f"{key}: {n} changed: the oracle reads a poisoned cell"
            assert np.isfinite(_win(p, n)).all()
            assert SV.outside_window_bits_equal(p, n, p.arrays[n], before.arrays[n]), f"{key}: {n} written outside the window"


# ---------------------------------------------------------------------------------------------
# single plants: the footprint table of the module docstring, as code
# ---------------------------------------------------------------------------------------------
def expected_footprint(p, field, value, site):
    """{output: bool array over the window} of the non-finite cells one plant at ``site`` = (i, k, j) makes (the table above)."""
    i0, i1, j0, j1, _k0, ke = SV.window(p)
    i, k, j = site
    masks = {n: np.zeros(_win(p, n).shape, bool) for n in SV.OUTPUTS}
    if (field, value) in FINITE_PLANTS:
        return masks

    def mark(n, di, dj, klo=None, khi=None):
        ci, cj = i + di, j + dj
        if not (i0 <= ci <= i1 and j0 <= cj <= j1):
            return
        if masks[n].ndim == 3:
            masks[n][cj - j0, max(klo, 1) - 1:min(khi, ke), ci - i0] = True
        else:
            masks[n][cj - j0, ci - i0] = True

    def column(di, dj, two_d=("mu", "muave", "muts", "mudf")):
        mark("ww", di, dj, 2, ke)
        mark("t", di, dj, 1, ke)
        for n in two_d:
            mark(n, di, dj)

    if field in ("u", "u_1", "muu", "msfuy"):
        column(-1, 0), column(0, 0)
    elif field in ("v", "v_1", "muv", "msfvx_inv"):
        column(0, -1), column(0, 0)
    elif field in ("mu_tend", "msftx", "msfty"):
        column(0, 0, () if (field, value) == ("msfty", "zero") else ("mu", "muave", "muts", "mudf"))
    elif field == "ww":
        mark("ww", 0, 0, 1, ke), mark("t", 0, 0, 1, ke)
    elif field == "ww_1":
        mark("ww", 0, 0, k, k), mark("t", 0, 0, k - 1, k)
    elif field == "t":
        mark("t", 0, 0, k, k), mark("t_ave", 0, 0, k, k)
    elif field == "ft":
        mark("t", 0, 0, k, k)
    elif field == "t_1":
        mark("t", 0, 0, k - 1, k + 1)
        for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            mark("t", di, dj, k, k)
    elif field == "mu":
        for n in ("mu", "muave", "muts"):
            mark(n, 0, 0)
    elif field == "mut":
        mark("muts", 0, 0)
    else:
        raise KeyError(field)
    return masks


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_single_plant_footprints(pkg, oracle, oracle_runs, dtype):
    name = np.dtype(dtype).name
    clean = SV.base_case(pkg, SV.PLANT_SHAPE, "none", dtype)
    oracle.advance_mu_t(*clean.args())
    seen_finite = set()
    for field, value, where in SV.single_plants():
        key = f"{SV.PLANT_SHAPE}/none/{name}/plant:{field}:{value}:{where}"
        before, p = oracle_runs(key)
        want = expected_footprint(p, field, value, SV.site(before, field, where))
        for n in SV.OUTPUTS:
            assert np.array_equal(~np.isfinite(_win(p, n)), want[n]), f"{key}: footprint in {n}"
            assert SV.outside_window_bits_equal(p, n, p.arrays[n], before.arrays[n]), (key, n)
        assert max(_nonfinite_share(p).values()) <= NAN_CAP, key
        changed = any(not bits_equal(_win(p, n), _win(clean, n)) for n in SV.OUTPUTS)
        if (field, value) in FINITE_PLANTS:
            seen_finite.add((field, value))
            assert not any(m.any() for m in want.values())
            # read there, by the Fortran: it changes finite output bits (mut = 0: that cell of muts = mut + mu)
            assert changed, f"{key}: the plant changes nothing"
        else:
            assert any(m.any() for m in want.values()), f"{key}: no non-finite output cell"
    assert seen_finite == FINITE_PLANTS


def test_mut_enters_muts_alone(oracle_runs):
    """module_small_step_em.f90:151-157: mut enters only muts = mut + mu.  A NaN there is that cell of muts; mut = 0 leaves
    every output finite and changes that cell of muts alone."""
    for dt in ("float32", "float64"):
        _, nan = oracle_runs(f"{SV.PLANT_SHAPE}/none/{dt}/plant:mut:nan:interior")
        _, zero = oracle_runs(f"{SV.PLANT_SHAPE}/none/{dt}/plant:mut:zero:interior")
        for n in SV.OUTPUTS:
            assert np.isfinite(zero.arrays[n]).all()
            same = bits_equal(nan.arrays[n], zero.arrays[n])
            assert same == (n != "muts"), n
        assert int(np.isnan(nan.arrays["muts"]).sum()) == 1
        i, _k, j = SV.site(zero, "mut", "interior")
        b = zero.bounds
        assert zero.arrays["muts"][j - b.jms, i - b.ims] == zero.arrays["mu"][j - b.jms, i - b.ims]


def test_same_up_to_nan_payload():
    for dt, u in ((np.float32, np.uint32), (np.float64, np.uint64)):
        a = np.array([1.0, -0.0, np.inf, np.nan, np.finfo(dt).tiny / 4], dtype=dt)
        b = a.copy()
        b[3] = SV.quiet_nan(dt, negative=True)
        b.view(u)[3] |= u(5)
        assert SV.same_up_to_nan_payload(a, b) and not bits_equal(a, b)
        for cell, other in ((1, 0.0), (2, -np.inf), (3, 1.0), (0, np.nan), (4, 0.0)):
            c = b.copy()
            c[cell] = other
            assert not SV.same_up_to_nan_payload(a, c), (cell, other)
        assert not SV.same_up_to_nan_payload(a, b.astype(np.float64 if dt is np.float32 else np.float32))
        assert not SV.same_up_to_nan_payload(a, b[:-1])
        assert cases.digest_canonical_nan(a) == cases.digest_canonical_nan(b) != cases.digest(b)
