"""The randomised geometry campaign (tests/random_geometry.py, played on the GPU by tests/test_gpu_12b_random_geometry.py) has
teeth: without a GPU, (1) the cases drawn with the default seed and the default counts contain every geometry the streaming
kernels decide on, (2) cases in which nothing may be written stay under a tenth of a family, and (3) every mutant -- a
deliberately wrong variant of a numpy reference, the shape of a bug these kernels could plausibly have -- put in the device's
place and pushed through the campaign's own comparison is caught by at least one drawn case of its family.  The kernels are not
mutated and nothing wrong is ever run on a device."""
import numpy as np
import pytest

import random_geometry as G

TILE_FAMILIES = tuple(f for f in G.FAMILIES if f not in G.BOX_FAMILIES)
_CASES = {}
_WANT = {}


def _cases(family):
    """The default campaign of a family: default seed, default count (whatever AMT_GEOM_* say)."""
    if family not in _CASES:
        _CASES[family] = list(G.cases(family, G.DEFAULT_CASES[family], G.DEFAULT_SEED))
    return _CASES[family]


def _want(case, ref, pkg):
    """The reference's play of a case; kept for the small cases, which several mutants of a family look at."""
    key = (case.family, case.number)
    if key in _WANT:
        return _WANT[key]
    want = G.run(case, ref, pkg)
    if not case.mid:
        _WANT[key] = want
    return want


@pytest.fixture(scope="module")
def ref(pkg, oracle):
    return G.RefOps(pkg, oracle)


@pytest.mark.parametrize("family", G.FAMILIES)
def test_the_default_campaign_contains_every_geometry(pkg, family):
    cs = _cases(family)
    assert len(cs) == G.DEFAULT_CASES[family]
    what = lambda text: f"{family}, seed {G.DEFAULT_SEED}, {len(cs)} cases: no draw with {text}"
    for dtype in (G.F64, G.F32):
        p = G.per(dtype)
        mine = [c for c in cs if c.dtype is dtype]
        phases = {G.run_geometry(c)[0] % p for c in mine}
        tails = {G.run_geometry(c)[1] % p for c in mine if G.run_geometry(c)[1] > 0}
        assert phases == set(range(p)), what(f"every 16-byte phase of the tile's first element ({np.dtype(dtype).name}: {sorted(phases)})")
        assert tails == set(range(p)), what(f"every tail length ({np.dtype(dtype).name}: {sorted(tails)})")
    assert {c.bounds.idim % 2 for c in cs} == {0, 1}, what("odd and even idim")
    assert any(G.member_stride_off_16(c) for c in cs), what("a member stride off 16 bytes")
    assert {c.bounds.kms for c in cs} == set(G.KMS_SET), what("each of kms = 1, 0, -2")
    assert any(c.bounds.kme > c.bounds.kde for c in cs), what("kme > kde")
    assert any(c.bounds.its == c.bounds.ite for c in cs), what("a one-column tile")
    assert any(c.bounds.jts == c.bounds.jte for c in cs), what("a one-row tile")
    assert any(G.grid_stride(c) for c in cs), what("more work items than one pass of the launch grid")
    if family in TILE_FAMILIES:
        b = [c.bounds for c in cs]
        assert any(x.ite == x.ide and x.jte < x.jde for x in b), what("ite == ide and jte < jde")
        assert any(x.jte == x.jde and x.ite < x.ide for x in b), what("jte == jde and ite < ide")
        assert any(x.its == x.ids for x in b) and any(x.its > x.ids for x in b), what("its == ids, and its > ids")
        assert {c.flags for c in cs} == set(G.admitted_flag_sets(family)), what("every admitted flag set")
    if family == "cyclic":
        assert {c.params["axes"] for c in cs} == {1, 2, 3}, what("cyclic x, y and both")
    if family == "handles":
        assert {c.params["axes"] for c in cs} == {0, 1, 2, 3}, what("no cyclic axis, x, y and both")
        assert {c.params["kind"] for c in cs} == {"domain", "ensemble"}
        assert {(c.params["spec_bdy"], c.params["stage"], c.params["sumflux"] > 0) for c in cs} >= {(a, s, f) for a in (False, True)
                                                                                                   for s in (False, True) for f in (False, True)}
    if family == "ensemble":
        assert {c.members for c in cs} == {2, 3, 4} and {c.params["register"] for c in cs} == {False, True}
    if family == "stage":
        assert {(c.params["rk_step"], c.params["with_h"]) for c in cs} == {(r, h) for r in (1, 2, 3) for h in (False, True)}
        assert {c.params["n"] for c in cs} == {1, 2, 3, 4}
    if family == "sumflux":
        assert {c.params["n"] for c in cs} == {1, 2, 3, 4}
    if family == "moments":
        assert {c.params["rank"] for c in cs} == {2, 3} and {len(c.params["want"]) for c in cs} == {1, 2, 3, 4}


@pytest.mark.parametrize("family", G.FAMILIES)
def test_cases_in_which_nothing_may_be_written_are_there_but_rare(pkg, family):
    cs = _cases(family)
    empty = sum(G.empty_contract(c) for c in cs)
    assert empty <= 0.10 * len(cs), (family, empty, len(cs))
    print(f"{family}: {empty} of {len(cs)} default draws have an empty contract range")
    if family in ("ensemble", "cyclic", "spec_bdy", "stage", "handles"):             # the families that can have one
        assert empty >= 1, f"{family}: not one empty range in the {len(cs)} draws of the default campaign"


def test_cells_no_call_reads_are_poisoned_in_the_sweep_families(pkg):
    """Families a and h start from synth.make_patch, which fills every cell: every cell outside the read masks must hold a NaN
    and every cell inside them a finite value, in every member, and the poison must come back with every refresh of the
    exchanged inputs."""
    for family, masks_of in (("ensemble", G.sweep_read_masks), ("handles", G.handles_read_masks)):
        for case in _cases(family)[:25]:
            if case.mid:
                continue
            S = pkg.synth
            stacked, scalars = G.ensemble_state(case, pkg, masks_of)
            if case.members == 1:                                  # a domain's arrays have no member axis (as handles_state)
                stacked = {n: (a if S.field_rank(n) == 1 else a[0]) for n, a in stacked.items()}
            for sweep in (None, 0):
                if sweep is not None:
                    if family != "handles":
                        break
                    G.refresh_exchanged(case, pkg, stacked, scalars, sweep)
                for m in range(case.members):
                    one = {n: (a if S.field_rank(n) == 1 or case.members == 1 else a[m]) for n, a in stacked.items()}
                    for n, read in masks_of(case, pkg, one).items():
                        assert np.isfinite(one[n][read]).all() and np.isnan(one[n][~read]).all(), (case.what(), n, m, sweep)
            assert any(np.isnan(a).any() for a in stacked.values())


def test_a_draw_is_a_function_of_the_seed(pkg):
    for family in G.FAMILIES:
        one = [c.what() for c in G.cases(family, 12, 5)]
        assert one == [c.what() for c in G.cases(family, 12, 5)]
        assert one != [c.what() for c in G.cases(family, 12, 6)]
        assert all(f"seed 5, family {family}, case {k}: bounds=(" in text for k, text in enumerate(one))


def test_the_vectorised_accumulation_is_the_reference_bit_for_bit(pkg, ref):
    """Mid-sized sumflux draws go through random_geometry.sumflux_vec (the reference loops cell by cell in Python): on every small
    draw of the campaign the two agree in every bit of every array after every iteration."""

    class Vec(G.RefOps):
        def sumflux(self, acc, inp, case, iteration, n):
            G.sumflux_vec(acc, inp, case.bounds, iteration == 1, iteration == n, n, case.members)

    vec, seen = Vec(), 0
    for case in _cases("sumflux"):
        if case.mid:
            continue
        bad = G.first_difference(case, G.run(case, vec, pkg), _want(case, ref, pkg))
        assert bad is None, bad
        seen += 1
    assert seen >= 0.9 * G.DEFAULT_CASES["sumflux"]


@pytest.mark.parametrize("mutant", G.MUTANTS, ids=[m.__name__ for m in G.MUTANTS])
def test_every_mutant_is_caught_by_a_drawn_case(pkg, oracle, ref, mutant):
    """The mutant's play of the family's script in the device's place: the campaign's comparison must name a difference in at
    least one case of the default campaign.  A mutant that survives means the generator misses a geometry."""
    wrong = mutant(pkg, oracle)
    for case in _cases(mutant.family):
        if case.mid:
            continue                                               # a small case does it, and quicker
        bad = G.first_difference(case, G.run(case, wrong, pkg), _want(case, ref, pkg))
        if bad is not None:
            print(f"mutant {mutant.__name__} ({mutant.what}): caught by {bad}")
            assert f"seed {G.DEFAULT_SEED}, family {mutant.family}, case {case.number}: bounds={case.bounds.as_tuple()}" in bad
            return
    raise AssertionError(f"mutant {mutant.__name__} ({mutant.what}) survives all {len(_cases(mutant.family))} cases of {mutant.family}")


def test_the_comparison_itself(pkg, ref):
    """One flipped bit anywhere in any array of a play is a difference, and its text carries seed, case number and bounds; a
    sum inside diag_ref's bound is none, one outside it is."""
    case = next(c for c in _cases("stage") if not c.mid and not G.empty_contract(c) and c.members > 1)
    want = _want(case, ref, pkg)
    assert G.first_difference(case, G.run(case, ref, pkg), want) is None
    got = G.run(case, ref, pkg)
    got[1][1]["mu_old"].reshape(-1).view(np.uint8)[-1] ^= 1          # the last byte of an input of finish
    bad = G.first_difference(case, got, want)
    assert bad and "mu_old" in bad and f"case {case.number}" in bad and str(case.bounds.as_tuple()) in bad and f"seed {G.DEFAULT_SEED}" in bad
    case = next(c for c in _cases("diag") if c.params["planted"] == 0 and not c.mid)
    want = _want(case, ref, pkg)
    got = G.run(case, ref, pkg)
    rec, w = got[0][1]["records"][0], want[0][1]["records"][0]
    import diag_ref as DR
    bound = DR.sum_bound(w["count"], w["abs_sum"])
    rec["sum"] = w["sum"] + 0.5 * bound
    assert G.first_difference(case, got, want) is None
    rec["sum"] = w["sum"] + 2.0 * bound + 1e-300
    assert "sum" in G.first_difference(case, got, want)
    rec["sum"], rec["count"] = w["sum"], w["count"] + 1
    assert "count" in G.first_difference(case, got, want)
