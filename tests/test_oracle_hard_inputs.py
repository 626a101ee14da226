"""The oracle, the reference Fortran and the build's Fortran CPU path on inputs without the generator's symmetries
(tests/hard_inputs.py: WRF-like vertical metrics, scalars with long mantissas), every shape of cases.SHAPES plus a tall
sub-tile, every flag combination, fp32 and fp64, each scalar set.  Anchored on tests/golden/hard_inputs_digests.json -- the
outputs of the reference Fortran itself (tests/golden/make_golden.py) -- and on the reference live where oracle/_ref exists.
Bit-exact; CPU only.  The golden files of the synthetic inputs cannot see an fnp rebuilt as 1 - fnm, a metric read from 8
levels away or dts*a + dts*b for dts*(a + b); these can."""
import json
from pathlib import Path

import numpy as np
import pytest

import cases
import hard_inputs as H
from conftest import bits_equal

DIGESTS = json.loads((Path(__file__).resolve().parent / "golden" / "hard_inputs_digests.json").read_text())


def test_the_digest_file_covers_every_case():
    assert sorted(DIGESTS) == sorted(H.hard_keys())
    assert any(rec["bounds"][4] - 1 >= 40 for rec in DIGESTS.values())


def _case(pkg, key):
    shape, flag, dtname, sset = key.split("/")
    p = H.hard_case(pkg, shape, flag, np.dtype(dtname), sset)
    rec = DIGESTS[key]
    assert list(p.bounds.as_tuple()) == rec["bounds"]
    assert [p.rdx, p.rdy, p.dts, p.epssm] == rec["scalars"]
    for n in H.RANK1:
        assert cases.digest(p.arrays[n]) == rec["metrics"][n], f"{key}: {n} drifted from the committed fixture"
    return p, rec


@pytest.mark.parametrize("key", sorted(DIGESTS))
def test_oracle_matches_reference_digests(pkg, oracle, key):
    p, rec = _case(pkg, key)
    oracle.advance_mu_t(*p.args())
    for n in pkg.synth.OUTPUTS:
        assert cases.digest(p.arrays[n]) == rec["outputs"][n], f"{key}: {n} differs from the reference Fortran"


@pytest.mark.parametrize("key", sorted(DIGESTS))
def test_fortran_cpu_path_matches_reference_digests(pkg, oracle, key):
    p, rec = _case(pkg, key)
    oracle.fortran_advance_mu_t(*p.args(), nthreads=3)
    for n in pkg.synth.OUTPUTS:
        assert cases.digest(p.arrays[n]) == rec["outputs"][n], f"{key}: {n} differs from the reference Fortran"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_oracle_matches_live_reference(pkg, oracle, dtype):
    if not oracle.have_ref(np.dtype(dtype).itemsize):
        pytest.skip("oracle/_ref is built only where the reference sources exist")
    for key in sorted(k for k in DIGESTS if k.split("/")[2] == np.dtype(dtype).name):
        p, _ = _case(pkg, key)
        q = p.copy()
        oracle.advance_mu_t(*p.args())
        oracle.ref_advance_mu_t(*q.args())
        for n in pkg.synth.FIELD_NAMES:
            assert bits_equal(p.arrays[n], q.arrays[n]), (key, n)


def test_the_new_inputs_change_every_output(pkg, oracle):
    """The metrics and the scalars both reach the answer: each alone moves every output but t_ave (the input t, copied) away
    from the synthetic run."""
    base = cases.make_case(pkg, "64x40x64", "specified", np.float64)
    runs = {}
    for what, levels, scalars in (("none", False, False), ("levels", True, False), ("scalars", False, True)):
        p = base.copy()
        H.apply(p, H.levels_for(p, H.LEVEL_SEED) if levels else None, H.SCALAR_SETS["rk3_dx12km"] if scalars else None)
        oracle.advance_mu_t(*p.args())
        runs[what] = p
    for what in ("levels", "scalars"):
        for n in pkg.synth.OUTPUTS:
            if n == "t_ave":
                continue
            assert not bits_equal(runs[what].arrays[n], runs["none"].arrays[n]), (what, n)
