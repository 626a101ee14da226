"""The ensemble moments from Fortran (include/amt_advance_mu_t.h section 13): advance_mu_t_driver with its 8th argument
`members` steps an amt_ensemble and writes mean / var / lo / hi of ww (handle level, memory), mu (handle level, window) and t
(pointer level, the memory less one cell on every side).  The files are compared bit for bit with tests/moments_ref.py on the
members of a Python Ensemble stepped from the same seed.  Without the argument the driver does what it always did."""
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch  # noqa: F401  -- before the HIP library initialises: both must share one HIP runtime (lib.py)

import moments_ref as R
from conftest import bits_equal
from special_values import same_up_to_nan_payload

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FDIR = ROOT / "wrf-model-cuda-sample_amd" / "fortran"
DIMS, SWEEPS, MEMBERS, SEED = (37, 5, 11), 2, 3, 12345
ENS_FILES = sorted(f"ens_{f}_{m}.bin" for f in ("ww", "mu", "t") for m in R.NAMES)


@pytest.fixture(scope="module")
def drivers(pkg):
    r = subprocess.run(["make", "-C", str(FDIR), "all"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"no Fortran toolchain: {r.stderr[-300:]}")
    return {4: FDIR / "advance_mu_t_driver_f32", 8: FDIR / "advance_mu_t_driver_f64"}


def _run(exe, outdir, *tail):
    outdir.mkdir()
    r = subprocess.run([str(exe), *map(str, DIMS), str(SWEEPS), str(outdir), "0", *tail], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("itemsize", [4, 8], ids=["f32", "f64"])
def test_driver_writes_the_moments_of_its_ensemble(pkg, oracle, drivers, tmp_path, itemsize):
    dtype = np.float64 if itemsize == 8 else np.float32
    S = pkg.synth
    plain = _run(drivers[itemsize], tmp_path / "plain")
    withm = _run(drivers[itemsize], tmp_path / "members", "0", str(MEMBERS))

    # without the 8th argument: the seven outputs and nothing else, the oracle's bits, no word of an ensemble
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == sorted(f"{n}.bin" for n in S.OUTPUTS)
    assert "ensemble" not in plain and "differing elements = 0" in plain
    b = S.domain_bounds(*DIMS)
    cfg = pkg.GridConfig()
    want = S.make_patch(b, cfg, dtype=dtype, seed=SEED, global_dims=DIMS)
    for _ in range(SWEEPS):
        oracle.advance_mu_t(*want.args())
    for n in S.OUTPUTS:
        got = np.fromfile(tmp_path / "plain" / f"{n}.bin", dtype=dtype).reshape(want.arrays[n].shape)
        assert bits_equal(got, want.arrays[n]), n
    # with it: the same seven files, byte for byte, and the twelve new ones
    assert sorted(p.name for p in (tmp_path / "members").iterdir()) == sorted(ENS_FILES + [f"{n}.bin" for n in S.OUTPUTS])
    for n in S.OUTPUTS:
        assert (tmp_path / "members" / f"{n}.bin").read_bytes() == (tmp_path / "plain" / f"{n}.bin").read_bytes(), n
    assert f"ensemble of {MEMBERS} members" in withm
    keep = lambda text: [l for l in text.splitlines() if l.startswith(("advance_mu_t ", "checksums", "one-shot vs", "deferred loop"))]
    assert keep(plain) == keep(withm) and len(keep(plain)) == 4

    ens = pkg.Ensemble(b, MEMBERS, cfg, dtype)
    try:
        ens.fill_synthetic(SEED, global_dims=DIMS)
        ens.step(SWEEPS)
        ens.sync()
        members = {n: np.stack([ens.download_member(n, m) for m in range(MEMBERS)]) for n in ("ww", "mu", "t")}
    finally:
        ens.close()
    ext = (b.ims, b.ime, b.jms, b.jme, b.kms, b.kme)
    i0, i1, j0, j1, k0, k1 = pkg.compute_window(cfg, b.ids, b.ide, b.jds, b.jde, b.its, b.ite, b.jts, b.jte, b.kts, b.kte)
    boxes = {"ww": (b.ims, b.ime, b.kms, b.kme, b.jms, b.jme), "mu": (i0, i1, k0, k1, j0, j1),
             "t": (b.ims + 1, b.ime - 1, b.kms + 1, b.kme - 1, b.jms + 1, b.jme - 1)}
    for f, a in members.items():
        idx = R.member_index(a, ext, boxes[f])
        ref = R.moments(a, ext, boxes[f])
        for n in R.NAMES:
            got = np.fromfile(tmp_path / "members" / f"ens_{f}_{n}.bin", dtype=dtype).reshape(a.shape[1:])
            assert same_up_to_nan_payload(got, R.expected(np.zeros(a.shape[1:], dtype), ref[n], idx)), (f, n)
        assert float(ref["var"].max()) > 0.0, f                          # the members differ: the test is not vacuous
