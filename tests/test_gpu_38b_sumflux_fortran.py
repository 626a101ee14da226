"""The flux averages from Fortran (include/amt_advance_mu_t.h section 14): advance_mu_t_driver with its 9th argument `nsmall`
runs an acoustic loop of that many sub-steps on a resident handle through the BIND(C) interfaces -- handle level with the
library's and with the caller's accumulators, pointer level, and on an ensemble -- and writes ru_m, rv_m, ww_m.  The files are
compared bit for bit with the oracle's sweeps followed by tests/sumflux_ref.py.  Without the argument the driver does what it
always did."""
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch  # noqa: F401  -- before the HIP library initialises: both must share one HIP runtime (lib.py)

import sumflux_ref as R
from conftest import bits_equal

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FDIR = ROOT / "wrf-model-cuda-sample_amd" / "fortran"
DIMS, SWEEPS, NSMALL, SEED = (37, 5, 11), 1, 3, 12345


@pytest.fixture(scope="module")
def drivers(pkg):
    r = subprocess.run(["make", "-C", str(FDIR), "all"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"no Fortran toolchain: {r.stderr[-300:]}")
    return {4: FDIR / "advance_mu_t_driver_f32", 8: FDIR / "advance_mu_t_driver_f64"}


@pytest.mark.parametrize("itemsize", [4, 8], ids=["f32", "f64"])
def test_driver_writes_the_flux_averages_of_its_loop(pkg, oracle, drivers, tmp_path, itemsize):
    dtype = np.float64 if itemsize == 8 else np.float32
    S = pkg.synth
    r = subprocess.run([str(drivers[itemsize]), *map(str, DIMS), str(SWEEPS), str(tmp_path), "0", "0", "0", str(NSMALL)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"flux averages over {NSMALL} sub-steps" in r.stdout and "flux averages of an ensemble of 1 members" in r.stdout
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted([f"{n}.bin" for n in S.OUTPUTS] + [f"{n}.bin" for n in R.ACCUMULATORS])
    # the state the driver's last loop accumulates: the seeded patch after NSMALL sweeps; u, v, ww do not change in between
    b = S.domain_bounds(*DIMS)
    want = S.make_patch(b, pkg.GridConfig(), dtype=dtype, seed=SEED, global_dims=DIMS)
    for _ in range(NSMALL):
        oracle.advance_mu_t(*want.args())
    acc = {n: np.zeros(b.shape("ww"), dtype) for n in R.ACCUMULATORS}
    for it in range(1, NSMALL + 1):
        R.sumflux(acc, want.arrays, b, it, NSMALL)
    for n in R.ACCUMULATORS:
        got = np.fromfile(tmp_path / f"{n}.bin", dtype=dtype).reshape(acc[n].shape)
        assert bits_equal(got, acc[n]), n
        assert float(np.abs(acc[n]).max()) > 0.0
