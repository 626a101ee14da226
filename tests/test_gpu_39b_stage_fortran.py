"""The bracket of a Runge-Kutta stage from Fortran (include/amt_advance_mu_t.h section 15): advance_mu_t_driver with its 10th
argument `bracket` = 1 runs two stages whose acoustic loops of `nsmall` sub-steps lie between small_step_prep and
small_step_finish, through the BIND(C) interfaces -- handle level with the caller's arrays, pointer level, and on an ensemble --
and writes the arrays.  The files are compared bit for bit with the same calls made from Python on a handle of its own.
Without the argument the driver writes what it always did."""
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch  # noqa: F401  -- before the HIP library initialises: both must share one HIP runtime (lib.py)

import stage_ref as R
import sumflux_ref as SF
from conftest import bits_equal

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FDIR = ROOT / "wrf-model-cuda-sample_amd" / "fortran"
DIMS, SWEEPS, NSMALL, SEED = (37, 5, 11), 1, 3, 12345
STAGE_FILES = ("t", "ww", "t_1", "ww_1", "mu", "muts") + R.EXTRAS
# what the driver's second handle lends: t_old, mu_old, mu_save, mub and the heating of the second stage
LENT = dict(t_old="t", mu_old="mu", mu_save="muave", mub="mut", h_diabatic="ft")


@pytest.fixture(scope="module")
def drivers(pkg):
    r = subprocess.run(["make", "-C", str(FDIR), "all"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"no Fortran toolchain: {r.stderr[-300:]}")
    return {4: FDIR / "advance_mu_t_driver_f32", 8: FDIR / "advance_mu_t_driver_f64"}


def _run(driver, outdir, *more):
    r = subprocess.run([str(driver), *map(str, DIMS), str(SWEEPS), str(outdir), "0", "0", "0", str(NSMALL), *more],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("itemsize", [4, 8], ids=["f32", "f64"])
def test_driver_runs_two_stages_between_prep_and_finish(pkg, drivers, tmp_path, itemsize):
    dtype = np.float64 if itemsize == 8 else np.float32
    S = pkg.synth
    plain, bracketed = tmp_path / "plain", tmp_path / "bracketed"
    plain.mkdir()
    bracketed.mkdir()
    out = _run(drivers[itemsize], plain)
    assert "Runge-Kutta" not in out
    today = sorted([f"{n}.bin" for n in S.OUTPUTS] + [f"{n}.bin" for n in SF.ACCUMULATORS])
    assert sorted(p.name for p in plain.iterdir()) == today
    assert "Runge-Kutta" not in _run(drivers[itemsize], tmp_path, "0") and not list(tmp_path.glob("stage_*"))
    out = _run(drivers[itemsize], bracketed, "1")
    assert f"two Runge-Kutta stages of {NSMALL} sub-steps" in out and "a Runge-Kutta stage of an ensemble of 1 members" in out
    assert sorted(p.name for p in bracketed.iterdir()) == sorted(today + [f"stage_{n}.bin" for n in STAGE_FILES])
    for name in today:                                             # with the bracket the driver's other files are what they were
        assert (plain / name).read_bytes() == (bracketed / name).read_bytes(), name
    # the same calls from Python
    b = S.domain_bounds(*DIMS)
    cfg = pkg.GridConfig()
    mine = S.make_patch(b, cfg, dtype=dtype, seed=SEED, global_dims=DIMS, device="cuda:0", native_domain=True)
    lent = S.make_patch(b, cfg, dtype=dtype, seed=SEED + 1, global_dims=DIMS, device="cuda:0", native_domain=True)
    dom = mine.owner
    torch.cuda.synchronize()
    dom.set_scalars(mine.rdx, mine.rdy, mine.dts, mine.epssm)
    dom.set_stage(True, *[lent.arrays[LENT[name]] for name in R.EXTRAS])
    for rk_step in (1, 2):
        dom.stage_prep(rk_step)
        dom.step(NSMALL)
        dom.stage_finish(NSMALL, lent.arrays[LENT["h_diabatic"]] if rk_step == 2 else None)
    dom.sync()
    for name in STAGE_FILES:
        want = (lent.arrays[LENT[name]] if name in LENT else mine.arrays[name]).cpu().numpy()
        got = np.fromfile(bracketed / f"stage_{name}.bin", dtype=dtype).reshape(want.shape)
        assert bits_equal(got, want), name
    assert np.isfinite(mine.arrays["t"].cpu().numpy()[R.cell_mask(b, "t")]).all()
    dom.set_stage(False)
