"""The one timing check of the cyclic boundary refresh, collected with the other clock-based tests after every parity file.
On one 4096 x 60 x 4096 fp64 amt_domain_create handle, A = plain amt_domain_step and B = the same with set_cyclic(X | Y)
alternate, 6 repeats of 10 sweeps each through amt_domain_step_timed (profiles/cyclic_ab.py).

    model    = bytes the refresh touches (a full 128-byte line read and a full line written per column element, the row runs
               as they are) / the sweep's algorithmic bytes W * NI * NJ * (11 * NK + 14): computed from the shapes
    spread_A = (max - min) / median of A's repeats in the same run

    assert median(B) <= median(A) * (1 + 4 * model + spread_A)

The factor 4 leaves room for the launch gap between the refresh and the march launch, which the byte model does not see."""
import importlib.util
import statistics
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def _ab():
    spec = importlib.util.spec_from_file_location("amt_cyclic_ab", ROOT / "profiles" / "cyclic_ab.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_refresh_costs_what_its_bytes_cost(pkg):
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    dims = (4096, 60, 4096)
    b = pkg.synth.domain_bounds(*dims, aligned=True)
    need = 10 * b.idim * b.kdim * b.jdim * 8 * 1.05
    if torch.cuda.mem_get_info(0)[0] < need:
        pytest.skip(f"needs {need / 1e9:.0f} GB of free HBM")
    ta, tb, model, label = _ab().measure_domain(pkg, torch, dims, reps=6, sweeps=10)
    # the model, restated here from the shapes: 4 three-dimensional and 2 two-dimensional columns and rows per refresh
    ni, nk, nj = dims
    cols, rows = 4 * b.kdim * nj + 2 * nj, 4 * b.kdim * ni + 2 * ni
    want_model = (cols * 2 * 128 + rows * 2 * 8) / (8 * ni * nj * (11 * nk + 14))
    assert abs(model - want_model) < 1e-12 and 0.001 < model < 0.01, (model, want_model)
    a, bm = statistics.median(ta), statistics.median(tb)
    spread_a = (max(ta) - min(ta)) / a
    print(f"  A (plain)  {a:.4f} ms per sweep, repeats {[round(x, 4) for x in ta]} ({label})")
    print(f"  B (cyclic) {bm:.4f} ms per sweep, repeats {[round(x, 4) for x in tb]}")
    print(f"  B / A = {bm / a:.5f}, model {model:.5f}, spread_A {spread_a:.5f}, bound {1 + 4 * model + spread_a:.5f}")
    assert bm <= a * (1 + 4 * model + spread_a), (ta, tb, model, spread_a)
