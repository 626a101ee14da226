"""The one timing check of the ensemble path, collected with the other clock-based tests after every parity file: 32 members
of 128 x 60 x 128 fp64 as ONE amt_ensemble are not slower than 32 amt_domain handles stepped one after the other.  The
launcher's cost model predicts a gain of tens of per cent there (one-row blocks against 32-row blocks, tests/test_ensemble_plan.py),
so a result inside the spread of A's own repeats means the batch plan is not in effect.  The measurement is
profiles/ensemble_ab.py's (one process, one stream, HIP events, after warm-up, A and B alternating)."""
import importlib.util
import statistics
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def _ab():
    spec = importlib.util.spec_from_file_location("amt_ensemble_ab", ROOT / "profiles" / "ensemble_ab.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_an_ensemble_is_not_slower_than_its_members_one_by_one(pkg):
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    members = 32
    ta, tb, label_a, label_b = _ab().measure(pkg, torch, np.float64, 128, 60, members, reps=5, sweeps=20)
    a, b = statistics.median(ta), statistics.median(tb)
    margin = max(ta) / min(ta)                       # the spread of A's own repeats in this run
    print(f"  A (32 handles) {a * 1e3:.2f} us per member-sweep, repeats {[round(x * 1e3, 2) for x in ta]} ({label_a})")
    print(f"  B (one ensemble) {b * 1e3:.2f} us per member-sweep, repeats {[round(x * 1e3, 2) for x in tb]} ({label_b})")
    print(f"  A / B = {a / b:.3f}, margin {margin:.3f}")
    assert f"members={members}" in label_b, label_b
    assert b <= a * margin, (ta, tb)
