"""calc_p_rho on the GPU where a wave leaves the first segment of its first unit (tests/prho_long_rows.py has the list and what
each shape exercises): rows of up to three wave segments with short last segments, more than 4096 units so that waves take a
second and a third one and carry from segment to row, level groups on several segments, members, and one stage on a created
domain whose rows take three segments.  The pointer-level call against tests/prho_ref.py with the machinery of
tests/test_gpu_41_p_rho.py: NaN with distinct payloads wherever the contract does not read, every one of the 13 arrays compared
whole and as bytes, p finite on the cells and NaN outside.  tests/test_prho_host.py runs the same list through the kernel's
text on the host: a difference here at a shape that is equal there is not in the index arithmetic."""
import numpy as np
import pytest

import prho_long_rows as LR
import test_gpu_41_p_rho as T41
from test_gpu_41_p_rho import torch_mod  # noqa: F401  -- the fixture

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
TYPES = pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])


def _run(pkg, torch, cases):
    for seed, c in enumerate(cases):
        T41._one_call(pkg, torch, LR.bounds(pkg, c), c.dtype, c.mode, c.step, 100 + seed, c.members, patterns=LR.nan_patterns)


@pytest.mark.parametrize("layout", LR.LAYOUTS, ids=["aligned", "one-element-later", "unpadded"])
@TYPES
def test_rows_of_one_to_three_segments(pkg, torch_mod, dtype, layout):
    """ni in {S - 1, S, S + 1, S + P - 1, S + P + 1, 2S + 3, 3S}, one and three rows, mode 2 on 3 levels and mode 1 on GROUP + 1,
    step 0 and 1."""
    cases = LR.segment_cases(dtype, layout)
    assert len(cases) == 56
    _run(pkg, torch_mod, cases)


@pytest.mark.parametrize("mode", [1, 2], ids=["nonhydrostatic", "hydrostatic"])
@pytest.mark.parametrize("shape", [0, 1, 2], ids=["8197-rows-of-one-segment", "1400-rows-of-three", "2800-rows-of-three"])
@TYPES
def test_waves_that_take_several_units(pkg, torch_mod, dtype, shape, mode):
    """More than 4096 units: a second and a third unit per wave, and with three segments a row the carry; aligned and unpadded
    rows, step 1."""
    cases = LR.unit_cases(dtype, LR.unit_shapes(dtype)[shape], mode)
    assert all(LR.measures(c)["most"] >= 2 for c in cases)
    _run(pkg, torch_mod, cases)


@TYPES
def test_three_members_on_rows_of_two_segments(pkg, torch_mod, dtype):
    _run(pkg, torch_mod, LR.member_cases(dtype))


@pytest.mark.parametrize("mode", [1, 2], ids=["nonhydrostatic", "hydrostatic"])
@TYPES
def test_one_stage_on_a_created_domain_with_long_rows(pkg, oracle, torch_mod, dtype, mode):
    """test_gpu_41_p_rho.test_two_stages_on_a_domain's sequence -- prep, the step-0 diagnosis, two sweeps with the zone update,
    the flux accumulation and the diagnosis behind each, finish -- on a domain whose rows take three segments."""
    T41._stages_on_a_domain(pkg, oracle, torch_mod, dtype, "created", LR.HANDLE_DIMS[dtype], ((1, 2, mode),))
