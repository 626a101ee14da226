"""Build-time resource check of the stage-bracket kernels (wrf-model-cuda-sample_amd/csrc/amt_stage.hip): streaming passes of
256 threads with no LDS and no scratch, in both precisions, as reported by the compiler's own kernel-resource-usage remarks in
csrc/build/stage_resources.txt (`make -C csrc check` fails the build on scratch).  No GPU needed."""
from pathlib import Path

from resource_remarks import _kernels

ROOT = Path(__file__).resolve().parent.parent
REMARKS = ROOT / "wrf-model-cuda-sample_amd" / "csrc" / "build" / "stage_resources.txt"
KERNELS = ("amt_stage_prep3_kernel", "amt_stage_prep2_kernel", "amt_stage_finish_kernel")


def test_the_stage_kernels_have_no_scratch_no_spills_and_no_lds(pkg):
    assert REMARKS.exists(), "the build writes csrc/build/stage_resources.txt"
    kernels = {k: v for k, v in _kernels(REMARKS).items() if "amt_stage_" in k and "kernel" in k}
    for base in KERNELS:
        assert len([k for k in kernels if base in k]) == 2, (base, sorted(kernels))          # float and double
    assert len(kernels) == 2 * len(KERNELS), sorted(kernels)      # every instantiation is one of the three
    for name, r in kernels.items():
        assert r["ScratchSize"] == 0, (name, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] == 0, (name, r)
        assert r["VGPRs"] <= 64, (name, r)                         # eight waves per SIMD: a streaming kernel lives on them
