"""Build-time resource check of the flux-average kernel (wrf-model-cuda-sample_amd/csrc/amt_sumflux.hip): a streaming pass of
256 threads with no LDS and no scratch, in both precisions, as reported by the compiler's own kernel-resource-usage remarks in
csrc/build/sumflux_resources.txt (`make -C csrc check` fails the build on scratch).  No GPU needed."""
from pathlib import Path

from resource_remarks import _kernels

ROOT = Path(__file__).resolve().parent.parent
REMARKS = ROOT / "wrf-model-cuda-sample_amd" / "csrc" / "build" / "sumflux_resources.txt"


def test_the_flux_average_kernel_has_no_scratch_and_no_lds(pkg):
    assert REMARKS.exists(), "the build writes csrc/build/sumflux_resources.txt"
    kernels = {k: v for k, v in _kernels(REMARKS).items() if "amt_sumflux_kernel" in k}
    assert len(kernels) == 2, sorted(kernels)                      # float and double
    for name, r in kernels.items():
        assert r["ScratchSize"] == 0, (name, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] == 0, (name, r)
        assert r["VGPRs"] <= 64, (name, r)                         # eight waves per SIMD: a streaming kernel lives on them
