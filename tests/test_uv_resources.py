"""Build-time resource check of the momentum-update kernel (wrf-model-cuda-sample_amd/csrc/amt_uv.hip): a streaming pass of
256 threads with no LDS, no scratch and no spills, float and double, both forms, as reported by the compiler's own
kernel-resource-usage remarks in csrc/build/uv_resources.txt (`make -C csrc check` fails the build on scratch).  No GPU
needed."""
import re
from pathlib import Path

from resource_remarks import _kernels

ROOT = Path(__file__).resolve().parent.parent
REMARKS = ROOT / "wrf-model-cuda-sample_amd" / "csrc" / "build" / "uv_resources.txt"


def test_the_uv_kernels_have_no_scratch_no_spills_and_no_lds(pkg):
    assert REMARKS.exists(), "the build writes csrc/build/uv_resources.txt"
    kernels = {k: v for k, v in _kernels(REMARKS).items() if "amt_uv_kernel" in k}
    # amt_uv_kernel<T, NH>: I<f|d>Lb<0|1>E in the mangled name
    assert sorted(re.search(r"amt_uv_kernelI([fd])Lb([01])E", k).groups() for k in kernels) == [("d", "0"), ("d", "1"), ("f", "0"), ("f", "1")]
    for name, r in kernels.items():
        assert r["ScratchSize"] == 0, (name, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] == 0, (name, r)
        assert r["VGPRs"] <= 128, (name, r)                        # four waves per SIMD at least
