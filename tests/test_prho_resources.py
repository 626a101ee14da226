"""Build-time resource check of the pressure-diagnosis kernel (wrf-model-cuda-sample_amd/csrc/amt_p_rho.hip): a streaming pass
of 256 threads with no LDS and no scratch, float and double, both modes, as reported by the compiler's own
kernel-resource-usage remarks in csrc/build/p_rho_resources.txt (`make -C csrc check` fails the build on scratch).  No GPU
needed."""
import re
from pathlib import Path

from resource_remarks import _kernels

ROOT = Path(__file__).resolve().parent.parent
REMARKS = ROOT / "wrf-model-cuda-sample_amd" / "csrc" / "build" / "p_rho_resources.txt"


def test_the_p_rho_kernels_have_no_scratch_no_spills_and_no_lds(pkg):
    assert REMARKS.exists(), "the build writes csrc/build/p_rho_resources.txt"
    kernels = {k: v for k, v in _kernels(REMARKS).items() if "amt_p_rho_kernel" in k}
    # amt_p_rho_kernel<T, MODE>: I<f|d>Li<1|2>E in the mangled name
    assert sorted(re.search(r"amt_p_rho_kernelI([fd])Li([12])E", k).groups() for k in kernels) == [("d", "1"), ("d", "2"), ("f", "1"), ("f", "2")]
    for name, r in kernels.items():
        assert r["ScratchSize"] == 0, (name, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] == 0, (name, r)
        assert r["VGPRs"] <= 64, (name, r)                         # eight waves per SIMD: a streaming kernel lives on them
