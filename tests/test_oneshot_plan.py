"""The host arithmetic of the one-shot call -- chunk plan and arena layout, csrc/amt_oneshot_plan.h -- checked by a stand-alone
host program (tests/oneshot_plan_check.cpp) built with the undefined-behaviour sanitizer (array bounds included): no GPU, no HIP call."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_plan_and_layout_hold_over_shapes_regimes_and_knobs(tmp_path):
    exe = tmp_path / "oneshot_plan_check"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-D_GLIBCXX_ASSERTIONS",
                        "-D__HIP_PLATFORM_AMD__", "-I", f"{rocm}/include", "-I", str(ROOT / "wrf-model-cuda-sample_amd" / "csrc"),
                        str(ROOT / "tests" / "oneshot_plan_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith("AMT_")}     # the program sets the knobs itself
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout
