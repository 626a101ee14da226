"""The pressure-diagnosis kernel's own text -- wrf-model-cuda-sample_amd/csrc/amt_p_rho_kernel.h, what amt_p_rho.hip compiles for
the device -- run on the host: tests/p_rho_host_check.cpp includes the header behind stand-ins for the thread indices, runs a
launch as nested loops and compares every array of the call, whole and as bytes, with a plain loop nest written from the
contract; built with the address and undefined-behaviour sanitizers.  No GPU, no HIP call; the program is run directly.

The cases are the long-row list of tests/prho_long_rows.py at the gridDim.x the launcher chooses, and the same list at
gridDim.x = 1, 2 and 3, where every wave takes many units -- which the device cannot be asked for.

Mutants: the same program against copies of the header with ONE textual replacement each must NOT come out equal on the list at
the launcher's own gridDim.x.  That is what says the shapes the device sees are the discriminating ones: a mutant that
survives means a shape is missing from the list."""
import os
import subprocess
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import pytest

import prho_long_rows as LR

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "wrf-model-cuda-sample_amd" / "csrc"
HEADER = CSRC / "amt_p_rho_kernel.h"
PROGRAM = ROOT / "tests" / "p_rho_host_check.cpp"
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

# (name, old, new): each old occurs exactly once in the header
MUTANTS = [
    ("the carry without ++j", "if (sg >= segs) { sg -= segs; ++j; }", "if (sg >= segs) { sg -= segs; }"),
    ("cur = at3: the walk's advance forgotten", "cur = at3 + (long)nlev * job.idim;", "cur = at3;"),
    ("cnt always kPer", "const int cnt = rest < 0 ? 0 : rest < kPer ? rest : kPer;", "const int cnt = kPer;"),
    ("at2 without + i0", "at2 = (long)j * job.idim + i0;", "at2 = (long)j * job.idim;"),
    ("wide without cnt == kPer", "const bool wide = phase && cnt == kPer && (((long)ph0", "const bool wide = phase && (((long)ph0"),
    ("wide without the at3 term", "const bool wide = phase && cnt == kPer && (((long)ph0 + at3 * (long)sizeof(T)) & 15) == 0;",
     "const bool wide = phase && cnt == kPer;"),
    ("ds = waves % nj", "ds = waves - dj * segs;", "ds = waves % nj;"),
    ("nlev always AMT_P_RHO_GROUP", "const int nlev = MODE == 1 && left > AMT_P_RHO_GROUP ? AMT_P_RHO_GROUP : left;",
     "const int nlev = AMT_P_RHO_GROUP;"),
    ("phk = vph1 removed", "        phk = vph1;\n", ""),
    ("left from nk - 1", "const int left = job.nk - k0;", "const int left = job.nk - 1 - k0;"),
]


def _compiler():
    """ROCm's clang++ (ext_vector_type rules out g++), found the way csrc/Makefile finds hipcc: $HIPCC, else /opt/rocm/bin/hipcc;
    clang++ is the llvm/bin next to that bin.  A missing compiler fails the test."""
    hipcc = Path(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    assert hipcc.exists(), f"{hipcc}: the product's compiler is missing"
    for rocm in (hipcc.parent.parent, hipcc.resolve().parent.parent):
        for sub in ("llvm/bin/clang++", "lib/llvm/bin/clang++"):
            if (rocm / sub).exists():
                return rocm / sub
    raise AssertionError(f"no clang++ next to {hipcc}")


def _workers():
    return max(1, min(8, len(os.sched_getaffinity(0))))


def _build(clang, include, exe, sanitize="address,undefined"):
    flags = [f for f in FLAGS if not f.startswith("-fsanitize=")] + [f"-fsanitize={sanitize}"]
    r = subprocess.run([str(clang), *flags, "-I", str(include), str(PROGRAM), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _line(case, grid, array_phases=0):
    idim, lead = LR.row_geometry(case)
    return (f"{LR.dtype_name(case.dtype)} {case.ni} {case.nk} {case.nj} {case.members} {case.mode} {case.step} {grid} {lead} "
            f"{array_phases} {idim}")


def _cost(line):
    f = line.split()
    return int(f[1]) * int(f[2]) * int(f[3]) * int(f[4])


def _launcher_lines():
    """The list at the launcher's gridDim.x, cheap cases first (a mutant is killed by the first case that can)."""
    lines = [_line(c, LR.launcher_blocks(c)) for dtype in LR.DTYPES for c in LR.all_cases(dtype)]
    return sorted(lines, key=_cost)


def _forced_lines():
    """gridDim.x = 1, 2, 3: every wave strides over many units; and the member cases with the 13 arrays on different phases."""
    lines = [_line(c, grid) for dtype in LR.DTYPES for c in LR.all_cases(dtype) for grid in (1, 2, 3)]
    lines += [_line(c, grid, 1) for dtype in LR.DTYPES for c in LR.member_cases(dtype) for grid in (LR.launcher_blocks(c), 1)]
    return lines


def _run(exe, path, stop=False):
    return subprocess.run([str(exe)] + (["-x"] if stop else []) + [str(path)], capture_output=True, text=True)


@pytest.fixture(scope="module")
def clang():
    return _compiler()


def test_the_kernel_text_equals_the_contract_on_the_host(clang, tmp_path):
    """Every case of the list at the launcher's gridDim.x and at 1, 2 and 3: 0 differences, no sanitizer report."""
    t0 = time.perf_counter()
    exe = _build(clang, CSRC, tmp_path / "p_rho_host_check")
    lines = _launcher_lines() + _forced_lines()
    assert any(l.split()[7] == "1024" for l in lines) and {"1", "2", "3"} <= {l.split()[7] for l in lines}
    lines.sort(key=_cost, reverse=True)                            # dealt out by cost: the parts take about the same time
    n = _workers()
    parts = [lines[k::n] for k in range(n)]
    for k, part in enumerate(parts):
        (tmp_path / f"cases{k}.txt").write_text("\n".join(part) + "\n")
    with ThreadPoolExecutor(n) as pool:
        results = list(pool.map(lambda k: _run(exe, tmp_path / f"cases{k}.txt"), range(n)))
    for part, r in zip(parts, results):
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"p_rho host check: {len(part)} cases, 0 failures" in r.stdout, r.stdout
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    print(f"  {len(lines)} cases in {n} processes, build included: {time.perf_counter() - t0:.1f} s")


def test_every_mutant_of_the_kernel_text_is_killed_by_the_shapes_the_device_sees(clang, tmp_path):
    t0 = time.perf_counter()
    text = HEADER.read_text()
    for name, old, new in MUTANTS:
        assert text.count(old) == 1, f"{name}: {old!r} occurs {text.count(old)} times in {HEADER.name}"
    cases = tmp_path / "cases.txt"
    lines = _launcher_lines()
    cases.write_text("\n".join(lines) + "\n")

    def one(k):
        name, old, new = MUTANTS[k]
        d = tmp_path / f"mutant{k}"
        d.mkdir()
        (d / HEADER.name).write_text(text.replace(old, new))
        exe = _build(clang, d, d / "p_rho_host_check")
        return _run(exe, cases, stop=True)

    with ThreadPoolExecutor(_workers()) as pool:
        results = list(pool.map(one, range(len(MUTANTS))))
    survivors = []
    for (name, _old, _new), r in zip(MUTANTS, results):
        named = [l for l in r.stdout.splitlines() if l.startswith("case ")]
        assert r.returncode != 2 and named, (name, r.stdout[-400:], r.stderr[-400:])
        if r.returncode == 0:
            survivors.append(name)
            continue
        how = "sanitizer report" if ("runtime error" in r.stderr or "AddressSanitizer" in r.stderr) else "byte difference"
        print(f"  {name}: killed by {named[-1]} ({how})")
    assert not survivors, f"mutants the list does not kill (a shape is missing from tests/prho_long_rows.py): {survivors}"
    print(f"  {len(MUTANTS)} mutants against {len(lines)} cases: {time.perf_counter() - t0:.1f} s")
