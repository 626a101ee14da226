"""The momentum-update kernel's own text -- wrf-model-cuda-sample_amd/csrc/amt_uv_kernel.h, what amt_uv.hip compiles for the
device -- run on the host: tests/uv_host_check.cpp includes the header behind stand-ins for the thread indices, runs a launch
as nested loops and compares every array of the call, whole and as bytes, with a plain loop nest written from the contract;
built with the address and undefined-behaviour sanitizers.  No GPU, no HIP call; the program is run directly.

The cases are the shapes tests/test_gpu_43_advance_uv.py gives the device -- short rows and tails, level groups, long rows,
many units, members, array phases -- at the gridDim.x the launcher chooses, and at gridDim.x = 1, 2 and 3, where every wave
takes many units, which the device cannot be asked for.  Runs end their memory row (idim = row_phase + 1 + ni), so the last
cell read is the allocation's last element.

Mutants: the same program against copies of the header with ONE textual replacement each must NOT come out equal on the
same list."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "wrf-model-cuda-sample_amd" / "csrc"
HEADER = CSRC / "amt_uv_kernel.h"
PROGRAM = ROOT / "tests" / "uv_host_check.cpp"
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
GROUP = 8

# (name, old, new): each old occurs exactly once in the header
MUTANTS = [
    ("the carry without ++j", "if (sg >= segs) { sg -= segs; ++j; }", "if (sg >= segs) { sg -= segs; }"),
    ("cnt always kPer", "const int cnt = rest < 0 ? 0 : rest < kPer ? rest : kPer;", "const int cnt = kPer;"),
    ("wide without cnt == kPer", "const bool wide = phase && cnt == kPer;", "const bool wide = phase;"),
    ("phase without the start of the run", "const bool phase = ph0 == 0 && same(tend)", "const bool phase = same(tend)"),
    ("nlev always AMT_UV_GROUP", "const int nlev = left > AMT_UV_GROUP ? AMT_UV_GROUP : left;", "const int nlev = AMT_UV_GROUP;"),
    ("dphk not carried", "            dphk[i] = dph1;\n", ""),
    ("dpn not carried", "if (NH) { dpnk = dpn1; sa = sb;", "if (NH) { sa = sb;"),
    ("the element in front of the chunk unguarded", "nbr[0] = cnt > 0 ? before[at] : T(0);", "nbr[0] = before[at];"),
    ("the v part's rows from the u part's", "const long row = (long)pt->j0 + j;", "const long row = (long)jp->part[0].j0 + j + PART;"),
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


def _build(clang, include, exe):
    r = subprocess.run([str(clang), *FLAGS, "-I", str(include), "-I", str(CSRC), str(PROGRAM), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _launcher_blocks(dtype, ni, nj):
    seg = 64 * (16 // (8 if dtype == "f64" else 4))
    return min(1024, (nj * ((ni + seg - 1) // seg) + 3) // 4)


def _shapes(dtype):
    """(ni, nk, nj, members, nh, row_phase, array_phases, shrink)"""
    per = 16 // (8 if dtype == "f64" else 4)
    out = []
    for nh in (0, 1):
        for nk in ((1, 2) if not nh else ()) + (3, 4, GROUP, GROUP + 1, 2 * GROUP - 1):
            for ni in (1, 2, 3, 4, 5, 7, 8, 9):
                nj = 1 + (ni + nk) % 3
                out.append((ni, nk, nj, 1, nh, (ni + nk) % per, 0, 1 if ni > 1 and nj > 1 and (ni + nk) % 2 else 0))
        for phases in range(1, per + 1):                           # every phase of the arrays against one another; 16-element rows
            out.append((16 - per, 4, 3, 1, nh, per - 1, phases % per, 0))
        out.append((2 * per + 2, 5, 2, 3, nh, per - 1, 0, 1))      # members, strides off 16 bytes
        out.append((2 * 64 * per + 3, 3, 2, 1, nh, per - 1, 0, 0))  # three wave segments, a short tail; the run starts on a boundary
        out.append((2 * 64 * per + 3, 3, 2, 1, nh, 0, 1, 1))
        out.append((3, 3, 4100, 1, nh, 0, 0, 1))                   # more units than the launch has waves
    return out


def _lines(forced):
    lines = []
    for dtype in ("f64", "f32"):
        for ni, nk, nj, members, nh, lead, phases, shrink in _shapes(dtype):
            idim = lead + 1 + ni                                   # the run ends its memory row
            grids = (1, 2, 3) if forced else (_launcher_blocks(dtype, ni, nj),)
            for grid in grids:
                if forced and nj > 100 and grid > 1:
                    continue
                lines.append(f"{dtype} {ni} {nk} {nj} {members} {nh} {grid} {lead} {phases} {idim} {shrink}")
    return lines


def _cost(line):
    f = line.split()
    return int(f[1]) * int(f[2]) * int(f[3]) * int(f[4])


def _run(exe, path, stop=False):
    return subprocess.run([str(exe)] + (["-x"] if stop else []) + [str(path)], capture_output=True, text=True)


@pytest.fixture(scope="module")
def clang():
    return _compiler()


def test_the_kernel_text_equals_the_contract_on_the_host(clang, tmp_path):
    """Every case at the launcher's gridDim.x and at 1, 2 and 3: 0 differences, no sanitizer report."""
    exe = _build(clang, CSRC, tmp_path / "uv_host_check")
    lines = _lines(False) + _lines(True)
    assert any(l.split()[6] == "1024" for l in lines) and {"1", "2", "3"} <= {l.split()[6] for l in lines}
    lines.sort(key=_cost, reverse=True)                            # dealt out by cost: the parts take about the same time
    n = _workers()
    parts = [lines[k::n] for k in range(n)]
    for k, part in enumerate(parts):
        (tmp_path / f"cases{k}.txt").write_text("\n".join(part) + "\n")
    with ThreadPoolExecutor(n) as pool:
        results = list(pool.map(lambda k: _run(exe, tmp_path / f"cases{k}.txt"), range(n)))
    for part, r in zip(parts, results):
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"uv host check: {len(part)} cases, 0 failures" in r.stdout, r.stdout
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_every_mutant_of_the_kernel_text_is_killed(clang, tmp_path):
    text = HEADER.read_text()
    for name, old, new in MUTANTS:
        assert text.count(old) == 1, f"{name}: {old!r} occurs {text.count(old)} times in {HEADER.name}"
    cases = tmp_path / "cases.txt"
    lines = sorted(_lines(False) + _lines(True), key=_cost)        # gridDim.x = 1, 2, 3: the unit loop's carries
    cases.write_text("\n".join(lines) + "\n")

    def one(k):
        name, old, new = MUTANTS[k]
        d = tmp_path / f"mutant{k}"
        d.mkdir()
        (d / HEADER.name).write_text(text.replace(old, new))
        exe = _build(clang, d, d / "uv_host_check")
        return _run(exe, cases, stop=True)

    with ThreadPoolExecutor(_workers()) as pool:
        results = list(pool.map(one, range(len(MUTANTS))))
    survivors = []
    for (name, _old, _new), r in zip(MUTANTS, results):
        named = [l for l in r.stdout.splitlines() if l.startswith("case ")]
        assert r.returncode != 2 and named, (name, r.stdout[-400:], r.stderr[-400:])
        if r.returncode == 0:
            survivors.append(name)
    assert not survivors, f"mutants the list does not kill: {survivors}"
