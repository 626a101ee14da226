"""The (chunk, k, j) decomposition of a work item in the streaming kernels -- csrc/amt_chunk_index.h, called by amt_stage.hip and
amt_sumflux.hip -- on the host: the 64-bit branch, which on the device needs a job of more than 2^31 - 1 work items (tens of
GB), against 128-bit arithmetic in a stand-alone program (tests/chunk_index_check.cpp) and against vectors computed here with
Python's integers.  Built with the undefined-behaviour and address sanitizers: no GPU, no HIP call."""
import random
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
EDGES = ((1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 40) - 1, 1 << 40)


def _vectors():
    """"kPer ni nk nj e j k i0 cnt" lines from the definition e = (j * nk + k) * chunks + c, in Python's integers."""
    rng = random.Random(20261020)
    lines = []
    jobs = [(2, 7, 300, (1 << 31) - 1), (4, 602, 34, 1 << 24), (4, 1, 1, 1 << 33), (2, 3, 1 << 9, 1 << 30), (4, 13, 5, 9), (2, 70, 9, 6),
            (4, 4099, 300, 1 << 20)]
    for per, ni, nk, nj in jobs:
        chunks = -(-ni // per)
        total = nk * nj * chunks
        es = [e for e in EDGES if e < total] + [0, total - 1] + [rng.randrange(total) for _ in range(200)]
        for e in es:
            r, c = divmod(e, chunks)
            j, k = divmod(r, nk)
            i0 = c * per
            lines.append(f"{per} {ni} {nk} {nj} {e} {j} {k} {i0} {min(per, ni - i0)}")
    assert any(int(l.split()[4]) == 1 << 40 for l in lines) and any(int(l.split()[4]) == (1 << 32) - 1 for l in lines)
    return lines


def test_narrow_and_wide_paths_agree_and_the_wide_path_is_exact_past_2_to_the_32(tmp_path):
    exe = tmp_path / "chunk_index_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined",
                        "-I", str(ROOT / "wrf-model-cuda-sample_amd" / "csrc"), str(ROOT / "tests" / "chunk_index_check.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    vectors = _vectors()
    (tmp_path / "vectors.txt").write_text("\n".join(vectors) + "\n")
    r = subprocess.run([str(exe), str(tmp_path / "vectors.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f" {len(vectors)} vectors, 0 failures" in r.stdout, r.stdout
    counts = [int(x) for x in r.stdout.replace(",", " ").split() if x.isdigit()]
    checks, narrow, wide, boundaries = counts[:4]
    assert narrow > 10000 and wide > 10000 and boundaries >= 100, r.stdout


def test_chunk_load_and_store_move_exactly_cnt_elements_on_the_host(tmp_path):
    """csrc/amt_chunk_io.h, the load and store the streaming kernels share, in a stand-alone program (tests/chunk_io_check.cpp):
    both element types, every cnt in 0..kPer and every phase of the start, wide only for a whole chunk on a 16-byte boundary,
    in guarded buffers and in allocations that end with the chunk.  ROCm's clang++: ext_vector_type rules out g++."""
    from test_prho_host import _compiler
    exe = tmp_path / "chunk_io_check"
    r = subprocess.run([str(_compiler()), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(ROOT / "wrf-model-cuda-sample_amd" / "csrc"),
                        str(ROOT / "tests" / "chunk_io_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    # float: 5 counts x 4 phases, double: 3 x 2, each in two buffers, and the whole aligned chunk once more as a wide access
    assert "chunk io: 56 loads, 56 stores, 4 of the cases wide, 0 failures" in r.stdout, r.stdout
