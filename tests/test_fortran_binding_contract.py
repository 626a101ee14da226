"""The Fortran binding module (wrf-model-cuda-sample_amd/fortran/amt_c_binding.f90) against the C header it restates.  A
BIND(C) interface is a second, hand-written copy of a prototype and nothing ties the two together: a missing VALUE, two pointer
arguments swapped, a c_float where C takes double or two record members in the wrong order all compile and link.  Here the two
files are compared as source -- signatures, records, constants -- a ledger keeps every interface called by a Fortran program
and every header symbol either bound or excused, and amt_halo_plan is called from Fortran (host arithmetic, no device).
Nothing in this file needs a GPU."""
import ctypes
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
FDIR = ROOT / "wrf-model-cuda-sample_amd" / "fortran"
MODULE = FDIR / "amt_c_binding.f90"
HEADERS = [ROOT / "include" / "amt_advance_mu_t.h", ROOT / "include" / "amt_synth.h"]
HOST_DIR = ROOT / "tests" / "fortran"
HOST_SRC = HOST_DIR / "amt_binding_host.f90"
# the Fortran programs of the repository: the three drivers and the host of the binding tests
PROGRAMS = [FDIR / "advance_mu_t_driver.f90", FDIR / "advance_mu_t_slab_driver.f90", FDIR / "advance_mu_t_grid_driver.f90", HOST_SRC]


# ---------------------------------------------------------------------------------------------------------------------
# the C side
# ---------------------------------------------------------------------------------------------------------------------
def _c_text():
    text = "\n".join(p.read_text() for p in HEADERS)
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"\\\n", " ", text)
    return "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))


def _c_type(decl):
    """'const float *ww' -> ('float', 1, 'ww'); 'void *const *fields' -> ('void', 2, 'fields'); a result type has no name."""
    stars = decl.count("*")
    words = [w for w in re.sub(r"[*]", " ", decl).split() if w != "const"]
    return words, stars


def c_prototypes():
    """name -> (result (base, stars), [(base, stars, parameter name)])"""
    out = {}
    for m in re.finditer(r"(?:^|[;}])\s*((?:const\s+)?\w+(?:\s+\w+)?[\s*]+)(amt_\w+)\s*\(([^)]*)\)\s*;", _c_text(), re.S | re.M):
        rwords, rstars = _c_type(m.group(1))
        params = []
        body = " ".join(m.group(3).split())
        if body != "void":
            for p in body.split(","):
                words, stars = _c_type(p)
                assert len(words) >= 2, (m.group(2), p)
                params.append((" ".join(words[:-1]), stars, words[-1]))
        assert m.group(2) not in out, m.group(2)
        out[m.group(2)] = ((" ".join(rwords), rstars), params)
    return out


def c_records():
    """record name -> member names in order"""
    out = {}
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", _c_text(), re.S):
        assert m.group(1) == m.group(3)
        members = []
        for stmt in m.group(2).split(";"):
            if stmt.strip():
                members += [re.findall(r"\w+", n)[-1] for n in stmt.split(",")]
        out[m.group(1)] = members
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the Fortran side
# ---------------------------------------------------------------------------------------------------------------------
def _f_lines(path):
    """Source lines without comments, continuation lines joined, lower case kept as written."""
    lines, cur = [], ""
    for raw in path.read_text().splitlines():
        code = re.sub(r"!.*$", "", raw).rstrip()           # no string of these sources holds a '!'
        if not code.strip():
            continue
        code = code.strip()
        if cur:
            code = code[1:].lstrip() if code.startswith("&") else code
        if code.endswith("&"):
            cur += code[:-1] + " "
            continue
        lines.append(cur + code)
        cur = ""
    assert not cur
    return lines


def _split_top(s):
    """Split at commas that are not inside parentheses."""
    parts, depth, cur = [], 0, ""
    for ch in s:
        depth += ch == "("
        depth -= ch == ")"
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    parts.append(cur.strip())
    return parts


def f_interfaces():
    """C symbol -> dict(name, args [dummy names], result name, decl {name: (typespec, by_value)})"""
    out, cur = {}, None
    for line in _f_lines(MODULE):
        m = re.match(r"function\s+(\w+)\s*\(([^)]*)\)\s*bind\(C,\s*name=\"(\w+)\"\)\s*result\((\w+)\)\s*$", line, re.I)
        if m:
            assert cur is None, line
            args = [a.strip().lower() for a in m.group(2).split(",") if a.strip()]
            cur = dict(name=m.group(1), args=args, result=m.group(4).lower(), decl={})
            assert m.group(1) == m.group(3), "the Fortran name of an interface is its C symbol"
            assert m.group(3) not in out, m.group(3)
            out[m.group(3)] = cur
            continue
        if cur is None:
            continue
        if re.match(r"end\s+function", line, re.I):
            cur = None
            continue
        if re.match(r"import\b", line, re.I):
            continue
        left, right = line.split("::")
        spec = [p.replace(" ", "").lower() for p in _split_top(left)]
        for n in _split_top(right):
            name = re.match(r"\w+", n).group(0).lower()
            assert name not in cur["decl"], (cur["name"], name)
            cur["decl"][name] = (spec[0], "value" in spec[1:])
    assert cur is None
    return out


def f_records():
    out, cur = {}, None
    for line in _f_lines(MODULE):
        m = re.match(r"type,\s*bind\(C\)\s*::\s*(\w+)", line, re.I)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and re.match(r"end\s+type", line, re.I):
            cur = None
        elif cur is not None:
            cur += [re.match(r"\w+", n.strip()).group(0) for n in line.split("::")[1].split(",")]
    return out


def f_parameters():
    """Every AMT_* named constant of the module -> its kind."""
    out = {}
    for line in _f_lines(MODULE):
        m = re.match(r"integer\((\w+)\),\s*parameter\s*::(.*)$", line, re.I)
        if m:
            for name in re.findall(r"\b(AMT_[A-Z0-9_]+)\s*=", m.group(2)):
                assert name not in out, name
                out[name] = m.group(1)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# signatures
# ---------------------------------------------------------------------------------------------------------------------
SCALAR = {"int": "integer(c_int)", "long": "integer(c_long)", "float": "real(c_float)", "double": "real(c_double)",
          "size_t": "integer(c_size_t)", "int64_t": "integer(c_int64_t)", "uint64_t": "integer(c_int64_t)"}
# what a by-reference dummy of a `T *` parameter may be; void * by reference is raw bytes (a communicator id)
POINTEE = dict(SCALAR, char="character(kind=c_char)", void="character(kind=c_char)")
# (C parameter name, Fortran dummy name) pairs that may differ: the opaque handle, and one host pointer
ALLOWED_NAME_PAIRS = {("d", "handle"), ("e", "handle"), ("domain", "handle"), ("out", "handle"), ("out", "slab"), ("out", "grid"),
                      ("a", "handle_a"), ("b", "handle_b"), ("host_ptr", "ptr")}


def _dummy_matches(ctype, stars, spec, by_value, records):
    if stars == 0:
        return by_value and SCALAR.get(ctype) == spec
    if stars == 1:
        if spec == "type(c_ptr)":
            return by_value
        want = f"type({ctype})" if ctype in records else POINTEE.get(ctype)
        return not by_value and want == spec
    return stars == 2 and spec == "type(c_ptr)" and not by_value


def _signature_problems(protos, ifaces, records):
    bad = []
    for sym, it in ifaces.items():
        if sym not in protos:
            bad.append(f"{sym}: no such C symbol")
            continue
        (rtype, rstars), params = protos[sym]
        if len(params) != len(it["args"]):
            bad.append(f"{sym}: {len(it['args'])} dummies for {len(params)} C parameters")
            continue
        for pos, ((ctype, stars, cname), fname) in enumerate(zip(params, it["args"])):
            if cname.lower() != fname and (cname, fname) not in ALLOWED_NAME_PAIRS:
                bad.append(f"{sym}: argument {pos + 1} is '{fname}', the header has '{cname}'")
            if fname not in it["decl"]:
                bad.append(f"{sym}: dummy '{fname}' is not declared")
                continue
            spec, by_value = it["decl"][fname]
            if not _dummy_matches(ctype, stars, spec, by_value, records):
                bad.append(f"{sym}: '{fname}' is {spec}{', value' if by_value else ''} for C '{ctype} {'*' * stars}{cname}'")
        rspec, rvalue = it["decl"].get(it["result"], ("<undeclared>", False))
        want = "type(c_ptr)" if rstars == 1 else SCALAR.get(rtype) if rstars == 0 else None
        if rvalue or rspec != want:
            bad.append(f"{sym}: result is {rspec} for C '{rtype} {'*' * rstars}'")
        extra = set(it["decl"]) - set(it["args"]) - {it["result"]}
        if extra:
            bad.append(f"{sym}: declares {sorted(extra)} that are not dummies")
    return bad


def test_the_parsers_see_both_files_whole():
    protos, ifaces = c_prototypes(), f_interfaces()
    header = re.sub(r"/\*.*?\*/", "", HEADERS[0].read_text(), flags=re.S)
    assert sorted(protos) == sorted(set(re.findall(r"\b(amt_[a-z0-9_]+)\s*\(", header)))      # what tests/test_abi.py counts
    assert len(ifaces) == len(re.findall(r"bind\(C, name=", MODULE.read_text())) >= 107
    assert protos["amt_domain_wrap"][1][-2] == ("void", 2, "fields") and protos["amt_last_error"] == (("char", 1), [])
    assert ifaces["amt_spec_bdy_update_device_f32"]["decl"]["dts"] == ("real(c_float)", True)


def test_every_interface_matches_its_prototype():
    """The C symbol exists; same argument count; position by position the same name (but for the pairs spelled out above), the
    matching kind and passing mode; the matching result kind."""
    bad = _signature_problems(c_prototypes(), f_interfaces(), c_records())
    assert not bad, "\n".join(bad)


def test_the_names_differ_only_where_allowed_and_exactly_there():
    """Which pairs are in use: a pair nobody needs any more leaves the list."""
    protos, ifaces = c_prototypes(), f_interfaces()
    used = set()
    for sym, it in ifaces.items():
        for (_t, _s, cname), fname in zip(protos[sym][1], it["args"]):
            if cname.lower() != fname:
                used.add((cname, fname))
    assert used == ALLOWED_NAME_PAIRS, used ^ ALLOWED_NAME_PAIRS


# ---------------------------------------------------------------------------------------------------------------------
# records and constants: two tiny programs, one per language
# ---------------------------------------------------------------------------------------------------------------------
RECORDS = ("amt_field_stats", "amt_field_diff", "amt_guard_report", "amt_halo_message")


def _fc():
    for name in ("amdflang", "flang", "gfortran"):
        r = subprocess.run(["sh", "-c", f"command -v {name}"], capture_output=True, text=True)
        if r.returncode == 0:
            return r.stdout.strip()
    return None


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, **kw)
    assert r.returncode == 0, f"{' '.join(map(str, cmd))}\n{r.stdout}\n{r.stderr}"
    return r.stdout


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """(C table, Fortran table): 'sizeof <record> <n>', 'offsetof <record> <member> <n>' and 'const <NAME> <value>' lines.  The C
    program takes its member names from the header, the Fortran one from the module; both print the module's constants."""
    fc = _fc()
    if fc is None:
        pytest.skip("no Fortran compiler")
    tmp = tmp_path_factory.mktemp("binding_tables")
    crec, frec, consts = c_records(), f_records(), f_parameters()
    assert set(RECORDS) <= set(crec) and set(frec) == set(RECORDS)
    c = ['#include <stdio.h>', '#include <stddef.h>', '#include "amt_synth.h"', '#include "amt_advance_mu_t.h"', "int main(void) {"]
    for r in RECORDS:
        c.append(f'  printf("sizeof {r} %ld\\n", (long)sizeof({r}));')
        c += [f'  printf("offsetof {r} {m} %ld\\n", (long)offsetof({r}, {m}));' for m in crec[r]]
    c += [f'  printf("const {n} %lld\\n", (long long)({n}));' for n in sorted(consts)]
    c += ["  return 0;", "}"]
    (tmp / "c_table.c").write_text("\n".join(c) + "\n")
    _run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-o", str(tmp / "c_table"), str(tmp / "c_table.c")])
    f = ["program f_table", "  use iso_c_binding", "  use amt_c_binding", "  implicit none"]
    f += [f"  type({r}), target :: v_{r}" for r in RECORDS]
    for r in RECORDS:
        f.append(f"  print '(a,1x,i0)', 'sizeof {r}', c_sizeof(v_{r})")
        f += [f"  print '(a,1x,i0)', 'offsetof {r} {m}', transfer(c_loc(v_{r}%{m}), 0_c_intptr_t) - transfer(c_loc(v_{r}), 0_c_intptr_t)"
              for m in frec[r]]
    f += [f"  print '(a,1x,i0)', 'const {n}', {n}" for n in sorted(consts)]
    f.append("end program f_table")
    (tmp / "f_table.f90").write_text("\n".join(f) + "\n")
    # the module's amt_check refers to amt_last_error: a stub stands in for the library, nothing of it is needed here
    (tmp / "stub.c").write_text('const char *amt_last_error(void) { return ""; }\n')
    _run(["gcc", "-c", "-o", str(tmp / "stub.o"), str(tmp / "stub.c")])
    _run([fc, "-o", str(tmp / "f_table"), str(MODULE), str(tmp / "f_table.f90"), str(tmp / "stub.o")], cwd=tmp)
    tab = lambda exe: [" ".join(line.split()) for line in _run([str(tmp / exe)]).splitlines() if line.strip()]
    return tab("c_table"), tab("f_table")


def test_records_have_the_same_members_at_the_same_offsets(tables):
    c, f = ([line for line in t if not line.startswith("const ")] for t in tables)
    assert len(c) == sum(len(c_records()[r]) + 1 for r in RECORDS)
    assert f == c, "\n".join(f"{a!r} (Fortran) != {b!r} (C)" for a, b in zip(f, c) if a != b)


def test_every_constant_of_the_module_has_the_headers_value(tables):
    c, f = ([line for line in t if line.startswith("const ")] for t in tables)
    names = {line.split()[1] for line in c}
    for prefix in ("AMT_F_", "AMT_SIDE_", "AMT_SLAB_", "AMT_CYCLIC_", "AMT_REGION_", "AMT_VARIANT_"):
        assert any(n.startswith(prefix) for n in names), prefix
    assert {"AMT_OK", "AMT_ERR_NONFINITE", "AMT_EXCHANGED_FIELDS", "AMT_LAUNCH_BESIDE_OTHERS"} <= names
    assert len([n for n in names if n.startswith("AMT_F_")]) == 26
    assert f == c, "\n".join(f"{a!r} (Fortran) != {b!r} (C)" for a, b in zip(f, c) if a != b)


# ---------------------------------------------------------------------------------------------------------------------
# the ledger
# ---------------------------------------------------------------------------------------------------------------------
# header symbols without an interface, each with its reason; a new header symbol forces a decision
NOT_BOUND = {
    "amt_calib_stream_copy": "calibration of the profiler's byte counters (profiles/): not a host call",
    "amt_calib_stream_rate": "the box's streaming ceilings for bench.py's roofline: not a host call",
    "amt_march_force_shape": "tuning and test hook: forces a wave shape for the whole process",
    "amt_march_last_kernel": "diagnosis: names the kernel the last launch plan chose",
    "amt_march_selectable": "diagnosis: lists the kernels the launcher can choose",
    "amt_march_set_xchunk": "diagnosis: workgroup-to-block mapping, not a tuning default",
    "amt_march_set_beside": "tuning hook: launch plan beside another stream's kernels (environment variables do the same)",
    "amt_march_set_stream_policy": "tuning hook: cache policy of the once-read streams (AMT_MARCH_NT does the same)",
    "amt_slab_pull_mode": "diagnosis of the IPC transport",
    "amt_grid_pull_mode": "diagnosis of the IPC transport",
    "amt_slab_set_skew_us": "test hook: neighbour skew",
    "amt_grid_set_skew_us": "test hook: neighbour skew",
}


def _calls(path):
    text = "\n".join(_f_lines(path)).lower()
    return set(re.findall(r"\b(amt_\w+)\s*\(", text))


def test_every_interface_is_called_by_a_fortran_program():
    called = set().union(*[_calls(p) for p in PROGRAMS])
    uncalled = sorted(set(f_interfaces()) - called)
    assert not uncalled, f"{len(uncalled)} interfaces no Fortran program calls: {uncalled}"


def test_every_header_symbol_is_bound_or_excused():
    protos, ifaces = set(c_prototypes()), set(f_interfaces())
    assert all(reason.strip() for reason in NOT_BOUND.values())
    assert not set(NOT_BOUND) & ifaces, "bound now: take it off the list"
    assert protos - ifaces == set(NOT_BOUND), sorted((protos - ifaces) ^ set(NOT_BOUND))


def test_integration_guide_names_only_bound_symbols_in_its_fortran_sections():
    """Sections 1 and 5-9 of INTEGRATION.md are written for a Fortran host: every header symbol they name has an interface,
    but for the tuning hooks excused above."""
    doc = (ROOT / "INTEGRATION.md").read_text()
    sec = lambda a, b: doc[doc.index(a): doc.index(b)] if b else doc[doc.index(a):]
    text = sec("## 1. Fortran-90", "## 2. C ") + sec("## 5. An ensemble host", None)
    named = set(re.findall(r"\bamt_[a-z0-9_]+", text)) & set(c_prototypes())
    assert len(named) > 60
    assert named - set(f_interfaces()) <= set(NOT_BOUND), sorted(named - set(f_interfaces()) - set(NOT_BOUND))


# ---------------------------------------------------------------------------------------------------------------------
# amt_halo_plan from Fortran
# ---------------------------------------------------------------------------------------------------------------------
DIMS = (37, 5, 11)
CYCLIC_X, CYCLIC_Y, HOST_BUFFERS = 8, 16, 64


@pytest.fixture(scope="module")
def host(pkg):
    """The Fortran host of tests/fortran, built against the library as the drivers are."""
    if _fc() is None:
        pytest.skip("no Fortran compiler")
    _run(["make", "-C", str(HOST_DIR), "all"])
    return {4: HOST_DIR / "amt_binding_host_f32", 8: HOST_DIR / "amt_binding_host_f64"}


def _records(path):
    return [line.split() for line in (path / "records.txt").read_text().splitlines()]


@pytest.mark.parametrize("pi,pj", [(2, 2), (3, 1)])
@pytest.mark.parametrize("flags", [0, CYCLIC_X | CYCLIC_Y | HOST_BUFFERS], ids=["plain", "cyclic"])
@pytest.mark.parametrize("itemsize", [4, 8], ids=["f32", "f64"])
def test_halo_plan_from_fortran_equals_the_python_call(pkg, host, tmp_path, itemsize, flags, pi, pj):
    """Every rank of the decomposition: status, count and side / peer / send_bytes / recv_bytes / on_host of each message as
    Python's call of the same arguments gives them; and the relations tests/test_halo_plan.py holds the planner to."""
    from wrf_model_cuda_sample_amd import lib
    S, P, L = pkg.synth, pkg.patch, pkg.load_library()
    gb = S.domain_bounds(*DIMS)
    _run([str(host[itemsize]), "plan", str(tmp_path), "1", "0", "0", "0", "0", *map(str, gb.as_tuple()), *map(str, DIMS),
          "17", "1e-3", "1.25e-3", "2.0", "0.1", str(pi), str(pj), str(flags)])
    recs = _records(tmp_path)
    assert recs[0] == ["real_bytes", str(itemsize)] and recs[-1] == ["done"]
    assert " ".join(next(r for r in recs if r[0] == "version")[1:]) == L.amt_version().decode()
    assert " ".join(next(r for r in recs if r[0] == "status_string_2")[1:]) == L.amt_status_string(2).decode()
    got = {r: [tuple(map(int, x[2:])) for x in recs if x[0] == "planned" and int(x[1]) == r] for r in range(pi * pj)}
    heads = {int(x[1]): (int(x[2]), int(x[3])) for x in recs if x[0] == "plan"}
    plans = {}
    for r in range(pi * pj):
        ri, rj = r % pi, r // pi
        b = S.patch_bounds(gb, ri, rj, pi, pj)
        out, n = (lib.HaloMessage * 4)(), ctypes.c_int(-1)
        st = L.amt_halo_plan(itemsize, 0, 0, 0, *b.as_tuple(), ri, rj, pi, pj, flags, out, 4, ctypes.byref(n))
        assert st == 0 and heads[r] == (st, n.value)
        plans[r] = [(m.side, m.peer, m.send_bytes, m.recv_bytes, m.on_host, int(bool(m.send or m.recv))) for m in out[:n.value]]
        assert got[r] == plans[r], (r, got[r], plans[r])
    cyc = bool(flags & CYCLIC_X)
    for r, msgs in got.items():
        ri, rj = r % pi, r // pi
        sides = [m[0] for m in msgs]
        want = S.neighbour_sides(ri, rj, pi, pj)
        want |= (S.SIDE_LEFT | S.SIDE_RIGHT) if cyc and pi > 1 else 0
        want |= (S.SIDE_BELOW | S.SIDE_ABOVE) if cyc and pj > 1 else 0
        assert sides == [s for s in P.SIDE_ORDER if s in sides] and sum(sides) == want
        for side, peer, send, recv, on_host, has_ptr in msgs:
            match = [o for o in got[peer] if o[1] == r and o[0] == P.OPPOSITE_SIDE[side]]
            assert len(match) == 1 and match[0][3] == send and match[0][2] == recv and send > 0 and recv > 0
            assert on_host == (1 if flags & HOST_BUFFERS else 0) and has_ptr == 0


def test_halo_plan_sizes_written_out_from_fortran(pkg, host, tmp_path):
    """Patch (1, 0) of 3 x 2, fp64 -- the case tests/test_halo_plan.py writes out: columns 13..24, rows 1..5, 6 memory levels."""
    gb = pkg.synth.domain_bounds(*DIMS)
    _run([str(host[8]), "plan", str(tmp_path), "1", "0", "0", "0", "0", *map(str, gb.as_tuple()), *map(str, DIMS),
          "17", "1e-3", "1.25e-3", "2.0", "0.1", "3", "2", str(HOST_BUFFERS)])
    got = [tuple(map(int, x[2:7])) for x in _records(tmp_path) if x[0] == "planned" and x[1] == "1"]
    assert got == [(2, 4, 8 * 6 * 12, 8 * (3 * 6 + 2) * 12, 1), (4, 0, 8 * (3 * 6 + 2) * 5, 8 * 6 * 5, 1),
                   (8, 2, 8 * 6 * 5, 8 * (3 * 6 + 2) * 5, 1)]
