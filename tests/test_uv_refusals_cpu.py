"""What amt_advance_uv_device_f32/_f64 (include/amt_advance_mu_t.h section 17) answer on the paths that return before the first
device call: one table of (arguments, status, exact text of amt_last_error).  Rows with two defects at once hold the ORDER of
the checks; rows that return AMT_OK hold what the pass counts as empty; every row leaves every array as it was, byte for byte.
A row marked ACCEPTED passes every check: without a device the call then stops at the missing device (status 1 or 4); with
one it would be launched on host memory, so such a row runs only where amt_device_count() is 0.  No device is needed."""
import ctypes

import numpy as np
import pytest

import uv_ref as R

OK, PRECONDITION, INVALID = 0, 2, 3
ACCEPTED = (1, 4)
F32, F64 = np.float32, np.float64
SCALARS = (1.0e-3, 1.25e-3, 2.0, 1.5, -0.75, 0.25, 0.01)
OVERLAP = "an output array overlaps another array of the call"
EXTENTS = "empty memory extents"


def _patch(pkg):
    return pkg.synth.domain_bounds(5, 3, 4)                       # memory 0:6, 1:4, 0:5; tile 1:6, 1:4, 1:5; ide 6, jde 5, kde 4


def _arrays(b, dtype, members):
    shape = {3: (members, b.jdim, b.kdim, b.idim), 2: (members, b.jdim, b.idim), 1: (b.kdim,)}
    rng = np.random.default_rng(5)
    return {n: rng.uniform(0.5, 1.5, shape[R.RANK[n]]).astype(dtype) for n in R.NAMES}


def _rows():
    rows = []
    add = lambda what, status, text, **kw: rows.append((what, kw, status, text))
    for n in R.NAMES:
        add(f"null {n}", INVALID, "null array pointer", null=(n,))
    add("members 0", INVALID, "members = 0: an ensemble has at least one member", members=0)
    add("null array, members 0", INVALID, "null array pointer", null=("rdnw",), members=0)
    add("members 0, no extents", INVALID, "members = 0: an ensemble has at least one member", members=0, bounds=lambda b: b.replace(ime=b.ims - 1))
    add("no extents", PRECONDITION, EXTENTS, bounds=lambda b: b.replace(jme=b.jms - 1))
    add("no extents, overlap", PRECONDITION, EXTENTS, bounds=lambda b: b.replace(ime=b.ims - 1), swap=lambda a: dict(p=a["u"]))
    add("p is u", INVALID, OVERLAP, swap=lambda a: dict(p=a["u"]))
    add("v one element into u", INVALID, OVERLAP, swap=lambda a: dict(v=a["u"].reshape(-1)[1:]))
    add("rdnw is the end of v", INVALID, OVERLAP, swap=lambda a: dict(rdnw=a["v"].reshape(-1)[-a["rdnw"].size:]))
    add("inputs alias one another", ACCEPTED, None, swap=lambda a: dict(pb=a["p"], al=a["alt"], muv=a["muu"], fnp=a["fnm"], cqv=a["cqu"]))
    add("overlap, kts 2", INVALID, OVERLAP, swap=lambda a: dict(p=a["u"]), bounds=lambda b: b.replace(kts=2))
    add("kts 2", PRECONDITION, "kts = 2, the library needs kts == 1", bounds=lambda b: b.replace(kts=2))
    add("kte is not kde", PRECONDITION, "kte = 3 is not kde = 4", bounds=lambda b: b.replace(kte=3))
    add("kme < kte", PRECONDITION, "levels kts:kte = 1:4 are not inside memory kms:kme = 1:3", bounds=lambda b: b.replace(kme=3))
    add("ite > ime", PRECONDITION, "the tile 1:7, 1:5 is not inside memory 0:6, 0:5", bounds=lambda b: b.replace(ite=7))
    add("jts < jms", PRECONDITION, "the tile 1:6, -1:5 is not inside memory 0:6, 0:5", bounds=lambda b: b.replace(jts=-1))
    # the pass's own refusals, behind the box
    add("non-hydrostatic, kde 3", PRECONDITION, "kde = 3: the non-hydrostatic form needs three levels of p (kde >= 4)", nh=1,
        bounds=lambda b: b.replace(kde=3, kte=3))
    add("hydrostatic, kde 3", ACCEPTED, None, nh=0, bounds=lambda b: b.replace(kde=3, kte=3))
    add("tile outside memory, non-hydrostatic kde 3", PRECONDITION, "the tile 1:7, 1:3 is not inside memory 0:6, 0:5", nh=1,
        bounds=lambda b: b.replace(kde=3, kte=3, ite=7, jte=3))
    add("column i_start-1 outside memory", PRECONDITION, "the cells read, 0:6, 0:5, are not inside memory 1:6, 0:5", bounds=lambda b: b.replace(ims=1))
    add("row j_start-1 outside memory", PRECONDITION, "the cells read, 0:6, 0:5, are not inside memory 0:6, 1:5", bounds=lambda b: b.replace(jms=1))
    add("kde 3 and column outside memory", PRECONDITION, "kde = 3: the non-hydrostatic form needs three levels of p (kde >= 4)", nh=1,
        bounds=lambda b: b.replace(kde=3, kte=3, ims=1))
    add("specified: i_start is ids+1, its-1 need not lie in memory", ACCEPTED, None, flags=(0, 1, 0), bounds=lambda b: b.replace(ims=1, jms=1))
    add("specified and periodic_x: columns unclipped", PRECONDITION, "the cells read, 0:6, 1:4, are not inside memory 1:6, 1:5", flags=(1, 1, 0),
        bounds=lambda b: b.replace(ims=1, jms=1))
    # what counts as empty: AMT_OK, the text of the last error stays
    add("ite < its", OK, None, bounds=lambda b: b.replace(ite=0))
    add("jte < jts outside memory", OK, None, bounds=lambda b: b.replace(jts=9, jte=8))
    add("kte == kts", OK, None, bounds=lambda b: b.replace(kde=1, kte=1))
    add("kte == kts, non-hydrostatic", OK, None, nh=1, bounds=lambda b: b.replace(kde=1, kte=1))
    add("both parts without a cell", OK, None, flags=(0, 1, 0), bounds=lambda b: b.replace(ids=1, ide=2, its=1, ite=2, jds=1, jde=2, jts=1, jte=2))
    add("both parts without a cell, non-hydrostatic kde 3", OK, None, flags=(0, 1, 0), nh=1,
        bounds=lambda b: b.replace(ids=1, ide=2, its=1, ite=2, jds=1, jde=2, jts=1, jte=2, kde=3, kte=3))
    add("every check passes", ACCEPTED, None)
    add("every check passes, non-hydrostatic", ACCEPTED, None, nh=1)
    return rows


ROWS = _rows()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("k", range(len(ROWS)), ids=[r[0].replace(" ", "_") for r in ROWS])
def test_the_call_answers_with_its_status_and_its_text_and_writes_nothing(pkg, k, dtype):
    L = pkg.load_library()
    what, kw, status, text = ROWS[k]
    kw = dict(kw)
    if status == ACCEPTED and L.amt_device_count() != 0:
        return                                                    # would be launched on host memory
    members = kw.pop("members", 1)
    b = _patch(pkg)
    arrays = _arrays(b, dtype, max(members, 1))
    b = kw.pop("bounds", lambda x: x)(b)
    arrays.update(kw.pop("swap", lambda a: {})(arrays))
    for n in kw.pop("null", ()):
        arrays[n] = None
    before = {n: a.tobytes() for n, a in arrays.items() if a is not None}
    who = f"amt_advance_uv_device_{'f64' if dtype is F64 else 'f32'}"
    fn = getattr(L, who)
    assert L.amt_domain_sync(None) == INVALID                     # a text of another call, for the rows that leave it
    earlier = L.amt_last_error()
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    got = fn(None, members, kw.pop("nh", 0), *[ptr(arrays[n]) for n in R.NAMES], *SCALARS, *kw.pop("flags", (0, 0, 0)), *b.as_tuple())
    assert not kw
    if status == ACCEPTED:
        assert got in ACCEPTED, (what, L.amt_last_error())
    else:
        assert got == status, (what, L.amt_last_error())
        assert L.amt_last_error() == (earlier if status == OK else f"{who}: {text}".encode()), what
    for n, image in before.items():
        assert arrays[n].tobytes() == image, (what, n)


# ---------------------------------------------------------------------------------------------------------------------
# the handle exports on a zeroed handle (every setting off, all bounds zero, no field): what returns before the first device call
# ---------------------------------------------------------------------------------------------------------------------
_blank = (ctypes.c_char * 8192)()
BLANK = ctypes.cast(_blank, ctypes.c_void_p)
_room = (ctypes.c_double * 128)()
ROOM = [ctypes.c_void_p(ctypes.addressof(_room) + 64 * k) for k in range(9)]
NONE9 = [None] * 9
S4 = (0.01, 1.5, -0.75, 0.25)
NEEDS_P_RHO = "the pressure diagnosis, whose al, p, ph, alt the update reads, is off (amt_*_set_p_rho)"
ALL = "give all nine arrays or none (the library then allocates them)"

# (call behind the prefix, arguments, status, text; None: the text is "null domain" / "null ensemble")
HANDLE = [
    ("set_uv", (None, 1, 0, *S4, *NONE9), INVALID, None),
    ("set_uv", (None, 0, 0, *S4, *NONE9), INVALID, None),
    ("uv", (None,), INVALID, None),
    ("uv", (BLANK,), PRECONDITION, "{p}_uv: the momentum update is off (amt_*_set_uv)"),
    # set_uv: all or none, then the pressure diagnosis
    ("set_uv", (BLANK, 1, 1, *S4, ROOM[0], *NONE9[1:]), INVALID, "{p}_set_uv: " + ALL),
    ("set_uv", (BLANK, 1, 0, *S4, *ROOM[:5], None, *ROOM[6:]), INVALID, "{p}_set_uv: " + ALL),
    ("set_uv", (BLANK, 1, 1, *S4, *NONE9), PRECONDITION, "{p}_set_uv: " + NEEDS_P_RHO),
    ("set_uv", (BLANK, 1, 0, *S4, *ROOM), PRECONDITION, "{p}_set_uv: " + NEEDS_P_RHO),
]


@pytest.mark.parametrize("prefix,who", [("amt_domain", "null domain"), ("amt_ensemble", "null ensemble")])
@pytest.mark.parametrize("k", range(len(HANDLE)), ids=[f"{r[0]}-{k}" for k, r in enumerate(HANDLE)])
def test_a_handle_call_refuses_with_its_status_and_its_text_and_changes_nothing(pkg, k, prefix, who):
    L = pkg.load_library()
    call, args, status, text = HANDLE[k]
    assert getattr(L, f"{prefix}_{call}")(*args) == status, (call, L.amt_last_error())
    assert L.amt_last_error().decode() == (who if text is None else text.format(p=prefix)), call
    assert all(getattr(L, f"{prefix}_uv_ptr")(BLANK, which) is None for which in range(-1, 10))
    assert bytes(_blank) == bytes(8192)
