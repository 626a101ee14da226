"""What the resident handles amt_domain_* / amt_ensemble_* answer on the paths that return before the first HIP call
(include/amt_advance_mu_t.h sections 4 and 8): one table of (call, arguments, status, exact text of amt_last_error -- or
the value a getter returns).  The domain and the ensemble exports share their bodies (csrc/amt_domain.hip); each keeps its own
checks and its own texts, and this table is what holds them.  No device is needed."""
import ctypes

import pytest

OK, PRECONDITION, INVALID = 0, 2, 3
N_FIELDS = 26

FLAGS = (0, 0, 0)
#         ids ide jds jde kde ims ime jms jme kms kme its ite jts jte kts kte
BOUNDS = (1, 17, 1, 17, 9, 0, 17, 0, 17, 1, 9, 1, 17, 1, 17, 1, 9)
EMPTY_I = BOUNDS[:5] + (0, -1) + BOUNDS[7:]
EMPTY_J = BOUNDS[:7] + (5, 4) + BOUNDS[9:]
EMPTY_K = BOUNDS[:9] + (1, 0) + BOUNDS[11:]
ROWS_4096 = BOUNDS[:7] + (0, 4095) + BOUNDS[9:]          # jdim = 4096: 2^20 members are 2^32 rows

_host = (ctypes.c_double * 8)()
HOST = ctypes.cast(_host, ctypes.c_void_p)
# a handle that is not NULL, for the checks in front of the first use of the handle: zeroed memory larger than either struct
_blank = (ctypes.c_char * 8192)()
BLANK = ctypes.cast(_blank, ctypes.c_void_p)


def _out():
    return ctypes.pointer(ctypes.c_void_p(0xdead))


def _fields(null_at=None):
    return (ctypes.c_void_p * N_FIELDS)(*[None if f == null_at else 0x1000 * (f + 1) for f in range(N_FIELDS)])


# (call, arguments, status, text)
NULL_HANDLE = [
    ("amt_domain_destroy", (None,), OK, None),
    ("amt_domain_set_scalars", (None, 1.0, 1.0, 1.0, 0.1), INVALID, "null domain"),
    ("amt_domain_set_variant", (None, 0), INVALID, "null domain"),
    ("amt_domain_upload", (None, 0, HOST), INVALID, "bad upload argument"),
    ("amt_domain_download", (None, 0, HOST), INVALID, "bad download argument"),
    ("amt_domain_upload_rows", (None, 0, 0, 0, HOST), INVALID, "bad row-copy argument"),
    ("amt_domain_download_rows", (None, 0, 0, 0, HOST), INVALID, "bad row-copy argument"),
    ("amt_domain_fill_synthetic", (None, 7, 0, 0, 0, 18, 9, 18), INVALID, "null domain"),
    ("amt_domain_fill_fields", (None, 1, 7, 0, 0, 0, 18, 9, 18), INVALID, "null domain"),
    ("amt_domain_poison_halos", (None, 1), INVALID, "bad poison argument"),
    ("amt_domain_step", (None, 1), INVALID, "bad step argument"),
    ("amt_domain_step_timed", (None, 1, None), INVALID, "bad step argument"),
    ("amt_domain_tune_placement", (None, 2, None), INVALID, "bad tuning argument"),
    ("amt_domain_sync", (None,), INVALID, "null domain"),
    ("amt_domain_cyclic_fill", (None, 1), INVALID, "null domain"),
    ("amt_domain_set_cyclic", (None, 1), INVALID, "null domain"),
    ("amt_domain_spec_bdy_update", (None,), INVALID, "null domain"),
    ("amt_domain_set_spec_bdy", (None, 1), INVALID, "null domain"),
    ("amt_domain_set_spec_bdy", (None, 0), INVALID, "null domain"),
    ("amt_ensemble_destroy", (None,), OK, None),
    ("amt_ensemble_set_scalars", (None, 1.0, 1.0, 1.0, 0.1), INVALID, "null ensemble"),
    ("amt_ensemble_set_variant", (None, 0), INVALID, "null ensemble"),
    ("amt_ensemble_upload_member", (None, 0, 0, HOST), INVALID, "bad member-copy argument"),
    ("amt_ensemble_download_member", (None, 0, 0, HOST), INVALID, "bad member-copy argument"),
    ("amt_ensemble_fill_synthetic", (None, 7, 0, 0, 0, 18, 9, 18), INVALID, "null ensemble"),
    ("amt_ensemble_step", (None, 1), INVALID, "bad step argument"),
    ("amt_ensemble_step_timed", (None, 1, None), INVALID, "bad step argument"),
    ("amt_ensemble_sync", (None,), INVALID, "null ensemble"),
    ("amt_ensemble_cyclic_fill", (None, 1), INVALID, "null ensemble"),
    ("amt_ensemble_set_cyclic", (None, 1), INVALID, "null ensemble"),
    ("amt_ensemble_spec_bdy_update", (None,), INVALID, "null ensemble"),
    ("amt_ensemble_set_spec_bdy", (None, 1), INVALID, "null ensemble"),
    ("amt_ensemble_set_spec_bdy", (None, 0), INVALID, "null ensemble"),
]

# the other arguments, refused in front of the first use of the handle
BAD_ARGUMENT = [
    ("amt_domain_set_variant", (BLANK, 7), INVALID, "unknown variant 7"),
    ("amt_domain_set_variant", (BLANK, -1), INVALID, "unknown variant -1"),
    ("amt_domain_upload", (BLANK, 0, None), INVALID, "bad upload argument"),
    ("amt_domain_upload", (BLANK, -1, HOST), INVALID, "bad upload argument"),
    ("amt_domain_upload", (BLANK, N_FIELDS, HOST), INVALID, "bad upload argument"),
    ("amt_domain_download", (BLANK, 0, None), INVALID, "bad download argument"),
    ("amt_domain_download", (BLANK, N_FIELDS, HOST), INVALID, "bad download argument"),
    ("amt_domain_upload_rows", (BLANK, 0, 0, 0, None), INVALID, "bad row-copy argument"),
    ("amt_domain_download_rows", (BLANK, N_FIELDS, 0, 0, HOST), INVALID, "bad row-copy argument"),
    ("amt_domain_upload_rows", (BLANK, 18, 0, 0, HOST), INVALID, "field 18 has no j rows"),
    ("amt_domain_fill_fields", (BLANK, 1 << N_FIELDS, 7, 0, 0, 0, 18, 9, 18), INVALID, "field mask names a field beyond AMT_F_COUNT"),
    ("amt_domain_poison_halos", (BLANK, 16), INVALID, "bad poison argument"),
    ("amt_domain_step", (BLANK, -1), INVALID, "bad step argument"),
    ("amt_domain_step_timed", (BLANK, -1, None), INVALID, "bad step argument"),
    ("amt_domain_tune_placement", (BLANK, 0, None), INVALID, "bad tuning argument"),
    ("amt_ensemble_set_variant", (BLANK, 7), INVALID, "unknown variant 7"),
    ("amt_ensemble_upload_member", (BLANK, 0, 0, None), INVALID, "bad member-copy argument"),
    ("amt_ensemble_download_member", (BLANK, N_FIELDS, 0, HOST), INVALID, "bad member-copy argument"),
    ("amt_ensemble_step", (BLANK, -1), INVALID, "bad step argument"),
    ("amt_ensemble_step_timed", (BLANK, -1, None), INVALID, "bad step argument"),
]

# getters: (call, arguments, value)
GETTERS = [
    ("amt_domain_cyclic", (None,), 0),
    ("amt_domain_spec_bdy", (None,), 0),
    ("amt_domain_field_ptr", (None, 0), None),
    ("amt_domain_field_ptr", (BLANK, -1), None),
    ("amt_domain_field_ptr", (BLANK, N_FIELDS), None),
    ("amt_domain_stream", (None,), None),
    ("amt_domain_placement", (None, None, 0), 0),
    ("amt_ensemble_cyclic", (None,), 0),
    ("amt_ensemble_spec_bdy", (None,), 0),
    ("amt_ensemble_members", (None,), 0),
    ("amt_ensemble_field_ptr", (None, 0), None),
    ("amt_ensemble_field_ptr", (BLANK, N_FIELDS), None),
    ("amt_ensemble_stream", (None,), None),
]


def _make_cases():
    """create / wrap: (call, arguments as a function of a fresh `out`, status, text).  The order of the checks is part of it."""
    D = lambda dt=8, b=BOUNDS: (dt, *FLAGS, *b)
    E = lambda m=2, dt=8, b=BOUNDS: (m, dt, *FLAGS, *b)
    rows = "1048576 members of 4096 rows: the stacked arrays have more than 2^31 - 1 rows"
    return [
        ("amt_domain_create", lambda o: (None, *D()), INVALID, "null out pointer"),
        ("amt_domain_create", lambda o: (o, *D(3)), INVALID, "dtype_bytes must be 4 or 8"),
        ("amt_domain_create", lambda o: (o, *D(0)), INVALID, "dtype_bytes must be 4 or 8"),
        ("amt_domain_create", lambda o: (o, *D(8, EMPTY_I)), PRECONDITION, "empty memory extents"),
        ("amt_domain_create", lambda o: (o, *D(4, EMPTY_J)), PRECONDITION, "empty memory extents"),
        ("amt_domain_create", lambda o: (o, *D(8, EMPTY_K)), PRECONDITION, "empty memory extents"),
        ("amt_domain_create", lambda o: (o, *D(3, EMPTY_K)), INVALID, "dtype_bytes must be 4 or 8"),
        ("amt_domain_wrap", lambda o: (o, *D(), None, None), INVALID, "amt_domain_wrap needs the 26 device pointers"),
        ("amt_domain_wrap", lambda o: (None, *D(), None, None), INVALID, "amt_domain_wrap needs the 26 device pointers"),
        ("amt_domain_wrap", lambda o: (None, *D(), _fields(), None), INVALID, "null out pointer"),
        ("amt_domain_wrap", lambda o: (o, *D(3), _fields(), None), INVALID, "dtype_bytes must be 4 or 8"),
        ("amt_domain_wrap", lambda o: (o, *D(8, EMPTY_J), _fields(), None), PRECONDITION, "empty memory extents"),
        ("amt_domain_wrap", lambda o: (o, *D(), _fields(0), None), INVALID, "amt_domain_wrap: field 0 is a null pointer"),
        ("amt_domain_wrap", lambda o: (o, *D(4), _fields(25), None), INVALID, "amt_domain_wrap: field 25 is a null pointer"),
        ("amt_domain_wrap", lambda o: (o, *D(8, EMPTY_I), _fields(5), None), PRECONDITION, "empty memory extents"),
        ("amt_ensemble_create", lambda o: (None, *E()), INVALID, "null out pointer"),
        ("amt_ensemble_create", lambda o: (o, *E(0)), INVALID, "members = 0: an ensemble has at least one member"),
        ("amt_ensemble_create", lambda o: (o, *E(-3)), INVALID, "members = -3: an ensemble has at least one member"),
        ("amt_ensemble_create", lambda o: (o, *E(0, 3)), INVALID, "members = 0: an ensemble has at least one member"),
        ("amt_ensemble_create", lambda o: (o, *E(2, 3)), INVALID, "dtype_bytes must be 4 or 8"),
        ("amt_ensemble_create", lambda o: (o, *E(2, 8, EMPTY_I)), PRECONDITION, "empty memory extents"),
        ("amt_ensemble_create", lambda o: (o, *E(2, 4, EMPTY_K)), PRECONDITION, "empty memory extents"),
        ("amt_ensemble_create", lambda o: (o, *E(1 << 20, 8, ROWS_4096)), PRECONDITION, rows),
        ("amt_ensemble_create", lambda o: (o, *E(1 << 20, 3, ROWS_4096)), INVALID, "dtype_bytes must be 4 or 8"),
        ("amt_ensemble_wrap", lambda o: (o, *E(), None, None), INVALID, "amt_ensemble_wrap needs the 26 device pointers"),
        ("amt_ensemble_wrap", lambda o: (None, *E(0), None, None), INVALID, "amt_ensemble_wrap needs the 26 device pointers"),
        ("amt_ensemble_wrap", lambda o: (None, *E(), _fields(), None), INVALID, "null out pointer"),
        ("amt_ensemble_wrap", lambda o: (o, *E(0), _fields(), None), INVALID, "members = 0: an ensemble has at least one member"),
        ("amt_ensemble_wrap", lambda o: (o, *E(2, 3), _fields(), None), INVALID, "dtype_bytes must be 4 or 8"),
        ("amt_ensemble_wrap", lambda o: (o, *E(2, 8, EMPTY_J), _fields(), None), PRECONDITION, "empty memory extents"),
        ("amt_ensemble_wrap", lambda o: (o, *E(1 << 20, 4, ROWS_4096), _fields(3), None), PRECONDITION, rows),
        ("amt_ensemble_wrap", lambda o: (o, *E(), _fields(0), None), INVALID, "amt_ensemble_wrap: field 0 is a null pointer"),
        ("amt_ensemble_wrap", lambda o: (o, *E(5, 4), _fields(17), None), INVALID, "amt_ensemble_wrap: field 17 is a null pointer"),
    ]


def _id(row):
    return row[0]


@pytest.mark.parametrize("row", NULL_HANDLE + BAD_ARGUMENT, ids=_id)
def test_a_refused_call_returns_its_status_and_its_text(pkg, row):
    L = pkg.load_library()
    name, args, status, text = row
    assert getattr(L, name)(*args) == status, (name, L.amt_last_error())
    if text is not None:
        assert L.amt_last_error().decode() == text, name


@pytest.mark.parametrize("row", GETTERS, ids=_id)
def test_a_getter_without_a_handle_returns_nothing(pkg, row):
    L = pkg.load_library()
    name, args, value = row
    assert getattr(L, name)(*args) == value, name


@pytest.mark.parametrize("k", range(len(_make_cases())), ids=[f"{r[0]}-{k}" for k, r in enumerate(_make_cases())])
def test_create_and_wrap_refuse_in_order_and_clear_the_out_pointer(pkg, k):
    L = pkg.load_library()
    name, make, status, text = _make_cases()[k]
    out = _out()
    args = make(out)
    assert getattr(L, name)(*args) == status, (name, L.amt_last_error())
    assert L.amt_last_error().decode() == text, name
    # *out is cleared by every refusal behind the null-out check (the wrap calls look at `fields` in front of it)
    cleared = args[0] is not None and "needs the 26 device pointers" not in text
    assert out.contents.value == (None if cleared else 0xdead), name
