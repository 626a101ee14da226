"""What the three streaming passes around the acoustic loop -- the flux averages, the stage bracket, the pressure diagnosis
(include/amt_advance_mu_t.h sections 14 to 16) -- answer on the paths that return before the first device call: one table of
(call, arguments, status, exact text of amt_last_error) for the eight pointer-level exports amt_sumflux_device_*,
amt_stage_prep_device_*, amt_stage_finish_device_* and amt_p_rho_device_*, and one for the handle exports on a zeroed handle.
Rows with two defects at once hold the ORDER of the checks; rows that return AMT_OK hold what each pass counts as empty; every
row leaves every array as it was, byte for byte.  A row marked ACCEPTED passes every check: without a device the call then
stops at the missing device (status 1 or 4); with one it would be launched on host memory, so such a row runs only where
amt_device_count() is 0.  No device is needed."""
import ctypes

import numpy as np
import pytest

OK, PRECONDITION, INVALID = 0, 2, 3
ACCEPTED = (1, 4)
DTS, T0, SMDIV = 1.7, 300.0, 0.1
F32, F64 = np.float32, np.float64

# pass -> the arrays in the export's argument order with their ranks, and the scalar arguments with a valid value
PASSES = {
    "sumflux": dict(arrays=dict(ru_m=3, rv_m=3, ww_m=3, u=3, v=3, ww=3, u_1=3, v_1=3, ww_1=3, muu=2, muv=2, msfuy=2, msfvx_inv=2),
                    scalars=dict(iteration=1, n=2)),
    "stage_prep": dict(arrays=dict(t=3, t_1=3, t_old=3, ww=3, ww_1=3, mu=2, mu_old=2, mu_save=2, muts=2, mudf=2, mut=2, mub=2),
                       scalars=dict(rk_step=1)),
    "stage_finish": dict(arrays=dict(t=3, t_1=3, ww=3, ww_1=3, mu=2, mu_save=2, muts=2, mut=2, h_diabatic=3),
                         scalars=dict(n=2)),
    "p_rho": dict(arrays=dict(al=3, p=3, ph=3, pm1=3, alt=3, c2a=3, t=3, t_old=3, mu=2, muts=2, rdnw=1, znu=1, dnw=1),
                  scalars=dict(mode=1, step=0)),
}
OVERLAP = "an output array overlaps another array of the call"
MEMBERS_0 = "members = 0: an ensemble has at least one member"
EXTENTS = "empty memory extents"


def _patch(pkg):
    return pkg.synth.domain_bounds(5, 3, 4)                       # memory 0:6, 1:4, 0:5; tile 1:6, 1:4, 1:5


def _one_cell(pkg):
    return pkg.synth.Bounds(ids=1, ide=2, jds=1, jde=2, kde=2, ims=1, ime=1, jms=1, jme=1, kms=1, kme=2, its=1, ite=1, jts=1, jte=1,
                            kts=1, kte=2)


def _arrays(name, b, dtype, members):
    shape = {3: (members, b.jdim, b.kdim, b.idim), 2: (members, b.jdim, b.idim), 1: (b.kdim,)}
    rng = np.random.default_rng(5)
    return {n: rng.uniform(0.5, 1.5, shape[r]).astype(dtype) for n, r in PASSES[name]["arrays"].items()}


def _invoke(L, name, dtype, arrays, b, members, scalars):
    fn = getattr(L, f"amt_{name}_device_{'f64' if dtype is F64 else 'f32'}")
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    s = dict(PASSES[name]["scalars"], **scalars)
    p = [ptr(arrays[n]) for n in PASSES[name]["arrays"]]
    if name == "sumflux":
        return fn(None, members, *p, s["iteration"], s["n"], *b.as_tuple())
    if name == "stage_prep":
        return fn(None, members, *p, s["rk_step"], *b.as_tuple())
    if name == "stage_finish":
        return fn(None, members, *p[:8], DTS, s["n"], p[8], *b.as_tuple())
    return fn(None, members, s["mode"], s["step"], *p, T0, SMDIV, *b.as_tuple())


def _flat(a):
    return a.reshape(-1)


def _behind_znu(elements_into):
    """al starts `elements_into` elements before the end of the kdim elements of znu, in one buffer."""
    def swap(a):
        buf = np.full(a["znu"].size + a["al"].size, 1.25, a["al"].dtype)
        at = a["znu"].size - elements_into
        return dict(znu=buf[:a["znu"].size], al=buf[at:at + a["al"].size].reshape(a["al"].shape), _buffer=buf)
    return swap


# A row: (pass, what, keywords, status, text behind "<export>: ").  Keywords: null = arrays passed as NULL; swap = a function
# of the arrays that returns the ones to replace; bounds = a function of the patch's bounds; members; one_cell = the one-cell
# patch (whose arrays are real at 65536 members); every other keyword is a scalar argument of the pass.
def _rows():
    rows = []
    add = lambda name, what, status, text, **kw: rows.append((name, what, kw, status, text))
    no_extents = lambda b: b.replace(ime=b.ims - 1)
    outside = "the tile 0:1, 1:1 is not inside memory 1:1, 1:1"
    for name, spec in PASSES.items():
        first, out = list(spec["arrays"])[0], list(spec["arrays"])[0]
        other = dict(sumflux="u", stage_prep="mut", stage_finish="t_1", p_rho="alt")[name]          # an input of the pass
        overlap = "an accumulator overlaps an input array" if name == "sumflux" else OVERLAP
        bad = dict(sumflux=[(dict(n=0), "n_small_steps = 0: an acoustic loop has at least one sub-step"),
                            (dict(n=-2), "n_small_steps = -2: an acoustic loop has at least one sub-step"),
                            (dict(iteration=0), "iteration 0 is not in 1..2"), (dict(iteration=3), "iteration 3 is not in 1..2")],
                   stage_prep=[(dict(rk_step=0), "rk_step = 0: at least 1"), (dict(rk_step=-3), "rk_step = -3: at least 1")],
                   stage_finish=[(dict(n=0), "n_small_steps = 0: at least 1"), (dict(n=-2), "n_small_steps = -2: at least 1")],
                   p_rho=[(dict(mode=0), "mode = 0: 1 (non-hydrostatic) or 2 (hydrostatic)"),
                          (dict(mode=3), "mode = 3: 1 (non-hydrostatic) or 2 (hydrostatic)"), (dict(step=-1), "step = -1: at least 0")])[name]
        alias = lambda a, out=out, other=other: {other: a[out]}
        # one defect each, in the order of the check
        for n in spec["arrays"]:
            if name == "stage_finish" and n == "h_diabatic":
                continue
            add(name, f"null {n}", INVALID, "null array pointer", null=(n,))
        add(name, "members 0", INVALID, MEMBERS_0, members=0)
        add(name, "members -1", INVALID, "members = -1: an ensemble has at least one member", members=-1)
        for kw, text in bad:
            add(name, f"bad {kw}", INVALID, text, **kw)
        for what, f in [("ime < ims", no_extents), ("jme < jms", lambda b: b.replace(jme=b.jms - 1)), ("kme < kms", lambda b: b.replace(kme=b.kms - 1))]:
            add(name, f"no extents, {what}", PRECONDITION, EXTENTS, bounds=f)
        add(name, f"{other} is {out}", INVALID, overlap, swap=alias)
        add(name, f"{other} one element into {out}", INVALID, overlap, swap=lambda a, out=out, other=other: {other: _flat(a[out])[1:]})
        add(name, "kts 2", PRECONDITION, "kts = 2, the library needs kts == 1", bounds=lambda b: b.replace(kts=2))
        add(name, "kte is not kde", PRECONDITION, "kte = 3 is not kde = 4", bounds=lambda b: b.replace(kte=3))
        add(name, "kme < kte", PRECONDITION, "levels kts:kte = 1:4 are not inside memory kms:kme = 1:3", bounds=lambda b: b.replace(kme=3))
        add(name, "kms > kts", PRECONDITION, "levels kts:kte = 1:4 are not inside memory kms:kme = 2:4", bounds=lambda b: b.replace(kms=2))
        add(name, "its < ims", PRECONDITION, "the tile -1:6, 1:5 is not inside memory 0:6, 0:5", bounds=lambda b: b.replace(its=-1))
        add(name, "ite > ime", PRECONDITION, "the tile 1:7, 1:5 is not inside memory 0:6, 0:5", bounds=lambda b: b.replace(ite=7))
        add(name, "jts < jms", PRECONDITION, "the tile 1:6, -1:5 is not inside memory 0:6, 0:5", bounds=lambda b: b.replace(jts=-1))
        add(name, "jte > jme", PRECONDITION, "the tile 1:6, 1:6 is not inside memory 0:6, 0:5", bounds=lambda b: b.replace(jte=6))
        add(name, "65536 members", PRECONDITION, "65536 members: one launch covers at most 65535", members=65536, one_cell=True)
        # two defects at once: the first in the order of the check answers
        add(name, "null array, members 0", INVALID, "null array pointer", null=(first,), members=0)
        add(name, f"members 0, bad {bad[0][0]}", INVALID, MEMBERS_0, members=0, **bad[0][0])
        for kw, text in bad:
            add(name, f"bad {kw}, no extents", INVALID, text, bounds=no_extents, **kw)
        add(name, "no extents, overlap", PRECONDITION, EXTENTS, bounds=no_extents, swap=alias)
        add(name, "overlap, kts 2", INVALID, overlap, swap=alias, bounds=lambda b: b.replace(kts=2))
        add(name, "kts 2, kte is not kde", PRECONDITION, "kts = 2, the library needs kts == 1", bounds=lambda b: b.replace(kts=2, kte=3))
        add(name, "kte is not kde, kme < kte", PRECONDITION, "kte = 5 is not kde = 4", bounds=lambda b: b.replace(kte=5))
        add(name, "tile outside memory, 65536 members", PRECONDITION, outside, members=65536, one_cell=True, bounds=lambda b: b.replace(its=0))
        # what counts as empty: AMT_OK, the text of the last error stays, nothing is touched
        add(name, "ite < its", OK, None, bounds=lambda b: b.replace(ite=0))
        add(name, "jte < jts", OK, None, bounds=lambda b: b.replace(jte=0))
        add(name, "ite < its outside memory", OK, None, bounds=lambda b: b.replace(its=9, ite=8))      # empty in front of the tile check
        one_level = lambda b: b.replace(kde=1, kte=1)
        add(name, "kte == kts", OK if name == "p_rho" else ACCEPTED, None, bounds=one_level)
        for what, f in [("its == ide", lambda b: b.replace(its=b.ide)), ("jts == jde", lambda b: b.replace(jts=b.jde))]:
            add(name, f"no mass column, {what}", ACCEPTED if name == "sumflux" else OK, None, bounds=f)
        if name != "sumflux":                                     # the mass range is looked at behind the tile and the members
            add(name, "no mass column, 65536 members", PRECONDITION, "65536 members: one launch covers at most 65535", members=65536,
                one_cell=True, bounds=lambda b: b.replace(ide=1))
        add(name, "every check passes", ACCEPTED, None)
    # sumflux has two overlap texts: accumulator against accumulator comes first for each accumulator
    add("sumflux", "rv_m is ru_m", INVALID, "two accumulators overlap", swap=lambda a: dict(rv_m=a["ru_m"]))
    add("sumflux", "ww_m one element into rv_m", INVALID, "two accumulators overlap", swap=lambda a: dict(ww_m=_flat(a["rv_m"])[1:]))
    add("sumflux", "u is ru_m, ww_m is rv_m", INVALID, "an accumulator overlaps an input array", swap=lambda a: dict(u=a["ru_m"], ww_m=a["rv_m"]))
    add("sumflux", "muu inside ww_m", INVALID, "an accumulator overlaps an input array", swap=lambda a: dict(muu=_flat(a["ww_m"])[5:5 + a["muu"].size]))
    add("sumflux", "inputs alias one another", ACCEPTED, None, swap=lambda a: dict(v=a["u"], ww=a["u"], v_1=a["u_1"], muv=a["muu"]))
    # the ranks of the overlap test.  p_rho: rdnw, znu and dnw count kdim elements whatever the members
    add("p_rho", "two members, al behind the kdim elements of znu", ACCEPTED, None, members=2, swap=_behind_znu(0))
    add("p_rho", "two members, al one element into znu", INVALID, OVERLAP, members=2, swap=_behind_znu(1))
    add("p_rho", "dnw is the end of p", INVALID, OVERLAP, swap=lambda a: dict(dnw=_flat(a["p"])[-a["dnw"].size:]))
    add("p_rho", "mu inside pm1", INVALID, OVERLAP, swap=lambda a: dict(mu=_flat(a["pm1"])[5:5 + a["mu"].size]))
    add("p_rho", "alt is ph, mode 1", ACCEPTED, None, swap=lambda a: dict(alt=a["ph"]))                 # ph is an output in mode 2 only
    add("p_rho", "alt is ph, mode 2", INVALID, OVERLAP, mode=2, swap=lambda a: dict(alt=a["ph"]))
    add("p_rho", "bad mode, ph is al", INVALID, "mode = 3: 1 (non-hydrostatic) or 2 (hydrostatic)", mode=3, swap=lambda a: dict(ph=a["al"]))
    # the stage bracket's optional arrays: h_diabatic may be NULL; mudf at rk_step > 1 takes no part
    add("stage_finish", "h_diabatic null", ACCEPTED, None, null=("h_diabatic",))
    add("stage_finish", "h_diabatic null, members 0", INVALID, MEMBERS_0, null=("h_diabatic",), members=0)
    add("stage_finish", "h_diabatic one element into t", INVALID, OVERLAP, swap=lambda a: dict(h_diabatic=_flat(a["t"])[1:]))
    add("stage_finish", "h_diabatic is t_1", ACCEPTED, None, swap=lambda a: dict(h_diabatic=a["t_1"]))
    add("stage_prep", "mudf null, rk_step 2", ACCEPTED, None, null=("mudf",), rk_step=2)
    add("stage_prep", "mudf is the end of t, rk_step 2", ACCEPTED, None, rk_step=2, swap=lambda a: dict(mudf=_flat(a["t"])[-a["mudf"].size:]))
    add("stage_prep", "mudf is the end of t, rk_step 1", INVALID, OVERLAP, swap=lambda a: dict(mudf=_flat(a["t"])[-a["mudf"].size:]))
    add("stage_prep", "t_old is ww, rk_step 2", ACCEPTED, None, rk_step=2, swap=lambda a: dict(t_old=a["ww"], mu_old=a["mub"]))   # inputs then
    add("stage_prep", "t_old is ww, rk_step 1", INVALID, OVERLAP, swap=lambda a: dict(t_old=a["ww"]))
    return rows


ROWS = _rows()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("k", range(len(ROWS)), ids=[f"{r[0]}-{r[1]}".replace(" ", "_") for r in ROWS])
def test_a_pointer_level_call_answers_with_its_status_and_its_text_and_writes_nothing(pkg, k, dtype):
    L = pkg.load_library()
    name, what, kw, status, text = ROWS[k]
    kw = dict(kw)
    if status == ACCEPTED and L.amt_device_count() != 0:
        return                                                    # would be launched on host memory
    members = kw.pop("members", 1)
    b = _one_cell(pkg) if kw.pop("one_cell", False) else _patch(pkg)
    arrays = _arrays(name, b, dtype, max(members, 1))
    b = kw.pop("bounds", lambda x: x)(b)
    arrays.update(kw.pop("swap", lambda a: {})(arrays))
    for n in kw.pop("null", ()):
        arrays[n] = None
    before = {n: a.tobytes() for n, a in arrays.items() if a is not None}
    who = f"amt_{name}_device_{'f64' if dtype is F64 else 'f32'}"
    assert L.amt_domain_sync(None) == INVALID                     # a text of another call, for the rows that leave it
    earlier = L.amt_last_error()
    got = _invoke(L, name, dtype, arrays, b, members, kw)
    if status == ACCEPTED:
        assert got in ACCEPTED, (what, L.amt_last_error())       # the text then names the HIP call that found no device
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
ROOM = [ctypes.c_void_p(ctypes.addressof(_room) + 64 * k) for k in range(8)]
NONE8 = [None] * 8
STAGE_OFF = "the stage bracket is off (amt_*_set_stage)"
NEEDS_STAGE = "the stage bracket, whose t_old the diagnosis reads, is off (amt_*_set_stage)"
ALL = "give all %s or none (the library then allocates them)"
ADMIT = "the handle's tile does not admit %s (kts == 1, kte == kde, tile inside memory)"
BAD_MODE = "mode = %d: 0 (off), 1 (non-hydrostatic) or 2 (hydrostatic)"

# (call behind the prefix, arguments, status, text; None: the text is "null domain" / "null ensemble")
HANDLE = [
    ("set_sumflux", (None, 2, None, None, None), INVALID, None),
    ("sumflux_accumulate", (None,), INVALID, None),
    ("sumflux_state", (None, None, None), INVALID, None),
    ("set_stage", (None, 1, None, None, None, None), INVALID, None),
    ("set_stage", (None, 0, None, None, None, None), INVALID, None),
    ("stage_prep", (None, 1), INVALID, None),
    ("stage_finish", (None, 1, None), INVALID, None),
    ("set_p_rho", (None, 1, 0, T0, SMDIV, *NONE8), INVALID, None),
    ("set_p_rho", (None, 0, 0, T0, SMDIV, *NONE8), INVALID, None),
    ("p_rho", (None, 0), INVALID, None),
    # the setting is off: INVALID for the flux averages, PRECONDITION for the other two, whatever the other arguments
    ("sumflux_accumulate", (BLANK,), INVALID, "{p}_sumflux_accumulate: the flux averages are off (amt_*_set_sumflux)"),
    ("stage_prep", (BLANK, 1), PRECONDITION, "{p}_stage_prep: " + STAGE_OFF),
    ("stage_prep", (BLANK, 0), PRECONDITION, "{p}_stage_prep: " + STAGE_OFF),
    ("stage_finish", (BLANK, 3, None), PRECONDITION, "{p}_stage_finish: " + STAGE_OFF),
    ("stage_finish", (BLANK, 0, ROOM[0]), PRECONDITION, "{p}_stage_finish: " + STAGE_OFF),
    ("p_rho", (BLANK, 0), PRECONDITION, "{p}_p_rho: the pressure diagnosis is off (amt_*_set_p_rho)"),
    ("p_rho", (BLANK, -1), PRECONDITION, "{p}_p_rho: the pressure diagnosis is off (amt_*_set_p_rho)"),
    # set_sumflux: n, then all or none, then the check of the pointer-level call or the handle's tile
    ("set_sumflux", (BLANK, -1, None, None, None), INVALID, "{p}_set_sumflux: n_small_steps = -1"),
    ("set_sumflux", (BLANK, -1, ROOM[0], None, None), INVALID, "{p}_set_sumflux: n_small_steps = -1"),
    ("set_sumflux", (BLANK, 2, ROOM[0], None, None), INVALID, "{p}_set_sumflux: " + ALL % "three accumulators"),
    ("set_sumflux", (BLANK, 2, None, ROOM[1], ROOM[2]), INVALID, "{p}_set_sumflux: " + ALL % "three accumulators"),
    ("set_sumflux", (BLANK, 2, ROOM[0], ROOM[1], ROOM[2]), INVALID, "{p}_set_sumflux: null array pointer"),
    ("set_sumflux", (BLANK, 2, None, None, None), PRECONDITION, "{p}_set_sumflux: " + ADMIT % "the flux averages"),
    # set_stage
    ("set_stage", (BLANK, 1, ROOM[0], None, None, None), INVALID, "{p}_set_stage: " + ALL % "four arrays"),
    ("set_stage", (BLANK, 1, ROOM[0], ROOM[1], None, ROOM[3]), INVALID, "{p}_set_stage: " + ALL % "four arrays"),
    ("set_stage", (BLANK, 1, *ROOM[:4]), INVALID, "{p}_set_stage: null array pointer"),
    ("set_stage", (BLANK, 1, None, None, None, None), PRECONDITION, "{p}_set_stage: " + ADMIT % "the stage bracket"),
    # set_p_rho: the mode, then all or none, then the stage bracket
    ("set_p_rho", (BLANK, 3, 1, T0, SMDIV, *NONE8), INVALID, "{p}_set_p_rho: " + BAD_MODE % 3),
    ("set_p_rho", (BLANK, -1, 1, T0, SMDIV, ROOM[0], *NONE8[1:]), INVALID, "{p}_set_p_rho: " + BAD_MODE % -1),
    ("set_p_rho", (BLANK, 1, 1, T0, SMDIV, ROOM[0], *NONE8[1:]), INVALID, "{p}_set_p_rho: " + ALL % "eight arrays"),
    ("set_p_rho", (BLANK, 2, 0, T0, SMDIV, *ROOM[:5], None, *ROOM[6:]), INVALID, "{p}_set_p_rho: " + ALL % "eight arrays"),
    ("set_p_rho", (BLANK, 1, 1, T0, SMDIV, *NONE8), PRECONDITION, "{p}_set_p_rho: " + NEEDS_STAGE),
    ("set_p_rho", (BLANK, 2, 0, T0, SMDIV, *ROOM), PRECONDITION, "{p}_set_p_rho: " + NEEDS_STAGE),
]


@pytest.mark.parametrize("prefix,who", [("amt_domain", "null domain"), ("amt_ensemble", "null ensemble")])
@pytest.mark.parametrize("k", range(len(HANDLE)), ids=[f"{r[0]}-{k}" for k, r in enumerate(HANDLE)])
def test_a_handle_call_refuses_with_its_status_and_its_text_and_changes_nothing(pkg, k, prefix, who):
    L = pkg.load_library()
    call, args, status, text = HANDLE[k]
    assert getattr(L, f"{prefix}_{call}")(*args) == status, (call, L.amt_last_error())
    assert L.amt_last_error().decode() == (who if text is None else text.format(p=prefix)), call
    for name, count in (("sumflux_ptr", 3), ("stage_ptr", 4), ("p_rho_ptr", 8)):
        assert all(getattr(L, f"{prefix}_{name}")(BLANK, which) is None for which in range(-1, count + 1))
    assert bytes(_blank) == bytes(8192)
