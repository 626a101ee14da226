"""The three settings of the passes around the acoustic loop on a resident handle -- amt_*_set_sumflux, amt_*_set_stage,
amt_*_set_p_rho (include/amt_advance_mu_t.h sections 14 to 16) --: who owns the arrays after each call, what a refusal leaves,
and the exact text of every refusal.  One 17 x 9 x 17 handle with a halo of 1, as a domain and as an ensemble of two members,
fp32 and fp64.  After every call: the status and the text, the *_ptr getters, and whether the setting is on -- the counter of
the flux averages, the pass's own call for the other two.  What the passes compute is held by tests/test_gpu_38*, 39* and 41*."""
import ctypes

import numpy as np
import pytest

import test_gpu_38_sumflux as T38

pytestmark = pytest.mark.gpu

OK, PRECONDITION, INVALID = 0, 2, 3
F64, F32 = np.float64, np.float32
T0, SMDIV = 300.0, 0.1
MEMBERS = 2
ALL = "give all %s or none (the library then allocates them)"
OVERLAP = "an output array overlaps another array of the call"
MIXED = "an array the library allocated, mixed with others"
STAGE_OFF = "the stage bracket is off (amt_*_set_stage)"
P_RHO_OFF = "the pressure diagnosis is off (amt_*_set_p_rho)"
NEEDS_STAGE = "the stage bracket, whose t_old the diagnosis reads, is off (amt_*_set_stage)"


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


class Handle:
    """A created handle and its exports by their name behind amt_domain_ / amt_ensemble_."""

    def __init__(self, pkg, torch, kind, dtype):
        self.L, self.torch, self.dtype = pkg.load_library(), torch, dtype
        self.S = pkg.synth
        self.b = self.S.domain_bounds(16, 8, 16)                   # ide = jde = 17, kde = 9; memory 0:17, 1:9, 0:17
        self.prefix = f"amt_{kind}"
        self.members = MEMBERS if kind == "ensemble" else 1
        self.h = ctypes.c_void_p()
        lead = (MEMBERS,) if kind == "ensemble" else ()
        assert self.fn("create")(ctypes.byref(self.h), *lead, np.dtype(dtype).itemsize, 0, 0, 0, *self.b.as_tuple()) == OK, self.L.amt_last_error()
        try:
            assert self.fn("fill_synthetic")(self.h, 7, 0, 0, 0, self.b.idim, self.b.kdim, self.b.jdim) == OK, self.L.amt_last_error()
        except BaseException:
            self.close()
            raise

    def fn(self, name):
        return getattr(self.L, f"{self.prefix}_{name}")

    def close(self):
        self.fn("sync")(self.h)
        self.fn("destroy")(self.h)

    def expect(self, name, args, status, text=None):
        """One call: its status, and the exact text of a refusal; a call that returns AMT_OK leaves the text of the last error."""
        assert self.L.amt_domain_sync(None) == INVALID
        got = self.fn(name)(self.h, *args)
        assert got == status, (name, got, self.L.amt_last_error())
        assert self.L.amt_last_error().decode() == ("null domain" if status == OK else f"{self.prefix}_{name}: {text}"), name

    def ptrs(self, name, count):
        assert self.fn(name)(self.h, -1) is None and self.fn(name)(self.h, count) is None
        return [self.fn(name)(self.h, k) for k in range(count)]

    def field(self, name):
        return ctypes.c_void_p(self.fn("field_ptr")(self.h, self.S.FIELD_NAMES.index(name)))

    def room(self, rank, value=1.0):
        """An array of the caller's: one field's extents, times the members for rank 3 and 2."""
        b = self.b
        shape = {3: (self.members, b.jdim, b.kdim, b.idim), 2: (self.members, b.jdim, b.idim), 1: (b.kdim,)}[rank]
        return self.torch.full(shape, value, dtype=self.torch.float64 if self.dtype is F64 else self.torch.float32, device="cuda:0")

    def sumflux_state(self):
        return T38._state(self.L, self.h, self.prefix)


@pytest.fixture(params=[("domain", F64), ("domain", F32), ("ensemble", F64), ("ensemble", F32)], ids=lambda p: f"{p[0]}-{np.dtype(p[1]).name}")
def handle(request, pkg, torch_mod):
    h = Handle(pkg, torch_mod, *request.param)
    yield h
    h.close()


def _address(t):
    return ctypes.c_void_p(t.data_ptr())


def _distinct(ptrs):
    return all(ptrs) and len(set(ptrs)) == len(ptrs)


def test_set_sumflux(handle):
    H = handle
    none3 = (None, None, None)
    off = "the flux averages are off (amt_*_set_sumflux)"
    assert H.ptrs("sumflux_ptr", 3) == [None] * 3 and H.sumflux_state() == (0, 1)
    H.expect("sumflux_accumulate", (), INVALID, off)
    # the library allocates
    H.expect("set_sumflux", (3, *none3), OK)
    mine = H.ptrs("sumflux_ptr", 3)
    assert _distinct(mine) and H.sumflux_state() == (3, 1)
    H.expect("sumflux_accumulate", (), OK)
    assert H.sumflux_state() == (3, 2)
    # its own arrays handed back: they stay, n and the counter are set anew
    H.expect("set_sumflux", (2, *mine), OK)
    assert H.ptrs("sumflux_ptr", 3) == mine and H.sumflux_state() == (2, 1)
    H.expect("sumflux_accumulate", (), OK)
    assert H.sumflux_state() == (2, 2)
    # refusals change nothing: one of the library's among the caller's, the caller's overlapping a field or one another
    theirs = [H.room(3) for _ in range(3)]
    given = [_address(t) for t in theirs]
    refusals = [((5, mine[0], given[1], given[2]), "an accumulator the library allocated, mixed with others"),
                ((5, given[0], given[1], mine[1]), "an accumulator the library allocated, mixed with others"),
                ((5, given[0], None, given[2]), ALL % "three accumulators"),
                ((-1, *given), "n_small_steps = -1"),
                ((5, H.field("u"), given[1], given[2]), "an accumulator overlaps an input array"),
                ((5, given[0], given[1], _address(theirs[1].view(-1)[1:])), "two accumulators overlap")]
    for args, text in refusals:
        H.expect("set_sumflux", args, INVALID, text)
        assert H.ptrs("sumflux_ptr", 3) == mine and H.sumflux_state() == (2, 2), text
    # the caller's arrays replace the library's, the library's replace the caller's
    H.expect("set_sumflux", (4, *given), OK)
    assert H.ptrs("sumflux_ptr", 3) == [g.value for g in given] and H.sumflux_state() == (4, 1)
    H.expect("sumflux_accumulate", (), OK)
    assert H.sumflux_state() == (4, 2)
    H.expect("set_sumflux", (2, *none3), OK)
    again = H.ptrs("sumflux_ptr", 3)
    assert _distinct(again) and not set(again) & {g.value for g in given} and H.sumflux_state() == (2, 1)
    H.expect("sumflux_accumulate", (), OK)
    H.expect("sumflux_accumulate", (), OK)
    assert H.sumflux_state() == (2, 1)                            # the counter wraps
    # off, then off again
    for _ in range(2):
        H.expect("set_sumflux", (0, *none3), OK)
        assert H.ptrs("sumflux_ptr", 3) == [None] * 3 and H.sumflux_state() == (0, 1)
        H.expect("sumflux_accumulate", (), INVALID, off)
    H.expect("set_sumflux", (0, *given), OK)                      # off looks at no array
    assert H.ptrs("sumflux_ptr", 3) == [None] * 3


def test_set_stage(handle):
    H = handle
    none4 = (None,) * 4

    def on(yes):
        if yes:
            H.expect("stage_prep", (2,), OK)
            H.expect("stage_finish", (2, None), OK)
        else:
            H.expect("stage_prep", (2,), PRECONDITION, STAGE_OFF)
            H.expect("stage_finish", (2, None), PRECONDITION, STAGE_OFF)

    assert H.ptrs("stage_ptr", 4) == [None] * 4
    on(False)
    # the library allocates
    H.expect("set_stage", (1, *none4), OK)
    mine = H.ptrs("stage_ptr", 4)
    assert _distinct(mine)
    on(True)
    # its own arrays handed back: nothing changes
    H.expect("set_stage", (1, *mine), OK)
    assert H.ptrs("stage_ptr", 4) == mine
    on(True)
    theirs = [H.room(3)] + [H.room(2) for _ in range(3)]
    given = [_address(t) for t in theirs]
    refusals = [((1, mine[0], *given[1:]), MIXED), ((1, *given[:3], mine[0]), MIXED), ((1, given[0], None, *given[2:]), ALL % "four arrays"),
                ((1, H.field("t"), *given[1:]), OVERLAP), ((1, given[0], given[1], given[1], given[3]), OVERLAP),
                ((1, *given[:3], H.field("muts")), OVERLAP)]
    for args, text in refusals:
        H.expect("set_stage", args, INVALID, text)
        assert H.ptrs("stage_ptr", 4) == mine, text
        on(True)
    # the caller's arrays replace the library's, the library's replace the caller's
    H.expect("set_stage", (1, *given), OK)
    assert H.ptrs("stage_ptr", 4) == [g.value for g in given]
    on(True)
    H.expect("set_stage", (1, *none4), OK)
    again = H.ptrs("stage_ptr", 4)
    assert _distinct(again) and not set(again) & {g.value for g in given}
    on(True)
    # off, then off again
    for _ in range(2):
        H.expect("set_stage", (0, *none4), OK)
        assert H.ptrs("stage_ptr", 4) == [None] * 4
        on(False)
    H.expect("set_stage", (0, given[0], None, None, None), OK)    # off looks at no array
    assert H.ptrs("stage_ptr", 4) == [None] * 4


def test_set_p_rho(handle):
    H, torch = handle, handle.torch
    none8 = (None,) * 8
    theirs = [H.room(3) for _ in range(6)] + [H.room(1, 0.5), H.room(1, -0.2)]
    given = [_address(t) for t in theirs]
    bad_mode = "mode = 3: 0 (off), 1 (non-hydrostatic) or 2 (hydrostatic)"
    # the stage bracket is off: refused behind the mode and "all eight", in front of everything else
    H.expect("set_p_rho", (3, 1, T0, SMDIV, given[0], *none8[1:]), INVALID, bad_mode)
    H.expect("set_p_rho", (1, 1, T0, SMDIV, given[0], *none8[1:]), INVALID, ALL % "eight arrays")
    H.expect("set_p_rho", (1, 1, T0, SMDIV, *none8), PRECONDITION, NEEDS_STAGE)
    H.expect("set_p_rho", (2, 0, T0, SMDIV, *given), PRECONDITION, NEEDS_STAGE)
    H.expect("set_p_rho", (2, 0, T0, SMDIV, given[0], H.field("t"), *given[2:]), PRECONDITION, NEEDS_STAGE)      # p is t: not looked at yet
    H.expect("p_rho", (0,), PRECONDITION, P_RHO_OFF)
    assert H.ptrs("p_rho_ptr", 8) == [None] * 8

    def stage_on():
        H.expect("set_stage", (1, None, None, None, None), OK)
        T38._view(torch, H.ptrs("stage_ptr", 4)[3], (H.members, H.b.jdim, H.b.idim), H.dtype).fill_(1.0)     # mub is the host's to fill
        torch.cuda.synchronize()
        H.expect("stage_prep", (1,), OK)

    stage_on()
    H.expect("p_rho", (0,), PRECONDITION, P_RHO_OFF)
    # the library allocates
    H.expect("set_p_rho", (1, 0, T0, SMDIV, *none8), OK)
    mine = H.ptrs("p_rho_ptr", 8)
    assert _distinct(mine)
    shapes = [theirs[k].shape for k in range(8)]
    views = [T38._view(torch, mine[k], shapes[k], H.dtype) for k in range(8)]
    for k, value in enumerate((1.0, 1.0, 1.0, 1.0, 1.0, 10.0, 0.5, -0.2)):                  # al, p, ph, pm1, alt, c2a, znu, dnw
        views[k].fill_(value)
    torch.cuda.synchronize()

    def ph_after_a_diagnosis():
        views[2].fill_(1.0)
        torch.cuda.synchronize()
        H.expect("p_rho", (0,), OK)
        assert H.fn("sync")(H.h) == OK
        return views[2].cpu().numpy()

    assert (ph_after_a_diagnosis() == 1.0).all()                   # mode 1 reads ph
    # its own arrays handed back: they stay, the mode and the scalars are set anew -- mode 2 integrates ph
    H.expect("set_p_rho", (2, 0, T0, SMDIV, *mine), OK)
    assert H.ptrs("p_rho_ptr", 8) == mine
    assert (ph_after_a_diagnosis() != 1.0).any()
    H.expect("set_p_rho", (1, 0, T0, SMDIV, *mine), OK)
    assert H.ptrs("p_rho_ptr", 8) == mine
    assert (ph_after_a_diagnosis() == 1.0).all()
    H.expect("set_p_rho", (2, 0, T0, SMDIV, *mine), OK)
    # refusals change nothing: the pointers stay, the mode stays 2
    refusals = [((3, 0, T0, SMDIV, *given), INVALID, bad_mode), ((1, 0, T0, SMDIV, *given[:7], None), INVALID, ALL % "eight arrays"),
                ((1, 0, T0, SMDIV, *mine[:7], given[7]), INVALID, MIXED), ((1, 0, T0, SMDIV, *given[:7], mine[0]), INVALID, MIXED),
                ((1, 0, T0, SMDIV, given[0], H.field("t"), *given[2:]), INVALID, OVERLAP),
                ((1, 0, T0, SMDIV, *given[:3], given[0], *given[4:]), INVALID, OVERLAP),
                ((2, 0, T0, SMDIV, given[0], given[1], H.field("mu"), *given[3:]), INVALID, OVERLAP)]
    for args, status, text in refusals:
        H.expect("set_p_rho", args, status, text)
        assert H.ptrs("p_rho_ptr", 8) == mine, text
        assert (ph_after_a_diagnosis() != 1.0).any(), text
    # the stage bracket goes off under the setting: the diagnosis and the setting both say so, the setting stays what it was
    H.expect("set_stage", (0, None, None, None, None), OK)
    H.expect("p_rho", (0,), PRECONDITION, NEEDS_STAGE)
    H.expect("set_p_rho", (1, 0, T0, SMDIV, *mine), PRECONDITION, NEEDS_STAGE)
    H.expect("set_p_rho", (1, 0, T0, SMDIV, *mine[:7], given[7]), PRECONDITION, NEEDS_STAGE)
    assert H.ptrs("p_rho_ptr", 8) == mine
    stage_on()
    assert (ph_after_a_diagnosis() != 1.0).any()
    # the caller's arrays replace the library's, the library's replace the caller's
    H.expect("set_p_rho", (1, 0, T0, SMDIV, *given), OK)
    assert H.ptrs("p_rho_ptr", 8) == [g.value for g in given]
    H.expect("p_rho", (0,), OK)
    H.expect("p_rho", (1,), OK)
    H.expect("p_rho", (-1,), INVALID, "step = -1: at least 0")
    H.expect("set_p_rho", (2, 1, T0, SMDIV, *none8), OK)
    again = H.ptrs("p_rho_ptr", 8)
    assert _distinct(again) and not set(again) & {g.value for g in given}
    H.expect("p_rho", (0,), OK)
    # off, then off again
    for _ in range(2):
        H.expect("set_p_rho", (0, 0, T0, SMDIV, *none8), OK)
        assert H.ptrs("p_rho_ptr", 8) == [None] * 8
        H.expect("p_rho", (0,), PRECONDITION, P_RHO_OFF)
    H.expect("set_p_rho", (0, 1, T0, SMDIV, given[0], *none8[1:]), OK)      # off looks at no array
    assert H.ptrs("p_rho_ptr", 8) == [None] * 8


def test_destroy_with_the_three_settings_on_and_library_owned(handle):
    H = handle
    H.expect("set_sumflux", (2, None, None, None), OK)
    H.expect("set_stage", (1, None, None, None, None), OK)
    H.expect("set_p_rho", (2, 1, T0, SMDIV, *[None] * 8), OK)
    assert _distinct(H.ptrs("sumflux_ptr", 3) + H.ptrs("stage_ptr", 4) + H.ptrs("p_rho_ptr", 8))
    H.expect("stage_prep", (1,), OK)
    H.expect("p_rho", (0,), OK)
    H.expect("step", (2,), OK)                                    # the accumulation and the diagnosis follow each sweep
    assert H.sumflux_state() == (2, 1)
    H.expect("stage_finish", (2, None), OK)
    assert H.fn("sync")(H.h) == OK                                # the fixture destroys the handle
