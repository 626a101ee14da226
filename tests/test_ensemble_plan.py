"""Host logic of the ensemble path (include/amt_advance_mu_t.h section 8), no GPU needed: the launch plan for `members`
patches stepped as one launch (amt_march_rows_for_members), the Python argument validation of advance_mu_t_ensemble, and the
absence of any CPU fall-back behind the new entry points."""
import ctypes

import numpy as np
import pytest

import cases

MAX_ROWS = 1 << 20          # 32-bit row offsets never bind at these sizes


def _cost(ntile_cols, nj, cus, r):
    """The launcher's own cost model (DESIGN.md section 4.2 "Launch plan"): rounds(r) * (r + 0.5) row-times."""
    blocks = ntile_cols * -(-nj // r)
    return -(-blocks // cus) * (r + 0.5)


def test_one_member_plans_like_a_single_patch(pkg):
    L = pkg.load_library()
    for ntile in (1, 2, 3, 4, 8, 9, 17, 64, 65, 129):
        for nj in (1, 2, 7, 64, 127, 128, 510, 1024):
            for cus in (1, 64, 104, 256, 304):
                for wbytes, hl in ((8, 1), (8, 2), (4, 1), (4, 4)):
                    for max_rows in (3, 40, MAX_ROWS):
                        want = L.amt_march_rows_for(ntile, nj, cus, max_rows, wbytes, hl)
                        got = L.amt_march_rows_for_members(ntile, 1, nj, cus, max_rows, wbytes, hl)
                        assert got == want, (ntile, nj, cus, wbytes, hl, max_rows, got, want)


def test_nothing_to_plan(pkg):
    L = pkg.load_library()
    assert L.amt_march_rows_for_members(2, 0, 128, 256, MAX_ROWS, 8, 1) == 0
    assert L.amt_march_rows_for_members(2, -3, 128, 256, MAX_ROWS, 8, 1) == 0
    assert L.amt_march_rows_for_members(0, 4, 128, 256, MAX_ROWS, 8, 1) == 0
    assert L.amt_march_rows_for_members(2, 4, 0, 256, MAX_ROWS, 8, 1) == 0


def test_32_members_of_128x128_get_long_blocks(pkg):
    """256 compute units, fp64, one level group: 2 tile columns x 128 rows.  Alone the patch is cut into one-row blocks
    (cost 1.5 per row of work); 32 of them as one launch get many-row blocks and a lower modelled cost per member."""
    L = pkg.load_library()
    ntile, nj, cus, members = 2, 128, 256, 32
    r1 = L.amt_march_rows_for(ntile, nj, cus, MAX_ROWS, 8, 1)
    rm = L.amt_march_rows_for_members(ntile, members, nj, cus, MAX_ROWS, 8, 1)
    assert rm > 1 and rm > r1
    alone = _cost(ntile, nj, cus, r1)                              # one member, its own launch
    batched = _cost(ntile * members, nj, cus, rm) / members        # its share of the one launch
    print(f"rows per block: alone {r1}, batched {rm}; modelled row-times per member: alone {alone}, batched {batched:.3f}, "
          f"ratio {alone / batched:.3f}")
    assert batched < alone
    # the batch is never planned worse than the single patch's own rows would do in the batch
    assert _cost(ntile * members, nj, cus, rm) <= _cost(ntile * members, nj, cus, r1)


def test_a_block_never_spans_two_members(pkg):
    L = pkg.load_library()
    for ntile in (1, 2, 5, 64):
        for members in (1, 2, 5, 32, 37, 400):
            for nj in (1, 2, 3, 11, 60, 128, 509):
                for cus in (8, 256):
                    for wbytes, hl in ((8, 1), (8, 4), (4, 2)):
                        for max_rows in (1, 5, MAX_ROWS):
                            r = L.amt_march_rows_for_members(ntile, members, nj, cus, max_rows, wbytes, hl)
                            assert 1 <= r <= nj and r <= max_rows, (ntile, members, nj, cus, wbytes, hl, max_rows, r)
                            if wbytes == 8 and hl >= 2:
                                assert r <= 64          # the fp64 level-group shapes keep their cap


# ---------------------------------------------------------------------------------------------
# Python argument validation: CPU tensors are enough to reach every check
# ---------------------------------------------------------------------------------------------
def _stacked(pkg, members, dtype=np.float64, dims=(12, 5, 6)):
    import torch
    E = pkg.ensemble
    b = pkg.synth.domain_bounds(*dims)
    tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    arrays = {n: torch.zeros(E.stacked_shape(b, n, members), dtype=tdt) for n in pkg.synth.FIELD_NAMES}
    return b, arrays


def _call(pkg, b, arrays, **kw):
    a = arrays
    return pkg.advance_mu_t_ensemble(
        a["ww"], a["ww_1"], a["u"], a["u_1"], a["v"], a["v_1"], a["mu"], a["mut"], a["muave"], a["muts"], a["muu"], a["muv"],
        a["mudf"], a["t"], a["t_1"], a["t_ave"], a["ft"], a["mu_tend"], 1e-3, 1e-3, 2.0, 0.1, a["dnw"], a["fnm"], a["fnp"],
        a["rdnw"], a["msfuy"], a["msfvx_inv"], a["msftx"], a["msfty"], pkg.GridConfig(), *b.as_tuple(), **kw)


def test_stacked_shapes(pkg):
    b = pkg.synth.domain_bounds(12, 5, 6)
    E = pkg.ensemble
    assert E.stacked_shape(b, "t", 3) == (3, b.jdim, b.kdim, b.idim)
    assert E.stacked_shape(b, "mu", 3) == (3, b.jdim, b.idim)
    assert E.stacked_shape(b, "dnw", 3) == (b.kdim,)


def test_validation_accepts_a_well_formed_ensemble(pkg):
    b, arrays = _stacked(pkg, 3)
    assert pkg.ensemble.validate_stacked(arrays, b) == 3
    assert pkg.ensemble.validate_stacked(arrays, b, 3) == 3


def test_wrong_member_count_in_one_tensor(pkg):
    import torch
    b, arrays = _stacked(pkg, 3)
    arrays["v_1"] = torch.zeros(pkg.ensemble.stacked_shape(b, "v_1", 2), dtype=torch.float64)
    with pytest.raises(TypeError, match="v_1: 2 members"):
        _call(pkg, b, arrays)
    b, arrays = _stacked(pkg, 3)
    arrays["muts"] = torch.zeros(pkg.ensemble.stacked_shape(b, "muts", 4), dtype=torch.float64)
    with pytest.raises(TypeError, match="muts: 4 members"):
        _call(pkg, b, arrays)
    b, arrays = _stacked(pkg, 3)
    with pytest.raises(TypeError, match="members"):
        _call(pkg, b, arrays, members=2)                # the tensors hold 3


def test_wrong_extents(pkg):
    import torch
    b, arrays = _stacked(pkg, 2)
    arrays["t"] = torch.zeros((2, b.jdim, b.kdim, b.idim + 1), dtype=torch.float64)
    with pytest.raises(TypeError, match="t: shape"):
        _call(pkg, b, arrays)
    b, arrays = _stacked(pkg, 2)
    arrays["dnw"] = torch.zeros((2, b.kdim), dtype=torch.float64)         # the 1-D metrics are shared, not stacked
    with pytest.raises(TypeError, match="dnw: shape"):
        _call(pkg, b, arrays)
    b, arrays = _stacked(pkg, 2)
    arrays["u"] = arrays["u"].reshape(2 * b.jdim, b.kdim, b.idim)         # a single taller patch is not an ensemble
    with pytest.raises(TypeError, match="u: shape"):
        _call(pkg, b, arrays)
    b, arrays = _stacked(pkg, 2)
    arrays["mu"] = torch.zeros((2, b.jdim, 2 * b.idim), dtype=torch.float64)[..., ::2]      # right shape, not contiguous
    with pytest.raises(TypeError, match="mu: not contiguous"):
        _call(pkg, b, arrays)


def test_mixed_dtypes(pkg):
    b, arrays = _stacked(pkg, 2)
    arrays["ft"] = arrays["ft"].float()
    with pytest.raises(TypeError, match="ft: dtype"):
        _call(pkg, b, arrays)
    b, arrays = _stacked(pkg, 2)
    arrays = {n: a.to(dtype=__import__("torch").float16) for n, a in arrays.items()}
    with pytest.raises(TypeError, match="unsupported dtype"):
        _call(pkg, b, arrays)


def test_host_tensors_are_refused_not_computed(pkg):
    """There is no CPU path: well-formed HOST tensors are a TypeError and stay as they were."""
    b, arrays = _stacked(pkg, 2)
    with pytest.raises(TypeError, match="device tensors"):
        _call(pkg, b, arrays)
    assert all(float(a.abs().sum()) == 0.0 for a in arrays.values())


# ---------------------------------------------------------------------------------------------
# no fall-back without a device
# ---------------------------------------------------------------------------------------------
def test_no_cpu_fallback_without_a_device(pkg):
    L = pkg.load_library()
    if L.amt_device_count() > 0:
        pytest.skip("a device is present")
    members = 3
    patches = [cases.make_case(pkg, "16x8x16", "none", np.float64, seed=40 + m) for m in range(members)]
    b = patches[0].bounds
    S = pkg.synth
    stacked = {n: (patches[0].arrays[n].copy() if S.field_rank(n) == 1 else np.stack([p.arrays[n] for p in patches]))
               for n in S.FIELD_NAMES}
    before = {n: a.copy() for n, a in stacked.items()}
    ptr = lambda n: stacked[n].ctypes.data_as(ctypes.c_void_p)
    st = L.amt_advance_mu_t_ensemble_device_f64(
        None, 0, members, *[ptr(n) for n in S.FIELD_NAMES[:18]], *[ctypes.c_double(x) for x in (S.RDX, S.RDY, S.DTS, S.EPSSM)],
        *[ptr(n) for n in S.FIELD_NAMES[18:]], 0, 0, 0, *b.as_tuple())
    assert st in (1, 4), (st, L.amt_last_error())
    for n in S.FIELD_NAMES:
        assert np.array_equal(stacked[n], before[n]), n
    h = ctypes.c_void_p()
    st = L.amt_ensemble_create(ctypes.byref(h), members, 8, 0, 0, 0, *b.as_tuple())
    assert st in (1, 4) and not h.value
    fields = (ctypes.c_void_p * len(S.FIELD_NAMES))(*[stacked[n].ctypes.data for n in S.FIELD_NAMES])
    st = L.amt_ensemble_wrap(ctypes.byref(h), members, 8, 0, 0, 0, *b.as_tuple(), fields, None)
    assert st in (1, 4) and not h.value
    with pytest.raises(pkg.AmtError) as e:
        pkg.Ensemble(b, members)
    assert e.value.status in (1, 4)


def test_bad_member_counts_are_invalid_arguments(pkg):
    """members < 1 is AMT_ERR_INVALID_ARG before anything touches a device."""
    L = pkg.load_library()
    b = pkg.synth.domain_bounds(16, 8, 16)
    h = ctypes.c_void_p()
    for members in (0, -1):
        assert L.amt_ensemble_create(ctypes.byref(h), members, 8, 0, 0, 0, *b.as_tuple()) == 3 and not h.value
        st = L.amt_advance_mu_t_ensemble_device_f32(
            None, 0, members, *[None] * 18, *[ctypes.c_float(1.0)] * 4, *[None] * 8, 0, 0, 0, *b.as_tuple())
        assert st == 3, st
    assert L.amt_ensemble_members(None) == 0
