"""The cyclic refresh through the one halo mover (csrc/amt_halo.hip; DESIGN.md sections 7.4 and 7.5) at the shapes where its
16-byte decision can go wrong.  The kernel decides per run, on the device, behind the member offset, whether a chunk moves as one
16-byte access; here runs of ONE job start on and off 16-byte boundaries and the members differ in phase:

* memory 37 x 5 x 11 (idim x kdim x jdim), a one-cell halo all round: the fp32 row distance is 148 bytes and the fp32 member
  distance 37 * 5 * 11 * 4 bytes, neither a multiple of 16 (fp64: 296 bytes and 37 * 5 * 11 * 8);
* memory 40 x 5 x 11 with ims = -3: every row run starts 4 elements into a row of 40 and is 32 elements long -- every run
  qualifies for 16-byte accesses in both dtypes and in every member, and its last chunk is whole.

amt_ensemble_cyclic_fill and amt_cyclic_fill_device_* against tests/cyclic_ref.py, all 26 arrays compared WHOLE and bit for bit,
so that a write outside a run shows.  Every element carries a bit pattern of its own (field, index), NaNs with payloads and
signalling NaNs among them: a shifted or duplicated chunk cannot compare equal."""
import numpy as np
import pytest

import cyclic_ref as CR
from conftest import bits_equal

pytestmark = pytest.mark.gpu

X, Y = CR.CYCLIC_X, CR.CYCLIC_Y
NAMES9 = ("u", "u_1", "v", "v_1", "t_1", "muu", "muv", "msfuy", "msfvx_inv")


def _bounds(S, idim):
    if idim == 37:
        b = S.domain_bounds(35, 4, 9)                            # memory 0:36, 1:5, 0:10
    else:
        b = S.domain_bounds(32, 4, 9).replace(ims=-3, ime=36)    # column ids = 1 lies 4 elements into a memory row of 40
    assert (b.idim, b.kdim, b.jdim) == (idim, 5, 11)
    assert b.ids - 1 >= b.ims and b.ide <= b.ime and b.jds - 1 == b.jms and b.jde == b.jme
    return b


def _patterns(S, b, dtype, members):
    """name -> member-stacked array; element e of field f holds a pattern made of (f, e), every third one a quiet NaN with that
    payload, every seventh a negative signalling NaN."""
    wide = np.dtype(dtype).itemsize == 8
    U = np.uint64 if wide else np.uint32
    out = {}
    for f, name in enumerate(S.FIELD_NAMES):
        shape = b.shape(name) if S.field_rank(name) == 1 else (members,) + tuple(b.shape(name))
        e = np.arange(int(np.prod(shape)), dtype=U)
        assert e.size < 1 << 13 and f < 32
        tag = (U(f) << U(13)) | e | U(1 << 19)                   # below 2^20, never zero, one per (field, element)
        if wide:
            bits = np.where(e % U(7) == 0, U(0xfff0000000000000) | tag,
                            np.where(e % U(3) == 0, U(0x7ff8000000000000) | (tag << U(20)), U(0x3000000000000000) | (tag << U(16))))
        else:
            bits = np.where(e % U(7) == 0, U(0xff800000) | tag, np.where(e % U(3) == 0, U(0x7fc00000) | tag, U(0x30000000) | tag))
        assert np.unique(bits).size == bits.size
        out[name] = bits.astype(U).view(dtype).reshape(shape)
    assert np.isnan(out["t_1"]).any() and not np.isnan(out["t_1"]).all()
    return out


_CASES = {}


def _case(S, idim, dtype, members, axes):
    """(inputs, bounds, what the reference makes of them): computed once per case, shared, left unchanged."""
    key = (idim, np.dtype(dtype).name, members, axes)
    if key not in _CASES:
        b = _bounds(S, idim)
        host = _patterns(S, b, dtype, members)
        want = CR.cyclic_fill({n: a.copy() for n, a in host.items()}, b, axes)
        changed = [n for n in S.FIELD_NAMES if not bits_equal(want[n], host[n])]
        assert changed and set(changed) <= set(CR.MAY_CHANGE)
        _CASES[key] = (host, b, want)
    return _CASES[key]


def _to_device(torch, arrays):
    return {n: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for n, a in arrays.items()}


@pytest.mark.parametrize("axes", [X, Y, X | Y], ids=["x", "y", "xy"])
@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("idim", [37, 40], ids=["37x5x11", "40x5x11-aligned"])
def test_refresh_is_bit_exact_and_writes_nothing_else(pkg, idim, dtype, members, axes):
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    S = pkg.synth
    cfg = pkg.GridConfig()
    host, b, want = _case(S, idim, dtype, members, axes)
    es = np.dtype(dtype).itemsize
    if idim == 37 and es == 4:
        assert (b.idim * es) % 16 and (b.idim * b.kdim * b.jdim * es) % 16 and (b.idim * b.jdim * es) % 16
    if idim == 40:
        i0, i1, _, _ = CR.window((0, 0, 0), b)
        assert ((i0 - b.ims) * es) % 16 == 0 and ((i1 - i0 + 1) * es) % 16 == 0 and (b.idim * es) % 16 == 0
    # the pointer level: amt_cyclic_fill_device_f32 / _f64
    dev = _to_device(torch, host)
    assert all(dev[n].data_ptr() % 16 == 0 for n in NAMES9)
    pkg.cyclic_fill(*[dev[n] for n in NAMES9], cfg, *b.as_tuple(), axes=axes, members=members)
    torch.cuda.synchronize()
    for n in S.FIELD_NAMES:
        assert bits_equal(dev[n].cpu().numpy(), want[n]), f"amt_cyclic_fill_device: {n} differs from the reference"
    # the handle: amt_ensemble_cyclic_fill
    dev2 = _to_device(torch, host)
    torch.cuda.synchronize()
    ens = pkg.Ensemble.wrap(dev2, b, cfg, stream=torch.cuda.Stream())
    try:
        ens.cyclic_fill(axes)
        ens.sync()
    finally:
        ens.close()
    for n in S.FIELD_NAMES:
        assert bits_equal(dev2[n].cpu().numpy(), want[n]), f"amt_ensemble_cyclic_fill: {n} differs from the reference"
