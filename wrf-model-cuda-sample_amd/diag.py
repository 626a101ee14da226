"""Statistics and bit comparison of fields that live on the device (include/amt_advance_mu_t.h section 10).

``field_stats(a)`` and ``compare(a, b)`` take torch device tensors in the package's layout -- a rank-3 field of shape
``(jdim, kdim, idim)``, a rank-2 field ``(jdim, idim)``, with ``stacked=True`` one more leading member dimension as in
``ensemble`` -- and return one ``FieldStats`` / ``FieldDiff`` per member, computed by one read of the box on the device
(``amt_stats_device_*`` / ``amt_compare_device_*``).  The call enqueues on ``stream`` (default: torch's current) and waits
for it.

``extents = (ims, ime, jms, jme, kms, kme)`` names the Fortran indices of the tensor's memory (default: zero-based, from the
shape); ``box = (i0, i1, k0, k1, j0, j1)`` is Fortran-inclusive inside them (default: everything; rank 2 ignores the k
entries).  Offsets in the records count elements from the member's base.  Argument errors raise ``AmtError`` with status
ERR_INVALID_ARG before any device call.

``moments(a)`` takes a member-STACKED tensor -- ``(members, jdim, kdim, idim)`` or ``(members, jdim, idim)`` -- and returns the
ensemble mean, sample variance and envelope over the members as device tensors of one member's shape (header section 13,
``amt_moments_device_*``): one streaming pass, asynchronous on ``stream``.
"""
from __future__ import annotations

import ctypes

from . import lib as _lib


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _plan(a, stacked, extents, box):
    """(rank, members, extents, box, suffix) of a call; raises AmtError(ERR_INVALID_ARG) for what the library cannot be asked."""
    if not _is_torch(a):
        raise _lib.AmtError(_lib.ERR_INVALID_ARG, "field statistics need a torch tensor (there is no host path)")
    import torch
    if a.dtype not in (torch.float32, torch.float64):
        raise _lib.AmtError(_lib.ERR_INVALID_ARG, f"unsupported dtype {a.dtype}: float32 or float64")
    rank = a.dim() - (1 if stacked else 0)
    members = int(a.shape[0]) if stacked and a.dim() > 0 else 1
    if rank not in (2, 3):
        raise _lib.AmtError(_lib.ERR_INVALID_ARG, f"a tensor of shape {tuple(a.shape)} is a rank-{rank} field: only rank 2 and 3 have a box")
    if not (a.is_cuda and a.is_contiguous()):
        raise _lib.AmtError(_lib.ERR_INVALID_ARG, "field statistics need a contiguous device tensor (there is no host path)")
    dims = tuple(int(n) for n in a.shape[1 if stacked else 0:])
    jdim, kdim, idim = (dims[0], dims[1], dims[2]) if rank == 3 else (dims[0], 1, dims[1])
    if extents is None:
        extents = (0, idim - 1, 0, jdim - 1, 0, kdim - 1)
    ims, ime, jms, jme, kms, kme = (int(x) for x in extents)
    if (ime - ims + 1, jme - jms + 1) != (idim, jdim) or (rank == 3 and kme - kms + 1 != kdim):
        raise _lib.AmtError(_lib.ERR_INVALID_ARG, f"extents {tuple(extents)} do not describe a tensor of shape {tuple(a.shape)}")
    if box is None:
        box = (ims, ime, kms, kme, jms, jme)
    return rank, members, (ims, ime, jms, jme, kms, kme), tuple(int(x) for x in box), "f64" if a.dtype == torch.float64 else "f32"


def _stream_handle(a, stream):
    import torch
    if stream is None:
        stream = torch.cuda.current_stream(a.device)
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)


def field_stats(a, *, stacked: bool = False, extents=None, box=None, stream=None):
    """One ``FieldStats`` per member (a list) of the box of ``a``."""
    L = _lib.load_library()
    rank, members, ext, bx, sfx = _plan(a, stacked, extents, box)
    out = (_lib.FieldStats * members)()
    fn = getattr(L, f"amt_stats_device_{sfx}")
    import torch
    with torch.cuda.device(a.device):
        _lib.check(fn(ctypes.c_void_p(_stream_handle(a, stream)), ctypes.c_void_p(a.data_ptr()), rank, members, *ext, *bx, out))
    return list(out)


def compare(a, b, *, stacked: bool = False, extents=None, box=None, stream=None):
    """One ``FieldDiff`` per member (a list) of the box of ``a`` against the same box of ``b``."""
    L = _lib.load_library()
    rank, members, ext, bx, sfx = _plan(a, stacked, extents, box)
    if not _is_torch(b) or b.dtype != a.dtype or tuple(b.shape) != tuple(a.shape):
        raise _lib.AmtError(_lib.ERR_INVALID_ARG, "compare needs two tensors of one dtype and shape")
    out = (_lib.FieldDiff * members)()
    fn = getattr(L, f"amt_compare_device_{sfx}")
    if not (b.is_cuda and b.is_contiguous()) or a.device != b.device:
        raise _lib.AmtError(_lib.ERR_INVALID_ARG, "compare needs contiguous tensors on one device")
    import torch
    with torch.cuda.device(a.device):
        _lib.check(fn(ctypes.c_void_p(_stream_handle(a, stream)), ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()),
                      rank, members, *ext, *bx, out))
    return list(out)


MOMENTS = ("mean", "var", "lo", "hi")


def moments_outputs(names, out, shape, dtype, device, alloc_stream_is_call_stream: bool):
    """The four output slots of a moments call: ``(tensors by name, [pointer or None] * 4)``.  A name of ``names`` without a
    tensor in ``out`` gets a zero-filled one (``+0.0`` outside the box); a tensor passed in keeps its cells outside the box."""
    import torch
    out = dict(out or {})
    names = tuple(names) + tuple(k for k in out if k not in names)
    for k in names:
        if k not in MOMENTS:
            raise _lib.AmtError(_lib.ERR_INVALID_ARG, f"unknown moment {k!r}: one of {MOMENTS}")
    res, fresh = {}, False
    for k in MOMENTS:
        if k not in names:
            continue
        t = out.get(k)
        if t is None:
            t = torch.zeros(shape, dtype=dtype, device=device)
            fresh = True
        elif not (_is_torch(t) and t.is_cuda and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == tuple(shape)
                  and t.device == device):
            raise _lib.AmtError(_lib.ERR_INVALID_ARG, f"out[{k!r}]: need a contiguous {dtype} device tensor of shape {tuple(shape)} "
                                                      "on the input's device")
        res[k] = t
    if fresh and not alloc_stream_is_call_stream:
        torch.cuda.current_stream(device).synchronize()       # the zeros are there before another stream writes the box
    return res, [ctypes.c_void_p(res[k].data_ptr()) if k in res else None for k in MOMENTS]


def moments(a, *, extents=None, box=None, stream=None, want=("mean", "var"), out=None):
    """Mean, sample variance, minimum and maximum over the members of the box of the stacked tensor ``a``, cell by cell in member
    order (the definition: header section 13).  Returns a dict name -> tensor for every name of ``want`` and every key of
    ``out``.  A tensor the call allocates is ``+0.0`` outside the box; one passed in through ``out={"mean": t, ...}`` keeps its
    cells outside the box.  Asynchronous on ``stream`` (default: torch's current stream)."""
    L = _lib.load_library()
    rank, members, ext, bx, sfx = _plan(a, True, extents, box)
    import torch
    call_stream = _stream_handle(a, stream)
    same = call_stream == torch.cuda.current_stream(a.device).cuda_stream
    res, ptrs = moments_outputs(want, out, tuple(a.shape[1:]), a.dtype, a.device, same)
    fn = getattr(L, f"amt_moments_device_{sfx}")
    with torch.cuda.device(a.device):
        _lib.check(fn(ctypes.c_void_p(call_stream), ctypes.c_void_p(a.data_ptr()), rank, members, *ext, *bx, *ptrs))
    return res
