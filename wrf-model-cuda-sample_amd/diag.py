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
