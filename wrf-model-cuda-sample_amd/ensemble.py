"""Ensembles: ``members`` patches of one shape advanced by ONE launch per sweep (include/amt_advance_mu_t.h section 8).

Every 3-D and 2-D field carries one more, leading, dimension: torch / numpy shape ``(members, jdim, kdim, idim)`` and
``(members, jdim, idim)`` (Fortran ``u(ims:ime, kms:kme, jms:jme, 1:members)``); the bounds, the flags, the four scalars and
the four 1-D metric arrays ``dnw, fnm, fnp, rdnw`` (shape ``(kdim,)``) are shared.  Each member keeps its own halo rows and
gets the bits the single-patch call gives that member alone.

* ``advance_mu_t_ensemble(...)`` -- the 48 arguments of ``advance_mu_t`` with member-stacked torch device tensors
  (``amt_advance_mu_t_ensemble_device_f32/_f64``), asynchronous on torch's current stream by default.
* ``Ensemble``                   -- the resident handle ``amt_ensemble_*``: library-owned arrays (``Ensemble(...)``) or the
  caller's torch tensors (``Ensemble.wrap(...)``).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import lib as _lib
from . import synth as _S
from .config import GridConfig, flags_as_ints

_NAMES_A = _S.FIELD_NAMES[:18]           # the arrays in front of the scalars
_NAMES_B = _S.FIELD_NAMES[18:]           # dnw fnm fnp rdnw msfuy msfvx_inv msftx msfty


def stacked_shape(b: _S.Bounds, name: str, members: int):
    """Shape of field ``name`` of an ensemble of ``members`` patches of bounds ``b``."""
    s = b.shape(name)
    return s if _S.field_rank(name) == 1 else (int(members),) + tuple(s)


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def validate_stacked(arrays: dict, b: _S.Bounds, members=None) -> int:
    """Checks the 26 member-stacked torch tensors as ``api.bind_device_call`` checks a patch's -- one floating dtype,
    contiguous, exactly the memory extents, every 3-D and 2-D tensor with the same leading member count -- and returns
    that count.  Raises TypeError; needs no device (where the tensors live is the caller's check)."""
    import torch
    ww = arrays["ww"]
    if not _is_torch(ww):
        raise TypeError("an ensemble call needs torch tensors")
    dt = ww.dtype
    if dt not in (torch.float32, torch.float64):
        raise TypeError(f"unsupported dtype {dt}")
    if members is None:
        if ww.dim() != 4:
            raise TypeError(f"ww: expected (members, jdim, kdim, idim), got shape {tuple(ww.shape)}")
        members = int(ww.shape[0])
    members = int(members)
    if members < 1:
        raise TypeError(f"members = {members}: an ensemble has at least one member")
    for name in _S.FIELD_NAMES:
        a = arrays[name]
        if not _is_torch(a):
            raise TypeError(f"{name}: not a torch tensor")
        if a.dtype != dt:
            raise TypeError(f"{name}: dtype {a.dtype}, but ww is {dt} (one dtype per call)")
        want = stacked_shape(b, name, members)
        if tuple(a.shape) != tuple(want):
            if _S.field_rank(name) != 1 and a.dim() == len(want) and tuple(a.shape[1:]) == tuple(want[1:]):
                raise TypeError(f"{name}: {int(a.shape[0])} members, the call has {members}")
            raise TypeError(f"{name}: shape {tuple(a.shape)}, the memory extents need {tuple(want)}")
        if not a.is_contiguous():
            raise TypeError(f"{name}: not contiguous")
    return members


def advance_mu_t_ensemble(ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv, mudf, t, t_1,
                          t_ave, ft, mu_tend, rdx, rdy, dts, epssm, dnw, fnm, fnp, rdnw,
                          msfuy, msfvx_inv, msftx, msfty, config_flags,
                          ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,
                          its, ite, jts, jte, kts, kte, *, members=None, stream=None, variant=0):
    """advance_mu_t over every member of an ensemble in one launch; the tensors are updated in place.  ``members`` defaults
    to the leading extent of ``ww``."""
    import torch
    arrays = dict(zip(_NAMES_A + _NAMES_B, (ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv, mudf, t, t_1, t_ave, ft,
                                            mu_tend, dnw, fnm, fnp, rdnw, msfuy, msfvx_inv, msftx, msfty)))
    b = _S.Bounds(*[int(x) for x in (ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)])
    members = validate_stacked(arrays, b, members)
    for name, a in arrays.items():
        if not a.is_cuda or a.device != ww.device:
            raise TypeError(f"{name}: an ensemble call needs device tensors of one device (there is no CPU path)")
    L = _lib.load_library()
    dt = ww.dtype
    real = ctypes.c_float if dt == torch.float32 else ctypes.c_double
    fn = L.amt_advance_mu_t_ensemble_device_f32 if dt == torch.float32 else L.amt_advance_mu_t_ensemble_device_f64
    if stream is None:
        stream = torch.cuda.current_stream(ww.device)
    handle = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
    with torch.cuda.device(ww.device):
        status = fn(ctypes.c_void_p(handle), int(variant), members,
                    *[ctypes.c_void_p(arrays[n].data_ptr()) for n in _NAMES_A],
                    *[real(float(s)) for s in (rdx, rdy, dts, epssm)],
                    *[ctypes.c_void_p(arrays[n].data_ptr()) for n in _NAMES_B],
                    *flags_as_ints(config_flags), *b.as_tuple())
    _lib.check(status)


class Ensemble(_lib.ResidentHandle):
    """Resident ensemble handle (``amt_ensemble_*``).  ``Ensemble(b, members, ...)`` lets the library allocate the stacked
    arrays on the current device; ``Ensemble.wrap(arrays, b, ...)`` steps the caller's torch tensors in place."""

    _PREFIX = "amt_ensemble"

    def _members(self) -> int:
        return self.members

    def __init__(self, b: _S.Bounds, members: int, config: GridConfig = GridConfig(), dtype=np.float64, *,
                 _fields=None, _stream=None, _keep=None):
        self.L = _lib.load_library()
        self.bounds, self.config, self.dtype = b, config, np.dtype(dtype)
        self.handle = ctypes.c_void_p()
        self._keep = _keep                       # wrapped tensors stay alive as long as the handle
        head = (ctypes.byref(self.handle), int(members), self.dtype.itemsize, *flags_as_ints(config), *b.as_tuple())
        if _fields is None:
            _lib.check(self.L.amt_ensemble_create(*head))
        else:
            ptrs = (ctypes.c_void_p * len(_fields))(*_fields)
            _lib.check(self.L.amt_ensemble_wrap(*head, ptrs, ctypes.c_void_p(_stream)))
        self.members = int(self.L.amt_ensemble_members(self.handle))

    @classmethod
    def wrap(cls, arrays: dict, b: _S.Bounds, config: GridConfig = GridConfig(), *, stream=None) -> "Ensemble":
        """Over member-stacked torch device tensors (``arrays``: field name -> tensor), on ``stream`` (default: torch's current).
        As with ``amt_domain_wrap``, the NULL stream is not adopted: when torch's current stream is the default stream the handle
        works on a stream of its own, and the caller orders it against torch's work with ``sync()``."""
        import torch
        members = validate_stacked(arrays, b)
        ww = arrays["ww"]
        for name in _S.FIELD_NAMES:
            if not arrays[name].is_cuda or arrays[name].device != ww.device:
                raise TypeError(f"{name}: Ensemble.wrap needs device tensors of one device")
        if stream is None:
            stream = torch.cuda.current_stream(ww.device)
        handle = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
        with torch.cuda.device(ww.device):
            return cls(b, members, config, np.float64 if ww.dtype == torch.float64 else np.float32,
                       _fields=[arrays[n].data_ptr() for n in _S.FIELD_NAMES], _stream=handle,
                       _keep=(dict(arrays), stream))

    def _host(self, name: str, a) -> np.ndarray:
        if not (isinstance(a, np.ndarray) and a.dtype == self.dtype and a.flags["C_CONTIGUOUS"]
                and tuple(a.shape) == tuple(self.bounds.shape(name))):
            raise TypeError(f"{name}: need a C-contiguous {self.dtype} array of shape {self.bounds.shape(name)} (ONE member)")
        return a

    def upload_member(self, name: str, member: int, host: np.ndarray) -> None:
        a = self._host(name, host)
        _lib.check(self.L.amt_ensemble_upload_member(self.handle, _S.FIELD_ID[name], int(member), a.ctypes.data_as(ctypes.c_void_p)))

    def download_member(self, name: str, member: int, out: np.ndarray = None) -> np.ndarray:
        a = np.empty(self.bounds.shape(name), self.dtype) if out is None else self._host(name, out)
        _lib.check(self.L.amt_ensemble_download_member(self.handle, _S.FIELD_ID[name], int(member), a.ctypes.data_as(ctypes.c_void_p)))
        return a

    def upload_patch(self, member: int, patch: _S.Patch) -> None:
        """All 26 fields of a host patch into member ``member`` (the 1-D fields are shared: the last upload stays)."""
        for name in _S.FIELD_NAMES:
            self.upload_member(name, member, patch.arrays[name])
        self.set_scalars(patch.rdx, patch.rdy, patch.dts, patch.epssm)

    def download_patch(self, member: int) -> dict:
        return {name: self.download_member(name, member) for name in _S.FIELD_NAMES}

    def fill_synthetic(self, seed: int, global_dims=None) -> None:
        """Member m as ``synth.make_patch(bounds, seed=seed + m)`` fills a single patch."""
        b = self.bounds
        gni, gnk, gnj = global_dims or (b.ide - b.ids, b.kde - 1, b.jde - b.jds)
        _lib.check(self.L.amt_ensemble_fill_synthetic(self.handle, ctypes.c_uint64(int(seed)), b.ims, b.kms - 1, b.jms,
                                                      gni + 2, gnk + 1, gnj + 2))

    def moments(self, field, region="window", want=("mean", "var"), out=None) -> dict:
        """``amt_ensemble_moments``: mean, sample variance, minimum and maximum over the members of ``field`` (a name or an
        ``amt_field`` id, rank 2 or 3) over ``region`` ("window" / "memory" or REGION_*), as torch tensors of ONE member's shape
        on the current device.  Returns a dict name -> tensor for every name of ``want`` and every key of ``out``; a tensor the
        call allocates is ``+0.0`` outside the region, one passed in through ``out`` keeps its cells there.  Enqueued on the
        handle's stream behind its stepping; ``sync()`` waits for it."""
        import torch
        from . import diag as _diag
        name = field if isinstance(field, str) else _S.FIELD_NAMES[int(field)]
        region = {"window": _lib.REGION_WINDOW, "memory": _lib.REGION_MEMORY}.get(region, region)
        dt = torch.float64 if self.dtype == np.float64 else torch.float32
        dev = torch.device("cuda", torch.cuda.current_device())
        same = self.stream == torch.cuda.current_stream(dev).cuda_stream
        res, ptrs = _diag.moments_outputs(want, out, tuple(self.bounds.shape(name)), dt, dev, same)
        _lib.check(self.L.amt_ensemble_moments(self.handle, _S.FIELD_ID[name], int(region), *ptrs))
        return res

    def close(self) -> None:
        super().close()
        self._keep = None
