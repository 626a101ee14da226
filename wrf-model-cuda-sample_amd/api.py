"""advance_mu_t -- Python mirror of the reference routine's interface.

Same name, argument order and meaning as ``SUBROUTINE advance_mu_t``
(module_small_step_em.f90:7-18); ``config_flags`` is anything with
``.periodic_x/.specified/.nested`` (``GridConfig``).  Arrays are updated in place.

* numpy arrays  -> one-shot host drop-in  ``amt_advance_mu_t_f32/_f64``
* torch CUDA tensors -> device-resident drop-in ``amt_advance_mu_t_device_f32/_f64`` on
  ``stream`` (default: torch's current stream), asynchronous.

Arrays are i-fastest: a 3-D field is a C-contiguous array of shape (jdim, kdim, idim)
(= Fortran (ims:ime, kms:kme, jms:jme)), a 2-D field (jdim, idim), a 1-D field (kdim,).
"""
from __future__ import annotations

import ctypes
import threading

import numpy as np

from . import lib as _lib
from .config import flags_as_ints

VARIANT_AUTO, VARIANT_COLUMN, VARIANT_MARCH = 0, 1, 2
LAUNCH_BESIDE_OTHERS = 0x100      # OR into `variant`: another stream's kernels run beside this launch (include/amt_advance_mu_t.h)


def compute_window(config_flags, ids, ide, jds, jde, its, ite, jts, jte, kts, kte):
    """(i_start, i_end, j_start, j_end, k_start, k_end) of module_small_step_em.f90:91-106."""
    L = _lib.load_library()
    out = [ctypes.c_int() for _ in range(6)]
    _lib.check(L.amt_compute_window(*flags_as_ints(config_flags), ids, ide, jds, jde,
                                    its, ite, jts, jte, kts, kte, *[ctypes.byref(o) for o in out]))
    return tuple(o.value for o in out)


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _expected_sizes(ims, ime, jms, jme, kms, kme):
    """Element counts of the 26 array arguments, in argument order (18 before the scalars, 8 after),
    for the memory extents ims:ime, kms:kme, jms:jme (module_small_step_em.f90:30-64)."""
    idim, kdim, jdim = ime - ims + 1, kme - kms + 1, jme - jms + 1
    rank3 = {0, 1, 2, 3, 4, 5, 13, 14, 15, 16}          # ww ww_1 u u_1 v v_1 | t t_1 t_ave ft
    want = [(jdim * kdim * idim) if n in rank3 else (jdim * idim) for n in range(18)]
    return want + [kdim] * 4 + [jdim * idim] * 4


def bind_device_call(ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv, mudf, t, t_1,
                     t_ave, ft, mu_tend, rdx, rdy, dts, epssm, dnw, fnm, fnp, rdnw,
                     msfuy, msfvx_inv, msftx, msfty, config_flags,
                     ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,
                     its, ite, jts, jte, kts, kte, *, stream=None, variant=VARIANT_AUTO):
    """Validate once and return a zero-argument callable that enqueues this device-resident
    advance_mu_t call (same tensors, same bounds) -- for per-sub-step loops, where rebuilding the
    48 ctypes arguments every sweep would make the host the bottleneck."""
    import torch
    L = _lib.load_library()
    arrays = (ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv, mudf, t, t_1, t_ave, ft, mu_tend,
              dnw, fnm, fnp, rdnw, msfuy, msfvx_inv, msftx, msfty)
    dt = ww.dtype
    if dt not in (torch.float32, torch.float64):
        raise TypeError(f"unsupported dtype {dt}")
    # the kernel gets raw pointers: a tensor of another extent (a slab patch bound with the whole
    # domain's bounds, say) would be read or written out of bounds on the device
    for a, n in zip(arrays, _expected_sizes(ims, ime, jms, jme, kms, kme)):
        if not (_is_torch(a) and a.is_cuda and a.dtype == dt and a.is_contiguous() and a.numel() == n):
            raise TypeError("device call needs contiguous CUDA tensors of one dtype and of the memory extents")
    real = ctypes.c_float if dt == torch.float32 else ctypes.c_double
    fn = L.amt_advance_mu_t_device_f32 if dt == torch.float32 else L.amt_advance_mu_t_device_f64
    if stream is None:
        stream = torch.cuda.current_stream(ww.device)
    handle = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
    cargs = ([ctypes.c_void_p(handle), int(variant)]
             + [ctypes.c_void_p(a.data_ptr()) for a in arrays[:18]]
             + [real(float(x)) for x in (rdx, rdy, dts, epssm)]
             + [ctypes.c_void_p(a.data_ptr()) for a in arrays[18:]]
             + list(flags_as_ints(config_flags))
             + [int(x) for x in (ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)])
    device_index = ww.device.index if ww.device.index is not None else torch.cuda.current_device()
    keep = arrays                                   # keeps the tensors alive as long as the closure

    def call():
        if torch.cuda.current_device() != device_index:
            torch.cuda.set_device(device_index)
        status = fn(*cargs)
        if status:
            _lib.check(status)
        return keep is None
    return call


CYCLIC_X, CYCLIC_Y = 1, 2         # enum amt_cyclic_axes


def cyclic_fill(u, u_1, v, v_1, t_1, muu, muv, msfuy, msfvx_inv, config_flags,
                ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,
                its, ite, jts, jte, kts, kte, *, axes=CYCLIC_X | CYCLIC_Y, members=1, stream=None):
    """Refresh the cyclic wrap cells of a patch's (``members`` > 1: a member-stacked ensemble's) torch device tensors in
    place (``amt_cyclic_fill_device_f32/_f64``): column ide <- ids of u, u_1, t_1, muu, msfuy and column ids-1 <- ide-1 of t_1
    (CYCLIC_X), row jde <- jds of v, v_1, t_1, muv, msfvx_inv and row jds-1 <- jde-1 of t_1 (CYCLIC_Y).  Asynchronous on
    ``stream`` (default: torch's current).  Call it in front of ``advance_mu_t`` on the same stream."""
    import torch
    L = _lib.load_library()
    arrays = (u, u_1, v, v_1, t_1, muu, muv, msfuy, msfvx_inv)
    idim, kdim, jdim = ime - ims + 1, kme - kms + 1, jme - jms + 1
    want = [jdim * kdim * idim] * 5 + [jdim * idim] * 4
    dt = t_1.dtype
    if dt not in (torch.float32, torch.float64):
        raise TypeError(f"unsupported dtype {dt}")
    for a, n in zip(arrays, want):
        if not (_is_torch(a) and a.is_cuda and a.dtype == dt and a.is_contiguous() and a.numel() == (-n if n < 0 else n * int(members))):
            raise TypeError("cyclic_fill needs contiguous CUDA tensors of one dtype and of the memory extents")
    if stream is None:
        stream = torch.cuda.current_stream(t_1.device)
    handle = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
    fn = L.amt_cyclic_fill_device_f32 if dt == torch.float32 else L.amt_cyclic_fill_device_f64
    with torch.cuda.device(t_1.device):
        status = fn(ctypes.c_void_p(handle), int(axes), int(members), *[ctypes.c_void_p(a.data_ptr()) for a in arrays],
                    *flags_as_ints(config_flags),
                    *[int(x) for x in (ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)])
    _lib.check(status)


def spec_bdy_update(t, ft, mu, muts, mu_tend, dts, config_flags,
                    ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,
                    its, ite, jts, jte, kts, kte, *, members=1, stream=None):
    """The boundary-zone update of a specified / nested patch's (``members`` > 1: a member-stacked ensemble's) torch device
    tensors in place (``amt_spec_bdy_update_device_f32/_f64``, header section 12): ``t += dts*ft`` (levels kts..kte-1),
    ``mu += dts*mu_tend``, ``muts += dts*mu_tend`` over the tile's cells outside the compute window.  Asynchronous on
    ``stream`` (default: torch's current).  Call it behind ``advance_mu_t`` on the same stream."""
    import torch
    L = _lib.load_library()
    arrays = (t, ft, mu, muts, mu_tend)
    idim, kdim, jdim = ime - ims + 1, kme - kms + 1, jme - jms + 1
    want = [jdim * kdim * idim] * 2 + [jdim * idim] * 3
    dt = t.dtype if _is_torch(t) else None
    if dt not in (torch.float32, torch.float64):
        raise TypeError(f"unsupported dtype {dt}")
    for a, n in zip(arrays, want):
        if not (_is_torch(a) and a.is_cuda and a.dtype == dt and a.is_contiguous() and a.numel() == (-n if n < 0 else n * int(members))):
            raise TypeError("spec_bdy_update needs contiguous CUDA tensors of one dtype and of the memory extents")
    if stream is None:
        stream = torch.cuda.current_stream(t.device)
    handle = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
    real = ctypes.c_float if dt == torch.float32 else ctypes.c_double
    fn = L.amt_spec_bdy_update_device_f32 if dt == torch.float32 else L.amt_spec_bdy_update_device_f64
    with torch.cuda.device(t.device):
        status = fn(ctypes.c_void_p(handle), int(members), *[ctypes.c_void_p(a.data_ptr()) for a in arrays], real(float(dts)),
                    *flags_as_ints(config_flags),
                    *[int(x) for x in (ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)])
    _lib.check(status)


def sumflux(ru_m, rv_m, ww_m, u, v, ww, u_1, v_1, ww_1, muu, muv, msfuy, msfvx_inv, iteration, n_small_steps,
            ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,
            its, ite, jts, jte, kts, kte, *, members=1, stream=None):
    """One accumulation of the acoustic loop's flux averages (``amt_sumflux_device_f32/_f64``, header section 14) on a patch's
    (``members`` > 1: a member-stacked ensemble's) torch device tensors: ``ru_m, rv_m, ww_m`` take ``u, v, ww`` of sub-step
    ``iteration`` of ``n_small_steps``; the last one turns the sums into the averages.  Asynchronous on ``stream`` (default:
    torch's current).  Call it behind ``advance_mu_t`` (and ``spec_bdy_update``) on the same stream."""
    import torch
    L = _lib.load_library()
    arrays = (ru_m, rv_m, ww_m, u, v, ww, u_1, v_1, ww_1, muu, muv, msfuy, msfvx_inv)
    idim, kdim, jdim = ime - ims + 1, kme - kms + 1, jme - jms + 1
    want = [jdim * kdim * idim] * 9 + [jdim * idim] * 4
    dt = ru_m.dtype if _is_torch(ru_m) else None
    if dt not in (torch.float32, torch.float64):
        raise TypeError(f"unsupported dtype {dt}")
    for a, n in zip(arrays, want):
        if not (_is_torch(a) and a.is_cuda and a.dtype == dt and a.is_contiguous() and a.numel() == (-n if n < 0 else n * int(members))):
            raise TypeError("sumflux needs contiguous CUDA tensors of one dtype and of the memory extents")
    if stream is None:
        stream = torch.cuda.current_stream(ru_m.device)
    handle = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
    fn = L.amt_sumflux_device_f32 if dt == torch.float32 else L.amt_sumflux_device_f64
    with torch.cuda.device(ru_m.device):
        status = fn(ctypes.c_void_p(handle), int(members), *[ctypes.c_void_p(a.data_ptr()) for a in arrays],
                    int(iteration), int(n_small_steps),
                    *[int(x) for x in (ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)])
    _lib.check(status)


def _stage_call(what, fn32, fn64, arrays, optional, sizes, members, stream, dtype, middle, bounds):
    """The checks and the call ``stage_prep`` and ``stage_finish`` share: ``arrays`` are torch device tensors or device addresses
    (then ``dtype`` names the element type), an entry of ``optional`` may be None.  ``sizes`` are elements per member; a negative
    one is an array the members share."""
    import torch
    L = _lib.load_library()
    tensors = [a for a in arrays if _is_torch(a)]
    dt = dtype if dtype is not None else tensors[0].dtype if tensors else None
    if dt not in (torch.float32, torch.float64):
        raise TypeError(f"unsupported dtype {dt}")
    for k, (a, n) in enumerate(zip(arrays, sizes)):
        if a is None and k in optional:
            continue
        if _is_torch(a):
            if not (a.is_cuda and a.dtype == dt and a.is_contiguous() and a.numel() == (-n if n < 0 else n * int(members))):
                raise TypeError(f"{what} needs contiguous CUDA tensors of one dtype and of the memory extents")
        elif not isinstance(a, int):
            raise TypeError(f"{what} needs CUDA tensors or device addresses")
    device = tensors[0].device if tensors else torch.device("cuda", torch.cuda.current_device())
    if stream is None:
        stream = torch.cuda.current_stream(device)
    handle = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
    ptrs = [ctypes.c_void_p(None if a is None else a.data_ptr() if _is_torch(a) else a) for a in arrays]
    with torch.cuda.device(device):
        status = (fn32 if dt == torch.float32 else fn64)(ctypes.c_void_p(handle), int(members), *middle(ptrs),
                                                          *[int(x) for x in bounds])
    _lib.check(status)


def stage_prep(t, t_1, t_old, ww, ww_1, mu, mu_old, mu_save, muts, mudf, mut, mub, rk_step,
               ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,
               its, ite, jts, jte, kts, kte, *, members=1, stream=None, dtype=None):
    """small_step_prep of Runge-Kutta step ``rk_step`` (``amt_stage_prep_device_f32/_f64``, header section 15) on a patch's
    (``members`` > 1: a member-stacked ensemble's) torch device tensors or device addresses (then with ``dtype``): the full
    ``t``, ``mu`` become the perturbation form ``advance_mu_t`` works on, ``t_1``, ``ww_1``, ``mu_save`` (and at step 1 ``t_old``,
    ``mu_old``) keep what finish needs, ``muts = mub + mu_old``.  ``mudf`` may be None at ``rk_step`` > 1.  Asynchronous on
    ``stream`` (default: torch's current)."""
    L = _lib.load_library()
    n3, n2 = (jme - jms + 1) * (kme - kms + 1) * (ime - ims + 1), (jme - jms + 1) * (ime - ims + 1)
    _stage_call("stage_prep", L.amt_stage_prep_device_f32, L.amt_stage_prep_device_f64,
                (t, t_1, t_old, ww, ww_1, mu, mu_old, mu_save, muts, mudf, mut, mub), {9} if int(rk_step) > 1 else set(),
                [n3] * 5 + [n2] * 7, members, stream, dtype, lambda p: p + [int(rk_step)],
                (ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte))


def stage_finish(t, t_1, ww, ww_1, mu, mu_save, muts, mut, dts, n_small_steps, h_diabatic,
                 ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,
                 its, ite, jts, jte, kts, kte, *, members=1, stream=None, dtype=None):
    """small_step_finish behind an acoustic loop of ``n_small_steps`` sweeps (``amt_stage_finish_device_f32/_f64``, header
    section 15): ``t = ((t - dts * n * mut * h_diabatic) + t_1 * mut) / muts`` (``h_diabatic`` may be None), ``ww += ww_1``,
    ``mu += mu_save``.  Asynchronous on ``stream`` (default: torch's current)."""
    L = _lib.load_library()
    n3, n2 = (jme - jms + 1) * (kme - kms + 1) * (ime - ims + 1), (jme - jms + 1) * (ime - ims + 1)
    _stage_call("stage_finish", L.amt_stage_finish_device_f32, L.amt_stage_finish_device_f64,
                (t, t_1, ww, ww_1, mu, mu_save, muts, mut, h_diabatic), {8}, [n3] * 4 + [n2] * 4 + [n3], members, stream, dtype,
                lambda p: p[:8] + [float(dts), int(n_small_steps), p[8]],
                (ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte))


def p_rho(mode, step, al, p, ph, pm1, alt, c2a, t, t_old, mu, muts, rdnw, znu, dnw, t0, smdiv,
          ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,
          its, ite, jts, jte, kts, kte, *, members=1, stream=None, dtype=None):
    """calc_p_rho behind acoustic sub-step ``step`` (``amt_p_rho_device_f32/_f64``, header section 16) on a patch's (``members``
    > 1: a member-stacked ensemble's) torch device tensors or device addresses (then with ``dtype``): ``al`` and ``p`` are
    diagnosed from ``t``, ``t_old``, ``mu``, ``muts``; ``mode`` 1 reads ``ph``, ``mode`` 2 integrates it up the column; ``p`` is
    damped against ``pm1`` at ``step`` != 0.  ``rdnw``, ``znu``, ``dnw`` are level arrays the members share.  Asynchronous on
    ``stream`` (default: torch's current)."""
    L = _lib.load_library()
    n3, n2, n1 = (jme - jms + 1) * (kme - kms + 1) * (ime - ims + 1), (jme - jms + 1) * (ime - ims + 1), kme - kms + 1
    arrays = (al, p, ph, pm1, alt, c2a, t, t_old, mu, muts, rdnw, znu, dnw)
    _stage_call("p_rho", L.amt_p_rho_device_f32, L.amt_p_rho_device_f64, arrays, set(),
                [n3] * 8 + [n2] * 2 + [-n1] * 3, members, stream, dtype,
                lambda q: [int(mode), int(step)] + q + [float(t0), float(smdiv)],
                (ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte))


def advance_uv(non_hydrostatic, u, v, ru_tend, rv_tend, p, pb, ph, php, alt, al, mu, muu, muv, mudf, cqu, cqv,
               msfux, msfuy, msfvx, msfvx_inv, msfvy, fnm, fnp, rdnw, rdx, rdy, dts, cf1, cf2, cf3, emdiv,
               periodic_x, specified, nested,
               ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,
               its, ite, jts, jte, kts, kte, *, members=1, stream=None, dtype=None):
    """advance_uv in front of an acoustic sub-step (``amt_advance_uv_device_f32/_f64``, header section 17) on a patch's
    (``members`` > 1: a member-stacked ensemble's) torch device tensors or device addresses (then with ``dtype``): ``u`` and ``v``
    are advanced in place by the horizontal pressure gradient of ``p``, ``al``, ``ph`` against the base state ``pb``, ``alt``,
    ``php`` and by the divergence damping of ``mudf``.  ``fnm``, ``fnp``, ``rdnw`` are level arrays the members share.  The mass
    cells at ``i_start-1`` and ``j_start-1`` are the caller's to fill.  Asynchronous on ``stream`` (default: torch's current)."""
    L = _lib.load_library()
    n3, n2, n1 = (jme - jms + 1) * (kme - kms + 1) * (ime - ims + 1), (jme - jms + 1) * (ime - ims + 1), kme - kms + 1
    arrays = (u, v, ru_tend, rv_tend, p, pb, ph, php, alt, al, mu, muu, muv, mudf, cqu, cqv, msfux, msfuy, msfvx, msfvx_inv, msfvy,
              fnm, fnp, rdnw)
    _stage_call("advance_uv", L.amt_advance_uv_device_f32, L.amt_advance_uv_device_f64, arrays, set(),
                [n3] * 10 + [n2] * 4 + [n3] * 2 + [n2] * 5 + [-n1] * 3, members, stream, dtype,
                lambda q: [int(bool(non_hydrostatic))] + q + [float(x) for x in (rdx, rdy, dts, cf1, cf2, cf3, emdiv)]
                + [int(bool(periodic_x)), int(bool(specified)), int(bool(nested))],
                (ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte))


def advance_mu_t(ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv, mudf, t, t_1,
                 t_ave, ft, mu_tend, rdx, rdy, dts, epssm, dnw, fnm, fnp, rdnw,
                 msfuy, msfvx_inv, msftx, msfty, config_flags,
                 ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,
                 its, ite, jts, jte, kts, kte, *, stream=None, variant=VARIANT_AUTO):
    L = _lib.load_library()
    arrays_a = (ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv, mudf, t, t_1, t_ave, ft, mu_tend)
    arrays_b = (dnw, fnm, fnp, rdnw, msfuy, msfvx_inv, msftx, msfty)
    ints = [int(x) for x in (ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)]
    want = _expected_sizes(ims, ime, jms, jme, kms, kme)
    flags = list(flags_as_ints(config_flags))

    if _is_torch(ww):
        import torch
        dt = ww.dtype
        if dt not in (torch.float32, torch.float64):
            raise TypeError(f"unsupported dtype {dt}")
        for a, n in zip(arrays_a + arrays_b, want):
            if not (_is_torch(a) and a.is_cuda and a.dtype == dt and a.is_contiguous() and a.numel() == n):
                raise TypeError("device call needs contiguous CUDA tensors of one dtype and of the memory extents")
        real = ctypes.c_float if dt == torch.float32 else ctypes.c_double
        if stream is None:
            stream = torch.cuda.current_stream(ww.device)
        handle = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
        fn = L.amt_advance_mu_t_device_f32 if dt == torch.float32 else L.amt_advance_mu_t_device_f64
        with torch.cuda.device(ww.device):
            status = fn(ctypes.c_void_p(handle), int(variant),
                        *[ctypes.c_void_p(a.data_ptr()) for a in arrays_a],
                        *[real(float(s)) for s in (rdx, rdy, dts, epssm)],
                        *[ctypes.c_void_p(a.data_ptr()) for a in arrays_b], *flags, *ints)
        _lib.check(status)
        return

    dt = ww.dtype
    if dt not in (np.float32, np.float64):
        raise TypeError(f"unsupported dtype {dt}")
    for a, n in zip(arrays_a + arrays_b, want):
        if not (isinstance(a, np.ndarray) and a.dtype == dt and a.size == n
                and (a.flags["C_CONTIGUOUS"] or a.flags["F_CONTIGUOUS"])):
            raise TypeError("host call needs contiguous numpy arrays of one dtype and of the memory extents")
    real = ctypes.c_float if dt == np.float32 else ctypes.c_double
    fn = L.amt_advance_mu_t_f32 if dt == np.float32 else L.amt_advance_mu_t_f64
    try:
        status = fn(*[a.ctypes.data_as(ctypes.c_void_p) for a in arrays_a],
                    *[real(float(s)) for s in (rdx, rdy, dts, epssm)],
                    *[a.ctypes.data_as(ctypes.c_void_p) for a in arrays_b], *flags, *ints)
    finally:
        # the library may have flushed deferred outputs into the PREVIOUS call's arrays during this call (other arrays,
        # other extents): those were kept alive until now; from here on it is this call's arrays it remembers
        _remember(arrays_a + arrays_b)
    _lib.check(status)


advance_mu_t.bind = bind_device_call        # SlabStepper pre-marshals its per-sweep launches through this


# Lifetime of host arrays the library remembers.  With the residency cache or deferred outputs on, the library
# keeps the host ADDRESSES of a call's arrays after the call returns: cached inputs are recognised by address, and a deferred
# output is written through its address later (amt_host_fetch, the automatic flush on a key change / release / defer-off, the
# check mode's canaries).  A C or Fortran host owns its arrays for the run; numpy arrays are garbage-collected -- so this
# module holds strong references to the arrays of the calling thread's LAST one-shot call for as long as either mode is on in
# that thread, and drops them when both are off and nothing is stale.
_tl = threading.local()


def _remember(arrays) -> None:
    if getattr(_tl, "cache_on", False) or getattr(_tl, "defer_on", False) or _stale_any():
        _tl.held = tuple(arrays)
    else:
        _tl.held = ()


def _stale_any() -> bool:
    return int(_lib.load_library().amt_host_stale(None)) != 0        # stale, or undefined after a failed call: still remembered


def _forget_if_idle() -> None:
    if not (getattr(_tl, "cache_on", False) or getattr(_tl, "defer_on", False)) and not _stale_any():
        _tl.held = ()


def held_arrays() -> tuple:
    """The host arrays this module keeps alive for the calling thread (see above); () when none."""
    return getattr(_tl, "held", ())


def host_cache_enable(on: bool = True, check: bool = False) -> None:
    """Residency cache of the one-shot (numpy) calls of the calling thread: ww_1, u_1, v_1, t_1, ft stay on the
    device between calls (header section 1: amt_host_cache_enable).  ``check``: the checksum debug mode."""
    L = _lib.load_library()
    _lib.check(L.amt_host_cache_enable(int(bool(on))))
    _lib.check(L.amt_host_cache_check(int(bool(check))))
    _tl.cache_on = bool(on)
    _forget_if_idle()


def host_defer(array=None, on: bool = True) -> None:
    """Deferred outputs of the one-shot (numpy) calls of the calling thread (header section 1: amt_host_defer): the
    output ``array`` (None: all seven) stays on the device after a call until ``host_fetch``.

    Lifetime: the library writes the deferred values through the array's ADDRESS later (fetch, or the automatic flush when
    another set of arrays, ``host_release`` or ``host_defer(..., False)`` comes).  This module keeps the arrays of the calling
    thread's last call alive until then (``held_arrays``); arrays passed to the C-ABI directly must outlive that point."""
    L = _lib.load_library()
    ptr = None if array is None else array.ctypes.data_as(ctypes.c_void_p)
    _lib.check(L.amt_host_defer(ptr, int(bool(on))))        # defer-off fetches what is stale while the arrays are still held
    if array is None:
        _tl.defer_on = bool(on)
    elif on:
        _tl.defer_on = True
    _forget_if_idle()


def host_fetch(array=None) -> None:
    """Bring the window's cells of a deferred output (None: every stale one) down to its host array."""
    L = _lib.load_library()
    ptr = None if array is None else array.ctypes.data_as(ctypes.c_void_p)
    _lib.check(L.amt_host_fetch(ptr))
    _forget_if_idle()


def host_release() -> None:
    """Free the calling thread's device workspace (amt_host_release): stale deferred outputs come down first."""
    _lib.check(_lib.load_library().amt_host_release())
    _forget_if_idle()


def host_set_devices(device_ids=()) -> None:
    """One call, several devices (amt_host_set_devices; the reference's own host call splits j over its GPUs,
    advance_mu_t_no_async.cu:108-162): from now on every one-shot call of this thread fans its tile's rows over these device
    slots -- ids may repeat -- with halo rows from the host arrays; () turns it off."""
    ids = [int(d) for d in device_ids]
    arr = (ctypes.c_int * max(len(ids), 1))(*ids)
    _lib.check(_lib.load_library().amt_host_set_devices(len(ids), arr))


def host_devices():
    """The device slots of the calling thread ([] when its one-shot calls run on the current device only)."""
    arr = (ctypes.c_int * 64)()
    n = int(_lib.load_library().amt_host_devices(arr, 64))
    return [int(arr[k]) for k in range(n)]


def host_stale(array=None) -> bool:
    """Is the device copy of a deferred output (None: of any) newer than the host array?  Raises AmtError when the device
    copy is undefined because a call failed part-way (``host_invalidate`` makes the host array the truth again)."""
    L = _lib.load_library()
    ptr = None if array is None else array.ctypes.data_as(ctypes.c_void_p)
    v = int(L.amt_host_stale(ptr))
    if v < 0:
        raise _lib.AmtError(_lib.ERR_PRECONDITION, "the device copy of a deferred output is undefined since a call failed part-way; "
                                                   "host_invalidate(array) makes the host array the truth again")
    return v > 0


def host_invalidate(array=None) -> None:
    """The host array (numpy) changed since the last call: upload it again.  None: all cached arrays."""
    L = _lib.load_library()
    ptr = None if array is None else array.ctypes.data_as(ctypes.c_void_p)
    _lib.check(L.amt_host_invalidate(ptr))
