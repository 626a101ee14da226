"""ctypes binding of the C-ABI declared in include/amt_advance_mu_t.h.

This is the "reference-side binding" a Python host would add (INTEGRATION.md shows the
Fortran ISO_C_BINDING and C ones).  Loading fails loudly when the HIP library has not
been built -- there is no fallback implementation.
"""
from __future__ import annotations

import ctypes
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
_LIB_NAME = "libamt_advance_mu_t.so"

# status codes of include/amt_advance_mu_t.h
OK, ERR_HIP, ERR_PRECONDITION, ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_ALLOC, ERR_COMM, ERR_NONFINITE = range(8)

REGION_WINDOW, REGION_MEMORY = 0, 1       # enum amt_region


class AmtError(RuntimeError):
    """``report``: the handle's ``GuardReport`` when the status is ERR_NONFINITE and a handle method raised it, else None."""

    def __init__(self, status: int, message: str, report=None):
        super().__init__(f"amt status {status}: {message}")
        self.status = status
        self.report = report


class _Record(ctypes.Structure):
    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={v!r}' for k, v in self.as_dict().items())})"


class FieldStats(_Record):
    """``amt_field_stats``"""
    _fields_ = [("count", ctypes.c_int64), ("n_nan", ctypes.c_int64), ("n_inf", ctypes.c_int64),
                ("first_nonfinite", ctypes.c_int64), ("min", ctypes.c_double), ("max", ctypes.c_double),
                ("max_abs", ctypes.c_double), ("sum", ctypes.c_double)]


class FieldDiff(_Record):
    """``amt_field_diff``"""
    _fields_ = [("count", ctypes.c_int64), ("n_diff", ctypes.c_int64), ("first_diff", ctypes.c_int64),
                ("max_abs_diff", ctypes.c_double)]


class GuardReport(_Record):
    """``amt_guard_report``"""
    _fields_ = [("sweeps_checked", ctypes.c_int64), ("sweep", ctypes.c_int64), ("field", ctypes.c_int32),
                ("member", ctypes.c_int32), ("offset", ctypes.c_int64), ("n_nonfinite", ctypes.c_int64)]


class HaloMessage(_Record):
    """``amt_halo_message`` (header section 11)"""
    _fields_ = [("side", ctypes.c_int), ("peer", ctypes.c_int), ("send", ctypes.c_void_p), ("send_bytes", ctypes.c_size_t),
                ("recv", ctypes.c_void_p), ("recv_bytes", ctypes.c_size_t), ("on_host", ctypes.c_int)]


def library_path() -> Path:
    """The in-tree HIP library; AMT_LIBRARY overrides it (A/B builds of the kernels)."""
    import os
    override = os.environ.get("AMT_LIBRARY")
    return Path(override) if override else PKG_DIR / _LIB_NAME


_lib = None

_P = ctypes.c_void_p
_I = ctypes.c_int
_L = ctypes.c_long


def _adv_sig(real, device: bool, ensemble: bool = False):
    head = ([_P, _I] if device else []) + ([_I] if ensemble else [])      # stream, variant[, members]
    return head + [_P] * 18 + [real] * 4 + [_P] * 8 + [_I] * (3 + 17)


# every symbol include/amt_advance_mu_t.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "amt_version": (ctypes.c_char_p, []),
    "amt_status_string": (ctypes.c_char_p, [_I]),
    "amt_last_error": (ctypes.c_char_p, []),
    "amt_device_count": (_I, []),
    "amt_advance_mu_t_f32": (_I, _adv_sig(ctypes.c_float, False)),
    "amt_advance_mu_t_f64": (_I, _adv_sig(ctypes.c_double, False)),
    "amt_advance_mu_t_device_f32": (_I, _adv_sig(ctypes.c_float, True)),
    "amt_advance_mu_t_device_f64": (_I, _adv_sig(ctypes.c_double, True)),
    "amt_compute_window": (_I, [_I] * 13 + [ctypes.POINTER(_I)] * 6),
    "amt_domain_create": (_I, [ctypes.POINTER(_P), _I] + [_I] * 20),
    "amt_domain_wrap": (_I, [ctypes.POINTER(_P), _I] + [_I] * 20 + [ctypes.POINTER(_P), _P]),
    "amt_domain_destroy": (_I, [_P]),
    "amt_domain_set_scalars": (_I, [_P] + [ctypes.c_double] * 4),
    "amt_domain_set_variant": (_I, [_P, _I]),
    "amt_domain_upload": (_I, [_P, _I, _P]),
    "amt_domain_download": (_I, [_P, _I, _P]),
    "amt_domain_upload_rows": (_I, [_P, _I, _I, _I, _P]),
    "amt_domain_download_rows": (_I, [_P, _I, _I, _I, _P]),
    "amt_domain_fill_synthetic": (_I, [_P, ctypes.c_uint64] + [_L] * 6),
    "amt_domain_fill_fields": (_I, [_P, ctypes.c_uint64, ctypes.c_uint64] + [_L] * 6),
    "amt_domain_poison_halos": (_I, [_P, _I]),
    "amt_domain_step": (_I, [_P, _I]),
    "amt_domain_tune_placement": (_I, [_P, _I, ctypes.POINTER(ctypes.c_float)]),
    "amt_domain_placement": (_I, [_P, ctypes.POINTER(ctypes.c_float), _I]),
    "amt_domain_step_timed": (_I, [_P, _I, ctypes.POINTER(ctypes.c_float)]),
    "amt_domain_sync": (_I, [_P]),
    "amt_domain_field_ptr": (_P, [_P, _I]),
    "amt_domain_stream": (_P, [_P]),
    "amt_synth_fill_host": (_I, [_I, _I, _P, ctypes.c_uint64] + [_L] * 9),
    "amt_synth_fill_device": (_I, [_P, _I, _I, _P, ctypes.c_uint64] + [_L] * 9),
    "amt_calib_stream_copy": (_I, [_P, _P, _P, ctypes.c_size_t, _I]),
    "amt_calib_stream_rate": (_I, [_P, _P, _P, ctypes.c_size_t, _I]),
    "amt_host_pin": (_I, [_P, ctypes.c_size_t]),
    "amt_host_unpin": (_I, [_P]),
    "amt_host_release": (_I, []),
    "amt_host_set_devices": (_I, [_I, ctypes.POINTER(_I)]),
    "amt_host_devices": (_I, [ctypes.POINTER(_I), _I]),
    "amt_host_cache_enable": (_I, [_I]),
    "amt_host_cache_check": (_I, [_I]),
    "amt_host_invalidate": (_I, [_P]),
    "amt_host_defer": (_I, [_P, _I]),
    "amt_host_fetch": (_I, [_P]),
    "amt_host_stale": (_I, [_P]),
    "amt_set_device": (_I, [_I]),
    "amt_comm_unique_id": (_I, [_P]),
    "amt_comm_rendezvous_file": (_I, [ctypes.c_char_p, ctypes.c_uint64, _I, _I, ctypes.c_double, _P]),
    "amt_comm_launch_nonce": (ctypes.c_uint64, []),
    "amt_slab_create": (_I, [ctypes.POINTER(_P), _P, _I, _I, _P, _I]),
    "amt_slab_destroy": (_I, [_P]),
    "amt_slab_exchange": (_I, [_P]),
    "amt_slab_step": (_I, [_P, _I]),
    "amt_slab_step_timed": (_I, [_P, _I, ctypes.POINTER(ctypes.c_float)]),
    "amt_slab_sync": (_I, [_P]),
    "amt_slab_transport": (ctypes.c_char_p, [_P]),
    "amt_slab_pull_mode": (ctypes.c_char_p, [_P]),
    "amt_slab_set_skew_us": (_I, [_P, _I]),
    "amt_slab_halo_bytes": (_L, [_P]),
    "amt_slab_comm_info": (_I, [_P, ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "amt_slab_barrier": (_I, [_P]),
    "amt_slab_max": (_I, [_P, ctypes.POINTER(ctypes.c_double)]),
    "amt_grid_create": (_I, [ctypes.POINTER(_P), _P, _I, _I, _I, _I, _P, _I]),
    "amt_grid_destroy": (_I, [_P]),
    "amt_grid_exchange": (_I, [_P]),
    "amt_grid_step": (_I, [_P, _I]),
    "amt_grid_step_timed": (_I, [_P, _I, ctypes.POINTER(ctypes.c_float)]),
    "amt_grid_sync": (_I, [_P]),
    "amt_grid_set_skew_us": (_I, [_P, _I]),
    "amt_grid_halo_bytes": (_L, [_P]),
    "amt_grid_transport": (ctypes.c_char_p, [_P]),
    "amt_grid_pull_mode": (ctypes.c_char_p, [_P]),
    "amt_grid_comm_info": (_I, [_P, ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "amt_grid_barrier": (_I, [_P]),
    "amt_grid_max": (_I, [_P, ctypes.POINTER(ctypes.c_double)]),
    "amt_advance_mu_t_ensemble_device_f32": (_I, _adv_sig(ctypes.c_float, True, ensemble=True)),
    "amt_advance_mu_t_ensemble_device_f64": (_I, _adv_sig(ctypes.c_double, True, ensemble=True)),
    "amt_ensemble_create": (_I, [ctypes.POINTER(_P), _I, _I] + [_I] * 20),
    "amt_ensemble_wrap": (_I, [ctypes.POINTER(_P), _I, _I] + [_I] * 20 + [ctypes.POINTER(_P), _P]),
    "amt_ensemble_destroy": (_I, [_P]),
    "amt_ensemble_set_scalars": (_I, [_P] + [ctypes.c_double] * 4),
    "amt_ensemble_set_variant": (_I, [_P, _I]),
    "amt_ensemble_members": (_I, [_P]),
    "amt_ensemble_upload_member": (_I, [_P, _I, _I, _P]),
    "amt_ensemble_download_member": (_I, [_P, _I, _I, _P]),
    "amt_ensemble_fill_synthetic": (_I, [_P, ctypes.c_uint64] + [_L] * 6),
    "amt_ensemble_step": (_I, [_P, _I]),
    "amt_ensemble_step_timed": (_I, [_P, _I, ctypes.POINTER(ctypes.c_float)]),
    "amt_ensemble_sync": (_I, [_P]),
    "amt_ensemble_field_ptr": (_P, [_P, _I]),
    "amt_ensemble_stream": (_P, [_P]),
    "amt_march_rows_for_members": (_I, [ctypes.c_long, _I, _I, _I, ctypes.c_long, _I, _I]),
    "amt_cyclic_fill_device_f32": (_I, [_P, _I, _I] + [_P] * 9 + [_I] * (3 + 17)),
    "amt_cyclic_fill_device_f64": (_I, [_P, _I, _I] + [_P] * 9 + [_I] * (3 + 17)),
    "amt_domain_cyclic_fill": (_I, [_P, _I]),
    "amt_domain_set_cyclic": (_I, [_P, _I]),
    "amt_domain_cyclic": (_I, [_P]),
    "amt_ensemble_cyclic_fill": (_I, [_P, _I]),
    "amt_ensemble_set_cyclic": (_I, [_P, _I]),
    "amt_ensemble_cyclic": (_I, [_P]),
    "amt_spec_bdy_update_device_f32": (_I, [_P, _I] + [_P] * 5 + [ctypes.c_float] + [_I] * (3 + 17)),
    "amt_spec_bdy_update_device_f64": (_I, [_P, _I] + [_P] * 5 + [ctypes.c_double] + [_I] * (3 + 17)),
    "amt_domain_spec_bdy_update": (_I, [_P]),
    "amt_domain_set_spec_bdy": (_I, [_P, _I]),
    "amt_domain_spec_bdy": (_I, [_P]),
    "amt_ensemble_spec_bdy_update": (_I, [_P]),
    "amt_ensemble_set_spec_bdy": (_I, [_P, _I]),
    "amt_ensemble_spec_bdy": (_I, [_P]),
    "amt_stats_device_f32": (_I, [_P, _P, _I, _I] + [_I] * 12 + [ctypes.POINTER(FieldStats)]),
    "amt_stats_device_f64": (_I, [_P, _P, _I, _I] + [_I] * 12 + [ctypes.POINTER(FieldStats)]),
    "amt_compare_device_f32": (_I, [_P, _P, _P, _I, _I] + [_I] * 12 + [ctypes.POINTER(FieldDiff)]),
    "amt_compare_device_f64": (_I, [_P, _P, _P, _I, _I] + [_I] * 12 + [ctypes.POINTER(FieldDiff)]),
    "amt_domain_field_stats": (_I, [_P, _I, _I, ctypes.POINTER(FieldStats)]),
    "amt_ensemble_field_stats": (_I, [_P, _I, _I, ctypes.POINTER(FieldStats)]),
    "amt_domain_compare": (_I, [_P, _P, _I, _I, ctypes.POINTER(FieldDiff)]),
    "amt_ensemble_compare": (_I, [_P, _P, _I, _I, ctypes.POINTER(FieldDiff)]),
    "amt_domain_set_guard": (_I, [_P, _I]),
    "amt_ensemble_set_guard": (_I, [_P, _I]),
    "amt_domain_guard_report": (_I, [_P, ctypes.POINTER(GuardReport)]),
    "amt_ensemble_guard_report": (_I, [_P, ctypes.POINTER(GuardReport)]),
    "amt_moments_device_f32": (_I, [_P, _P, _I, _I] + [_I] * 12 + [_P] * 4),
    "amt_moments_device_f64": (_I, [_P, _P, _I, _I] + [_I] * 12 + [_P] * 4),
    "amt_ensemble_moments": (_I, [_P, _I, _I] + [_P] * 4),
    "amt_sumflux_device_f32": (_I, [_P, _I] + [_P] * 13 + [_I] * (2 + 17)),
    "amt_sumflux_device_f64": (_I, [_P, _I] + [_P] * 13 + [_I] * (2 + 17)),
    "amt_domain_set_sumflux": (_I, [_P, _I, _P, _P, _P]),
    "amt_domain_sumflux_accumulate": (_I, [_P]),
    "amt_domain_sumflux_state": (_I, [_P, ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "amt_domain_sumflux_ptr": (_P, [_P, _I]),
    "amt_ensemble_set_sumflux": (_I, [_P, _I, _P, _P, _P]),
    "amt_ensemble_sumflux_accumulate": (_I, [_P]),
    "amt_ensemble_sumflux_state": (_I, [_P, ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "amt_ensemble_sumflux_ptr": (_P, [_P, _I]),
    "amt_stage_prep_device_f32": (_I, [_P, _I] + [_P] * 12 + [_I] * (1 + 17)),
    "amt_stage_prep_device_f64": (_I, [_P, _I] + [_P] * 12 + [_I] * (1 + 17)),
    "amt_stage_finish_device_f32": (_I, [_P, _I] + [_P] * 8 + [ctypes.c_float, _I, _P] + [_I] * 17),
    "amt_stage_finish_device_f64": (_I, [_P, _I] + [_P] * 8 + [ctypes.c_double, _I, _P] + [_I] * 17),
    "amt_domain_set_stage": (_I, [_P, _I, _P, _P, _P, _P]),
    "amt_domain_stage_ptr": (_P, [_P, _I]),
    "amt_domain_stage_prep": (_I, [_P, _I]),
    "amt_domain_stage_finish": (_I, [_P, _I, _P]),
    "amt_ensemble_set_stage": (_I, [_P, _I, _P, _P, _P, _P]),
    "amt_ensemble_stage_ptr": (_P, [_P, _I]),
    "amt_ensemble_stage_prep": (_I, [_P, _I]),
    "amt_ensemble_stage_finish": (_I, [_P, _I, _P]),
    "amt_p_rho_device_f32": (_I, [_P, _I, _I, _I] + [_P] * 13 + [ctypes.c_float] * 2 + [_I] * 17),
    "amt_p_rho_device_f64": (_I, [_P, _I, _I, _I] + [_P] * 13 + [ctypes.c_double] * 2 + [_I] * 17),
    "amt_domain_set_p_rho": (_I, [_P, _I, _I, ctypes.c_double, ctypes.c_double] + [_P] * 8),
    "amt_domain_p_rho_ptr": (_P, [_P, _I]),
    "amt_domain_p_rho": (_I, [_P, _I]),
    "amt_ensemble_set_p_rho": (_I, [_P, _I, _I, ctypes.c_double, ctypes.c_double] + [_P] * 8),
    "amt_ensemble_p_rho_ptr": (_P, [_P, _I]),
    "amt_ensemble_p_rho": (_I, [_P, _I]),
    "amt_advance_uv_device_f32": (_I, [_P, _I, _I] + [_P] * 24 + [ctypes.c_float] * 7 + [_I] * 20),
    "amt_advance_uv_device_f64": (_I, [_P, _I, _I] + [_P] * 24 + [ctypes.c_double] * 7 + [_I] * 20),
    "amt_domain_set_uv": (_I, [_P, _I, _I] + [ctypes.c_double] * 4 + [_P] * 9),
    "amt_domain_uv_ptr": (_P, [_P, _I]),
    "amt_domain_uv": (_I, [_P]),
    "amt_ensemble_set_uv": (_I, [_P, _I, _I] + [ctypes.c_double] * 4 + [_P] * 9),
    "amt_ensemble_uv_ptr": (_P, [_P, _I]),
    "amt_ensemble_uv": (_I, [_P]),
    "amt_halo_plan": (_I, [_I] * (4 + 17 + 5) + [ctypes.POINTER(HaloMessage), _I, ctypes.POINTER(_I)]),
    "amt_grid_halo_messages": (_I, [_P, ctypes.POINTER(HaloMessage), _I, ctypes.POINTER(_I)]),
    "amt_slab_halo_messages": (_I, [_P, ctypes.POINTER(HaloMessage), _I, ctypes.POINTER(_I)]),
    "amt_grid_step_begin": (_I, [_P]),
    "amt_grid_halo_wait": (_I, [_P]),
    "amt_grid_step_end": (_I, [_P]),
    "amt_grid_halo_pack": (_I, [_P]),
    "amt_grid_halo_unpack": (_I, [_P]),
    "amt_slab_step_begin": (_I, [_P]),
    "amt_slab_halo_wait": (_I, [_P]),
    "amt_slab_step_end": (_I, [_P]),
    "amt_slab_halo_pack": (_I, [_P]),
    "amt_slab_halo_unpack": (_I, [_P]),
    "amt_march_force_shape": (_I, [_I] * 7),
    "amt_march_rows_for": (_I, [ctypes.c_long, _I, _I, ctypes.c_long, _I, _I]),
    "amt_march_set_xchunk": (_I, [_I]),
    "amt_march_set_beside": (_I, [_I, _I]),
    "amt_march_set_stream_policy": (_I, [_I]),
    "amt_march_last_kernel": (ctypes.c_char_p, []),
    "amt_march_selectable": (_I, [ctypes.c_char_p, _I]),
}


def load_library() -> ctypes.CDLL:
    """Load the HIP library (once).  torch, when used in the same process, must be imported
    first so that both share one HIP runtime (same SONAME libamdhip64.so.7)."""
    global _lib
    if _lib is None:
        path = library_path()
        if not path.exists():
            raise AmtError(ERR_NO_DEVICE, f"{path} not built -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                                          "(make -C wrf-model-cuda-sample_amd/csrc); there is no CPU fallback")
        try:
            # one HIP runtime per process: torch ships its own libamdhip64.so.7 and must bring it in
            # before this library resolves the same SONAME from /opt/rocm (otherwise torch ends up on
            # a runtime its other bundled libraries do not match: "no ROCm-capable device")
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(str(path))
        for name, (res, args) in SYMBOLS.items():
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _lib = L
    return _lib


def check(status: int) -> None:
    if status != OK:
        L = load_library()
        msg = L.amt_last_error().decode() or L.amt_status_string(status).decode()
        raise AmtError(status, msg)


class DeviceView:
    """Device memory the library owns, for ``torch.as_tensor``: a ``__cuda_array_interface__`` over ``ptr`` that keeps ``owner`` --
    the Python object whose handle owns the memory -- alive for as long as a tensor views it."""

    def __init__(self, owner, ptr: int, shape, typestr: str):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": tuple(int(n) for n in shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class ResidentHandle:
    """What a resident handle does whichever kind it is (header sections 4, 8, 9, 10, 12, 14, 15, 16): stepping, the per-sweep settings,
    the diagnostics and the release.  The owning class names its C functions' prefix (``amt_domain`` / ``amt_ensemble``) in
    ``_PREFIX`` and its member count in ``_members()``, and holds the library in ``L`` and the handle in ``handle``.  The stepping
    methods pass their status through ``_check`` so that an ERR_NONFINITE error carries the guard's report."""
    _PREFIX = "amt_domain"

    def _members(self) -> int:
        return 1

    def _fn(self, name: str):
        return getattr(self.L, f"{self._PREFIX}_{name}")

    def _check(self, status: int) -> None:
        if status == ERR_NONFINITE:
            msg = self.L.amt_last_error().decode()
            raise AmtError(status, msg, report=self.guard_report())
        check(status)

    def set_scalars(self, rdx, rdy, dts, epssm) -> None:
        check(self._fn("set_scalars")(self.handle, float(rdx), float(rdy), float(dts), float(epssm)))

    def set_variant(self, variant: int) -> None:
        check(self._fn("set_variant")(self.handle, int(variant)))

    def step(self, n_sweeps: int = 1) -> None:
        """``step``: asynchronous on the handle's stream; every member of an ensemble in one launch per sweep."""
        self._check(self._fn("step")(self.handle, int(n_sweeps)))

    def step_timed(self, n_sweeps: int = 1) -> float:
        ms = ctypes.c_float()
        self._check(self._fn("step_timed")(self.handle, int(n_sweeps), ctypes.byref(ms)))
        return float(ms.value)

    def sync(self) -> None:
        self._check(self._fn("sync")(self.handle))

    def set_cyclic(self, axes: int) -> None:
        """``set_cyclic``: CYCLIC_X | CYCLIC_Y of api.py; every sweep of ``step`` / ``step_timed`` is then preceded by a refresh
        of the wrap cells (one launch over all members).  0 = off."""
        check(self._fn("set_cyclic")(self.handle, int(axes)))

    def cyclic(self) -> int:
        return int(self._fn("cyclic")(self.handle))

    def cyclic_fill(self, axes: int) -> None:
        """``cyclic_fill``: one refresh (of every member) now, asynchronous on the handle's stream."""
        check(self._fn("cyclic_fill")(self.handle, int(axes)))

    def set_spec_bdy(self, on: bool = True) -> None:
        """``set_spec_bdy``: every sweep of ``step`` / ``step_timed`` is then followed by the boundary-zone update of a specified /
        nested domain (header section 12; one launch over all members).  False = off."""
        check(self._fn("set_spec_bdy")(self.handle, int(bool(on))))

    def spec_bdy(self) -> bool:
        return bool(self._fn("spec_bdy")(self.handle))

    def spec_bdy_update(self) -> None:
        """``spec_bdy_update``: one update (of every member) now, asynchronous on the handle's stream."""
        check(self._fn("spec_bdy_update")(self.handle))

    def field_ptr(self, field) -> int:
        """Device address of the array of ``field`` (a name or an ``amt_field`` id); 0 for an id that names none."""
        if isinstance(field, str):
            from .synth import FIELD_ID
            field = FIELD_ID[field]
        return int(self._fn("field_ptr")(self.handle, int(field)) or 0)

    @property
    def stream(self) -> int:
        return int(self._fn("stream")(self.handle) or 0)

    def close(self) -> None:
        if self.handle:
            self._fn("destroy")(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def field_stats(self, field: int, region: int = REGION_WINDOW):
        """``FieldStats`` of ``field`` (enum amt_field) over ``region``; an ensemble returns a list, one per member."""
        out = (FieldStats * self._members())()
        check(self._fn("field_stats")(self.handle, int(field), int(region), out))
        return list(out) if self._PREFIX == "amt_ensemble" else out[0]

    def compare(self, other, field: int, region: int = REGION_MEMORY):
        """``FieldDiff`` of this handle's ``field`` against ``other``'s (same dtype, bounds and member count)."""
        out = (FieldDiff * self._members())()
        check(self._fn("compare")(self.handle, other.handle, int(field), int(region), out))
        return list(out) if self._PREFIX == "amt_ensemble" else out[0]

    def set_guard(self, every: int) -> None:
        """0: off.  n >= 1: ww, t and mu are checked for NaN / Inf after every n-th sweep of the handle's own stepping; the
        first finding makes ``sync`` / ``step`` raise ``AmtError`` (status ERR_NONFINITE, ``.report`` set)."""
        check(self._fn("set_guard")(self.handle, int(every)))

    def guard_report(self) -> GuardReport:
        out = GuardReport()
        check(self._fn("guard_report")(self.handle, ctypes.byref(out)))
        return out

    # the acoustic loop's flux averages ru_m, rv_m, ww_m (header section 14)
    def set_sumflux(self, n_small_steps: int, ru_m=None, rv_m=None, ww_m=None) -> None:
        """``set_sumflux``: 0 = off.  n >= 1: every sweep of the handle's stepping is followed by one accumulation, the counter
        running 1..n and wrapping.  Without arrays the library allocates the accumulators; otherwise all three are device
        tensors (or addresses) of one 3-D field's extents (times the members), which the caller keeps alive."""
        ptr = lambda a: ctypes.c_void_p(None if a is None else a.data_ptr() if hasattr(a, "data_ptr") else int(a))
        check(self._fn("set_sumflux")(self.handle, int(n_small_steps), ptr(ru_m), ptr(rv_m), ptr(ww_m)))

    def sumflux_accumulate(self) -> None:
        """One accumulation now, asynchronous on the handle's stream; advances the counter."""
        check(self._fn("sumflux_accumulate")(self.handle))

    def sumflux_state(self):
        """(n_small_steps, next_iteration); n_small_steps = 0: off."""
        n, nxt = ctypes.c_int(), ctypes.c_int()
        check(self._fn("sumflux_state")(self.handle, ctypes.byref(n), ctypes.byref(nxt)))
        return int(n.value), int(nxt.value)

    def sumflux_ptr(self, which: int) -> int:
        """Device address of ru_m (0), rv_m (1) or ww_m (2); 0 while the setting is off."""
        return int(self._fn("sumflux_ptr")(self.handle, int(which)) or 0)

    # the bracket of a Runge-Kutta stage: small_step_prep and small_step_finish (header section 15)
    def set_stage(self, on: bool = True, t_old=None, mu_old=None, mu_save=None, mub=None) -> None:
        """``set_stage``: False = off.  Without arrays the library allocates ``t_old`` (one 3-D field's extents) and ``mu_old``,
        ``mu_save``, ``mub`` (one 2-D field's, all times the members); otherwise all four are device tensors (or addresses) which
        the caller keeps alive.  ``mub`` is a pure input: fill it once (``stage_ptr(3)``)."""
        check(self._fn("set_stage")(self.handle, int(bool(on)), *[_address(a) for a in (t_old, mu_old, mu_save, mub)]))

    def stage_ptr(self, which: int) -> int:
        """Device address of t_old (0), mu_old (1), mu_save (2) or mub (3); 0 while the setting is off."""
        return int(self._fn("stage_ptr")(self.handle, int(which)) or 0)

    def stage_prep(self, rk_step: int) -> None:
        """``stage_prep``: small_step_prep of Runge-Kutta step ``rk_step`` >= 1 in front of the stage's acoustic loop,
        asynchronous on the handle's stream (every member of an ensemble in one launch)."""
        check(self._fn("stage_prep")(self.handle, int(rk_step)))

    def stage_finish(self, n_small_steps: int, h_diabatic=None) -> None:
        """``stage_finish``: small_step_finish behind a loop of ``n_small_steps`` sweeps, with the handle's dts;
        ``h_diabatic``: a device tensor (or address) of one 3-D field's extents, or None."""
        check(self._fn("stage_finish")(self.handle, int(n_small_steps), _address(h_diabatic)))

    # the pressure diagnosis that closes an acoustic sub-step: calc_p_rho (header section 16)
    def set_p_rho(self, mode: int, per_sweep: bool = False, t0: float = 300.0, smdiv: float = 0.0,
                  al=None, p=None, ph=None, pm1=None, alt=None, c2a=None, znu=None, dnw=None) -> None:
        """``set_p_rho``: mode 0 = off, 1 = non-hydrostatic, 2 = hydrostatic.  Without arrays the library allocates ``al``, ``p``,
        ``ph``, ``pm1``, ``alt``, ``c2a`` (one 3-D field's extents times the members) and ``znu``, ``dnw`` (one level array);
        otherwise all eight are device tensors (or addresses) which the caller keeps alive.  ``alt``, ``c2a``, ``ph``, ``znu``,
        ``dnw`` are the host's to fill (``p_rho_ptr``).  Needs ``set_stage``.  ``per_sweep``: every sweep of ``step`` is followed
        by one diagnosis with step != 0."""
        check(self._fn("set_p_rho")(self.handle, int(mode), int(bool(per_sweep)), float(t0), float(smdiv),
                                    *[_address(a) for a in (al, p, ph, pm1, alt, c2a, znu, dnw)]))

    def p_rho_ptr(self, which: int) -> int:
        """Device address of al (0), p (1), ph (2), pm1 (3), alt (4), c2a (5), znu (6) or dnw (7); 0 while the setting is off."""
        return int(self._fn("p_rho_ptr")(self.handle, int(which)) or 0)

    def p_rho(self, step: int) -> None:
        """``p_rho``: one diagnosis now, asynchronous on the handle's stream (every member of an ensemble in one launch);
        ``step`` 0 is the call behind ``stage_prep``."""
        check(self._fn("p_rho")(self.handle, int(step)))

    # the momentum update that opens an acoustic sub-step: advance_uv (header section 17)
    def set_uv(self, on: bool, per_sweep: bool = False, emdiv: float = 0.0, cf1: float = 0.0, cf2: float = 0.0, cf3: float = 0.0,
               ru_tend=None, rv_tend=None, pb=None, php=None, cqu=None, cqv=None, msfux=None, msfvx=None, msfvy=None) -> None:
        """``set_uv``: without arrays the library allocates ``ru_tend``, ``rv_tend``, ``pb``, ``php``, ``cqu``, ``cqv`` (one 3-D
        field's extents times the members) and ``msfux``, ``msfvx``, ``msfvy`` (one 2-D field's), which the host fills
        (``uv_ptr``); otherwise all nine are device tensors (or addresses) which the caller keeps alive.  Needs ``set_p_rho``,
        whose ``al``, ``p``, ``ph``, ``alt`` it reads; mode 1 there is the non-hydrostatic form here.  ``per_sweep``: every sweep
        of ``step`` is preceded by one update."""
        check(self._fn("set_uv")(self.handle, int(bool(on)), int(bool(per_sweep)), float(emdiv), float(cf1), float(cf2), float(cf3),
                                 *[_address(a) for a in (ru_tend, rv_tend, pb, php, cqu, cqv, msfux, msfvx, msfvy)]))

    def uv_ptr(self, which: int) -> int:
        """Device address of ru_tend (0), rv_tend (1), pb (2), php (3), cqu (4), cqv (5), msfux (6), msfvx (7) or msfvy (8); 0
        while the setting is off."""
        return int(self._fn("uv_ptr")(self.handle, int(which)) or 0)

    def uv(self) -> None:
        """``uv``: one update now, asynchronous on the handle's stream (every member of an ensemble in one launch), behind the
        wrap refresh of its read arrays on a cyclic handle."""
        check(self._fn("uv")(self.handle))


def _address(a):
    """A device tensor, an address or None as a ``c_void_p``."""
    return ctypes.c_void_p(None if a is None else a.data_ptr() if hasattr(a, "data_ptr") else int(a))


HandleDiag = ResidentHandle          # the name this class had while it held the diagnostics only
