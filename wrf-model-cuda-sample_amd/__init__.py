"""MI355X-native advance_mu_t (WRF-ARW acoustic sub-step: mu, ww, theta update).

Host-side mirror of the reference's interface for this one path:

* ``advance_mu_t(...)``  -- same name, argument order and meaning as
  ``SUBROUTINE advance_mu_t`` (module_small_step_em.f90:7-18); numpy arrays take the
  one-shot host drop-in, torch CUDA tensors the device-resident one.  Both go through
  the C-ABI of ``include/amt_advance_mu_t.h`` into the hand-written gfx950 kernels.
* ``GridConfig``         -- the three ``grid_config_rec_type`` logicals the routine reads.
* ``synth``              -- seeded WRF-shaped synthetic inputs (host and device fill).
* ``wrfdump``            -- the reference drivers' big-endian per-variable dump format.
* ``ensemble``           -- ``members`` same-shape patches advanced by one launch per sweep
  (``advance_mu_t_ensemble``, ``Ensemble``; member-stacked arrays).
* ``diag``               -- statistics and bit comparison of torch device tensors on the device
  (``field_stats``, ``compare``); the resident handles carry the same plus a non-finite guard.
* ``patch``              -- resident device patch (torch-allocated arrays) and j-slab
  decomposition with the one-row input-halo exchange over torch.distributed (RCCL).

The directory name contains '-' (it is the reference repository's name + ``_amd``), so it
is loaded through ``__graft_entry__.load_package()`` under the module name
``wrf_model_cuda_sample_amd``.  There is no CPU fallback: without the built HIP library
every compute entry point raises.
"""
from .config import GridConfig  # noqa: F401
from .lib import AmtError, load_library, library_path  # noqa: F401
from .lib import FieldStats, FieldDiff, GuardReport, REGION_WINDOW, REGION_MEMORY  # noqa: F401
from .api import advance_mu_t, bind_device_call, compute_window, VARIANT_AUTO, VARIANT_COLUMN, VARIANT_MARCH, LAUNCH_BESIDE_OTHERS  # noqa: F401
from .api import host_cache_enable, host_invalidate, host_defer, host_fetch, host_stale, host_release, held_arrays  # noqa: F401
from .api import host_set_devices, host_devices  # noqa: F401
from .api import cyclic_fill, spec_bdy_update, sumflux, stage_prep, stage_finish, p_rho, advance_uv, CYCLIC_X, CYCLIC_Y  # noqa: F401
from . import synth  # noqa: F401
from . import patch  # noqa: F401
from . import wrfdump  # noqa: F401
from . import ensemble  # noqa: F401
from .ensemble import Ensemble, advance_mu_t_ensemble  # noqa: F401
from . import diag  # noqa: F401
from .diag import field_stats, compare  # noqa: F401
