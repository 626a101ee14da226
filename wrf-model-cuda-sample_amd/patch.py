"""j-slab decomposition of advance_mu_t with a one-row input-halo exchange.

The reference splits the domain statically on j across its GPUs and refills three
redundant halo rows per side from the host copy on every call, with no inter-GPU
communication (advance_mu_t_no_async.cu:108-162).  Here one process owns one GPU and one
contiguous j-slab (``synth.slab_bounds``), keeps it resident, and before each sweep trades
exactly the rows the stencil reads across a slab edge:

  * from the slab above (j+1):  row jhi+1 of  v, v_1, t_1 (3-D)  and  muv, msfvx_inv (2-D)
    (module_small_step_em.f90:143, :241)
  * from the slab below (j-1):  row jlo-1 of  t_1                                  (:242)

All of them are pure inputs, so the exchange runs on a second stream while the interior
rows jlo+1..jhi-1 are computed; only the two edge rows wait for it.  In (i,k,j) layout a
j-row is one contiguous run of idim*kdim elements, so rows are sent in place (no packing).
Transport: ``torch.distributed`` point-to-point -- backend "nccl" is RCCL send/recv over
xGMI on ROCm; the same code runs over "gloo" on CPU tensors in the tests.  No collective
is needed anywhere in this path.
"""
from __future__ import annotations

from typing import Callable, Optional

from . import synth as _S
from .synth import Patch, HALO_FROM_ABOVE, HALO_FROM_BELOW


def _dist():
    import torch.distributed as dist
    return dist


def _fault(step: str, occurrence: int) -> bool:
    """AMT_TEST_FAULT="<step>@<n>" (csrc/amt_internal.h): the n-th exchange of a torch stepper is skipped by every rank
    ("skip_exchange") -- the halo-freshness tests must turn red on it.  Unset outside those tests."""
    import os
    spec = os.environ.get("AMT_TEST_FAULT", "")
    return bool(spec) and spec == f"{step}@{occurrence}"


CYCLIC_X_FLAG, CYCLIC_Y_FLAG = 8, 16            # AMT_SLAB_CYCLIC_X, AMT_SLAB_CYCLIC_Y of enum amt_slab_flags


def cyclic_sides(ri: int, rj: int, pi: int, pj: int, cyclic=(False, False)) -> int:
    """The sides of patch (ri, rj) of pi x pj whose halo is delivered every sweep: by a neighbour, or -- in a cyclic
    direction -- by the rank across the domain edge or by the patch itself (one rank in that direction)."""
    sides = _S.neighbour_sides(ri, rj, pi, pj)
    if cyclic[0]:
        sides |= _S.SIDE_LEFT | _S.SIDE_RIGHT
    if cyclic[1]:
        sides |= _S.SIDE_BELOW | _S.SIDE_ABOVE
    return sides


def _edge_cells(b):
    """Memory indices (c_first, c_last, r_first, r_last) of the compute window's edge columns and rows: what a patch sends
    across a cyclic domain edge, and next to which it receives (a last patch may end at ide-1 or at ide)."""
    return (b.its - b.ims, min(b.ite, b.ide - 1) - b.ims, b.jts - b.jms, min(b.jte, b.jde - 1) - b.jms)


def _self_wrap(patch: Patch, x: bool, y: bool) -> None:
    """A cyclic direction with ONE rank: the patch is its own neighbour there.  Column i_end+1 <-
    i_start of HALO_FROM_RIGHT and i_start-1 <- i_end of t_1 over the window's rows; row j_end+1 <- j_start of HALO_FROM_ABOVE
    and j_start-1 <- j_end of t_1 over the window's columns.  Torch slicing, for the CPU (gloo) tests and bring-up."""
    a = patch.arrays
    c0, c1, r0, r1 = _edge_cells(patch.bounds)
    if x:
        for name in _S.HALO_FROM_RIGHT:
            a[name][r0:r1 + 1, ..., c1 + 1] = a[name][r0:r1 + 1, ..., c0]
        a["t_1"][r0:r1 + 1, :, c0 - 1] = a["t_1"][r0:r1 + 1, :, c1]
    if y:
        for name in HALO_FROM_ABOVE:
            a[name][r1 + 1, ..., c0:c1 + 1] = a[name][r0, ..., c0:c1 + 1]
        a["t_1"][r0 - 1, :, c0:c1 + 1] = a["t_1"][r1, :, c0:c1 + 1]


def exchange_plan(ri: int, rj: int, pi: int, pj: int, cyclic=(False, False)):
    """Neighbours and the ORDER of the segments of one exchange of patch (ri, rj) of pi x pj, as amt_grid_create builds them
    (csrc/amt_grid.hip): (left, right, below, above, sends, recvs), a neighbour None where there is none, sends / recvs lists
    of (peer, what).  Per pair of ranks the k-th send to a peer is the k-th receive from it on the other side -- also when both
    neighbours of a direction are the SAME peer (two ranks in a cyclic direction): towards below / left first on the sending
    side, from above / right first on the receiving side."""
    rank = rj * pi + ri
    wx, wy = bool(cyclic[0]) and pi > 1, bool(cyclic[1]) and pj > 1
    left = rank - 1 if ri > 0 else rank + (pi - 1) if wx else None
    right = rank + 1 if ri < pi - 1 else rank - (pi - 1) if wx else None
    below = rank - pi if rj > 0 else rank + pi * (pj - 1) if wy else None
    above = rank + pi if rj < pj - 1 else rank - pi * (pj - 1) if wy else None
    sends, recvs = [], []
    if below is not None:
        sends += [(below, f"row_first:{n}") for n in HALO_FROM_ABOVE]
    if above is not None:
        sends += [(above, f"row_last:{n}") for n in HALO_FROM_BELOW]
    if left is not None:
        sends.append((left, "cols_first"))
    if right is not None:
        sends.append((right, "cols_last"))
    if above is not None:
        recvs += [(above, f"row_first:{n}") for n in HALO_FROM_ABOVE]
    if below is not None:
        recvs += [(below, f"row_last:{n}") for n in HALO_FROM_BELOW]
    if right is not None:
        recvs.append((right, "cols_first"))
    if left is not None:
        recvs.append((left, "cols_last"))
    return left, right, below, above, sends, recvs


class SlabStepper:
    """Runs advance_mu_t sweeps on one j-slab of a domain split over ``world`` ranks.

    ``patch``   : this rank's Patch (bounds from ``synth.slab_bounds``; arrays are torch
                  tensors -- CUDA for the product path, CPU in the gloo tests).
    ``compute`` : callable(*the 48 advance_mu_t arguments, stream=...) that updates a tile in
                  place.  The product passes ``api.advance_mu_t`` (HIP); there is no default
                  CPU implementation.
    """

    def __init__(self, patch: Patch, rank: int, world: int, compute: Callable, *,
                 group=None, overlap: bool = True, variant: int = 0, transport: Optional[Callable] = None,
                 stage_through_host: bool = False, cyclic=(False, False)):
        self.patch, self.rank, self.world = patch, rank, world
        # cyclic = (x, y): the domain is periodic in that direction.  x: a slab holds the whole period:
        # self wrap in front of every sweep.  y: slab 0 and slab world-1 are each other's neighbours (world == 1: self wrap).
        self.cyclic = (bool(cyclic[0]), bool(cyclic[1]))
        self.compute, self.group, self.overlap, self.variant = compute, group, overlap, variant
        # transport(stepper): replaces the torch.distributed exchange (tests run several slabs of
        # one domain in ONE process on one GPU and copy the halo rows device-to-device)
        self.transport = transport
        self._bound = {}          # (jts, jte) -> pre-marshalled device call (see api.bind_device_call)
        # stage_through_host: the process group cannot move device memory (gloo): bounce every row
        # through a host buffer.  Debug/bring-up only -- lets the whole N > 1 bench path run with
        # several ranks sharing one GPU, which RCCL refuses.
        self.stage_through_host = stage_through_host
        self.below: Optional[int] = rank - 1 if rank > 0 else None
        self.above: Optional[int] = rank + 1 if rank < world - 1 else None
        if self.cyclic[1] and world > 1:
            self.below = self.below if self.below is not None else world - 1
            self.above = self.above if self.above is not None else 0
        any_arr = patch.arrays["t_1"]
        self.on_gpu = bool(getattr(any_arr, "is_cuda", False))
        self.main_stream = self.comm_stream = None
        if self.on_gpu:
            import torch
            self.main_stream = torch.cuda.current_stream(any_arr.device)
            # high priority: the exchange and the edge rows are small and the sweep's join waits for them;
            # they must not queue behind the interior's remaining rounds of workgroups
            self.comm_stream = torch.cuda.Stream(device=any_arr.device, priority=-1)
        b = patch.bounds
        if world > 1 and (b.jme - b.jms + 1) != (b.jte - b.jts + 1) + 2:
            raise ValueError("a slab patch holds its rows plus exactly one halo row per side")

    # -- halo exchange -----------------------------------------------------------------
    def _p2p_ops(self):
        dist = _dist()
        a = self.patch.arrays
        jdim = self.patch.bounds.jdim
        first_owned, last_owned, halo_lo, halo_hi = 1, jdim - 2, 0, jdim - 1
        if self.cyclic[1]:                                 # the window's edge rows: a last slab may end at jde-1 or at jde
            _c0, _c1, first_owned, last_owned = _edge_cells(self.patch.bounds)
            halo_lo, halo_hi = first_owned - 1, last_owned + 1
        ops = []
        # order per peer pair is fixed (NCCL/RCCL matches send/recv by order, gloo by tag)
        if self.below is not None:
            for n, name in enumerate(HALO_FROM_ABOVE):     # my first row is their row jhi+1
                ops.append(dist.P2POp(dist.isend, a[name][first_owned], self.below, self.group, tag=10 + n))
            for n, name in enumerate(HALO_FROM_BELOW):
                ops.append(dist.P2POp(dist.irecv, a[name][halo_lo], self.below, self.group, tag=20 + n))
        if self.above is not None:
            for n, name in enumerate(HALO_FROM_ABOVE):
                ops.append(dist.P2POp(dist.irecv, a[name][halo_hi], self.above, self.group, tag=10 + n))
            for n, name in enumerate(HALO_FROM_BELOW):     # my last row is their row jlo-1
                ops.append(dist.P2POp(dist.isend, a[name][last_owned], self.above, self.group, tag=20 + n))
        return ops

    def exchange_halos(self):
        """Post the sends/receives of one sweep and wait for them on the current stream
        (device-side wait for RCCL; host wait for gloo)."""
        self._exchanges = getattr(self, "_exchanges", 0) + 1
        if _fault("skip_exchange", self._exchanges):
            return
        if self.transport is not None:
            self.transport(self)
            return
        ops = self._p2p_ops()
        if not ops:
            return
        if self.stage_through_host and self.on_gpu:
            dist = _dist()
            staged, recvs = [], []
            for op in ops:
                if op.op is dist.isend:
                    staged.append(dist.P2POp(dist.isend, op.tensor.cpu(), op.peer, op.group, op.tag))
                else:
                    host = op.tensor.new_empty(op.tensor.shape, device="cpu")
                    recvs.append((op.tensor, host))
                    staged.append(dist.P2POp(dist.irecv, host, op.peer, op.group, op.tag))
            for req in dist.batch_isend_irecv(staged):
                req.wait()
            for dev, host in recvs:
                dev.copy_(host, non_blocking=False)
            return
        for req in _dist().batch_isend_irecv(ops):
            req.wait()

    def halo_bytes_per_sweep(self) -> int:
        """Bytes this rank sends + receives per sweep."""
        a = self.patch.arrays
        n = 0
        for peer, names in ((self.below, HALO_FROM_ABOVE + HALO_FROM_BELOW),
                            (self.above, HALO_FROM_ABOVE + HALO_FROM_BELOW)):
            if peer is not None:
                n += sum(a[name][0].numel() * a[name].element_size() for name in names)
        return n

    # -- one sweep ---------------------------------------------------------------------
    def _tile(self, jts: int, jte: int, stream, beside: bool = False):
        if jte < jts:
            return
        if self.on_gpu:
            variant = self.variant | (0x100 if beside else 0)        # LAUNCH_BESIDE_OTHERS: leave round boundaries to the exchange
            key = (jts, jte, id(stream), beside)
            call = self._bound.get(key)
            if call is None:
                args = self.patch.with_bounds(jts=jts, jte=jte).args()
                binder = getattr(self.compute, "bind", None)
                if binder is None:                   # a plain callable: marshal on every call
                    self.compute(*args, stream=stream, variant=variant)
                    return
                call = self._bound[key] = binder(*args, stream=stream, variant=variant)
            call()
        else:
            self.compute(*self.patch.with_bounds(jts=jts, jte=jte).args())

    def step(self):
        b = self.patch.bounds
        jlo, jhi = b.jts, b.jte
        if self.cyclic[1]:
            jhi = min(jhi, b.jde - 1)
        if self.cyclic[0] or (self.cyclic[1] and self.world == 1):
            _self_wrap(self.patch, self.cyclic[0], self.cyclic[1] and self.world == 1)      # on the current stream: inputs are final
        if self.world == 1 or (self.below is None and self.above is None):
            self._tile(jlo, jhi, self.main_stream)
            return
        # rows that read a neighbour's data: jlo (if there is a slab below), jhi (if above)
        in_lo = jlo + (1 if self.below is not None else 0)
        in_hi = jhi - (1 if self.above is not None else 0)
        if self.on_gpu and self.overlap:
            import torch
            # comm stream: exchange, then the edge rows (they need nothing but the halos and the
            # inputs).  main stream: the interior.  The small edge launches (one row each) then fill
            # the CUs that the interior's last, partly filled round of workgroups leaves idle.
            self.comm_stream.wait_stream(self.main_stream)      # inputs of this sub-step are final
            self._tile(in_lo, in_hi, self.main_stream, beside=True)   # interior overlaps the exchange
            with torch.cuda.stream(self.comm_stream):
                self.exchange_halos()                           # RCCL send/recv on the comm stream
                self._edges(jlo, jhi, self.comm_stream)
            self.main_stream.wait_stream(self.comm_stream)
        else:
            self.exchange_halos()
            self._tile(in_lo, in_hi, self.main_stream)
            self._edges(jlo, jhi, self.main_stream)

    def _edges(self, jlo, jhi, stream):
        if self.below is not None:
            self._tile(jlo, min(jlo, jhi), stream)
        if self.above is not None and (jhi > jlo or self.below is None):
            self._tile(jhi, jhi, stream)


# i-direction halos (module_small_step_em.f90:145 reads u, u_1, muu, msfuy at i+1; :244-245 read
# t_1 at i+1 and i-1)
from .synth import HALO_FROM_RIGHT, HALO_FROM_LEFT  # noqa: E402  (re-exported: tests name them through this module)


class GridStepper:
    """advance_mu_t on patch (ri, rj) of a pi x pj decomposition in i AND j (SURVEY.md section 8f
    row 4).  j halos are contiguous rows and travel in place as in SlabStepper; i halos are columns
    (stride idim in memory), so they are packed into contiguous buffers, sent, and unpacked on
    arrival.  No diagonal neighbours are needed: the stencil reads (i+-1, j) and (i, j+-1) only.
    One launch per sweep after the exchange (no interior/edge split here: this decomposition is for
    domains too small in j to be bandwidth-bound per GPU).  Ranks are row-major: rank = rj*pi + ri.
    """

    def __init__(self, patch: Patch, ri: int, rj: int, pi: int, pj: int, compute: Callable, *,
                 group=None, variant: int = 0, stage_through_host: bool = False,
                 native: Optional[str] = None, unique_id: Optional[bytes] = None, overlap: bool = True, cyclic=(False, False)):
        self.patch, self.ri, self.rj, self.pi, self.pj = patch, ri, rj, pi, pj
        self.cyclic = (bool(cyclic[0]), bool(cyclic[1]))      # the torus topology of amt_grid_create (exchange_plan)
        self.compute, self.group, self.variant = compute, group, variant
        self.stage_through_host = stage_through_host
        # native="rccl" | "ipc": a device patch is stepped by the C++ runtime (amt_grid_*: HIP pack / unpack kernels, one
        # exchange, interior beside it) and this class only forwards; None: the torch.distributed path below (CPU tensors
        # over gloo in the tests; device tensors staged through the host for bring-up)
        self._native = None
        if native is not None:
            self._native = NativeGridStepper(patch, ri, rj, pi, pj, unique_id, overlap=overlap, variant=variant, transport=native,
                                             cyclic=self.cyclic)
        self.left, self.right, self.below, self.above, _sends, _recvs = exchange_plan(ri, rj, pi, pj, self.cyclic)
        self._self = (self.cyclic[0] and pi == 1, self.cyclic[1] and pj == 1)
        b = patch.bounds
        self.c_first, self.c_last = b.its - b.ims, b.ite - b.ims          # owned columns (memory index)
        self.r_first, self.r_last = 1, b.jdim - 2
        if any(self.cyclic):                                                # the window's edges (a last patch may end at ide / jde)
            c0, c1, r0, r1 = _edge_cells(b)
            if self.cyclic[0]:
                self.c_first, self.c_last = c0, c1
            if self.cyclic[1]:
                self.r_first, self.r_last = r0, r1
        self.c_halo_l, self.c_halo_r = self.c_first - 1, self.c_last + 1
        self.on_gpu = bool(getattr(patch.arrays["t_1"], "is_cuda", False))
        self._call = None

    def _col(self, name, c):
        a = self.patch.arrays[name]
        return a[..., c]                                   # (jdim, kdim) or (jdim,) strided view

    def exchange_halos(self):
        if self._native is not None:
            return self._native.exchange_halos()
        self._exchanges = getattr(self, "_exchanges", 0) + 1
        if _fault("skip_exchange", self._exchanges):
            return
        if any(self._self):
            _self_wrap(self.patch, *self._self)
        dist = _dist()
        a = self.patch.arrays
        ops, unpack = [], []
        host = self.stage_through_host and self.on_gpu

        def send(t, peer, tag):
            t = t.contiguous()
            ops.append(dist.P2POp(dist.isend, t.cpu() if host else t, peer, self.group, tag))

        def recv(view, peer, tag, packed):
            if packed or host:
                buf = view.new_empty(view.shape, device="cpu" if host else view.device)
                unpack.append((view, buf))
                ops.append(dist.P2POp(dist.irecv, buf, peer, self.group, tag))
            else:
                ops.append(dist.P2POp(dist.irecv, view, peer, self.group, tag))

        if self.below is not None:
            for n, name in enumerate(HALO_FROM_ABOVE):
                send(a[name][self.r_first], self.below, 10 + n)
            recv(a["t_1"][self.r_first - 1], self.below, 20, False)
        if self.above is not None:
            for n, name in enumerate(HALO_FROM_ABOVE):
                recv(a[name][self.r_last + 1], self.above, 10 + n, False)
            send(a["t_1"][self.r_last], self.above, 20)
        if self.left is not None:
            for n, name in enumerate(HALO_FROM_RIGHT):     # my first column is their column ihi+1
                send(self._col(name, self.c_first), self.left, 30 + n)
            recv(self._col("t_1", self.c_halo_l), self.left, 40, True)
        if self.right is not None:
            for n, name in enumerate(HALO_FROM_RIGHT):
                recv(self._col(name, self.c_halo_r), self.right, 30 + n, True)
            send(self._col("t_1", self.c_last), self.right, 40)
        if not ops:
            return
        for req in dist.batch_isend_irecv(ops):
            req.wait()
        for view, buf in unpack:
            view.copy_(buf)

    def step(self):
        if self._native is not None:
            return self._native.step(1)
        self.exchange_halos()
        args = self.patch.args()
        if self.on_gpu:
            if self._call is None:
                binder = getattr(self.compute, "bind", None)
                if binder is None:
                    self.compute(*args, variant=self.variant)
                    return
                self._call = binder(*args, variant=self.variant)
            self._call()
        else:
            self.compute(*args)


class _NativeStepper:
    """What the steppers over the C++ runtime share.  The 26 torch CUDA tensors of ``patch`` stay the owners: ``_open`` wraps
    them in an ``amt_domain_wrap`` handle (``_dom``) on ``stream``, configures it, and makes the stepper's own handle (``_h``)
    with ``<_HANDLE>_create``.  A subclass names the prefix of its handle's C functions in ``_HANDLE`` and sets ``cyclic`` and
    ``_halo_sides`` before it calls ``_open``."""

    NO_OVERLAP, LOOPBACK, TRANSPORT_IPC = 1, 2, 4          # enum amt_slab_flags
    _HANDLE = "amt_grid"

    def _open(self, patch: Patch, rank_args, flags: int, *, overlap, stream, variant, spec_bdy, sumflux, transport=None, unique_id=None):
        import ctypes
        import torch
        from . import lib as _lib
        from .synth import FIELD_NAMES
        self._lib, self._ct = _lib, ctypes
        self.L = L = _lib.load_library()
        self.patch = patch
        t0 = patch.arrays["t_1"]
        if not t0.is_cuda:
            raise TypeError(f"{type(self).__name__} needs a device patch (there is no CPU path)")
        if transport not in (None, "rccl", "ipc"):
            raise ValueError("transport is 'rccl' or 'ipc'")
        b = patch.bounds
        for name in FIELD_NAMES:
            t = patch.arrays[name]
            if not (t.is_cuda and t.dtype == t0.dtype and t.is_contiguous() and tuple(t.shape) == tuple(b.shape(name))):
                raise TypeError(f"{name}: need a contiguous device tensor of shape {b.shape(name)}")
        self.stream = stream if stream is not None else torch.cuda.Stream(device=t0.device)
        self.device_index = t0.device.index if t0.device.index is not None else torch.cuda.current_device()
        fields = (ctypes.c_void_p * len(FIELD_NAMES))(*[patch.arrays[n].data_ptr() for n in FIELD_NAMES])
        self.flags = (flags | (0 if overlap else self.NO_OVERLAP) | (self.TRANSPORT_IPC if transport == "ipc" else 0)
                      | (CYCLIC_X_FLAG if self.cyclic[0] else 0) | (CYCLIC_Y_FLAG if self.cyclic[1] else 0))
        self._dom, self._h = ctypes.c_void_p(), ctypes.c_void_p()
        with self._dev():
            _lib.check(L.amt_domain_wrap(ctypes.byref(self._dom), t0.element_size(), *patch.config.as_ints(),
                                         *b.as_tuple(), fields, ctypes.c_void_p(self.stream.cuda_stream)))
            try:
                _lib.check(L.amt_domain_set_scalars(self._dom, patch.rdx, patch.rdy, patch.dts, patch.epssm))
                _lib.check(L.amt_domain_set_variant(self._dom, int(variant)))
                if spec_bdy:                                  # the boundary-zone update behind every sweep (header section 12)
                    _lib.check(L.amt_domain_set_spec_bdy(self._dom, 1))
                if sumflux:                                   # the flux averages behind every sweep (header section 14)
                    _lib.check(L.amt_domain_set_sumflux(self._dom, int(sumflux), None, None, None))
                uid = None
                if unique_id is not None:
                    uid = (ctypes.c_char * 128).from_buffer_copy(bytes(unique_id))
                _lib.check(getattr(L, f"{self._HANDLE}_create")(ctypes.byref(self._h), self._dom, *rank_args, uid, self.flags))
            except BaseException:
                L.amt_domain_destroy(self._dom)
                self._dom = ctypes.c_void_p()
                raise

    def _dev(self):
        import torch
        return torch.cuda.device(self.device_index)

    def _fn(self, name: str):
        return getattr(self.L, f"{self._HANDLE}_{name}")

    def _call(self, name: str, *args):
        with self._dev():
            self._lib.check(self._fn(name)(self._h, *args))

    def sync(self):
        self._call("sync")

    def next_substep_inputs(self, seed: int, sweep: int, poison: bool = True):
        """What a host model does between two calls: new values in the fields that cross a patch boundary (the stand-in for
        advance_uv: amt_domain_fill_fields with AMT_EXCHANGED_FIELDS, seed + sweep) and, for verification, NaN in the halo
        rows and columns (amt_domain_poison_halos) -- both on the domain's stream.  Only an exchange that delivers THIS
        sweep's halos then gives the bits of the unsplit run."""
        b = self.patch.bounds
        gdims = self.patch.global_dims or (b.ide - b.ids, b.kde - 1, b.jde - b.jds)
        mask = 0
        for name in _S.EXCHANGED_INPUTS:
            mask |= 1 << _S.FIELD_ID[name]
        with self._dev():
            self._lib.check(self.L.amt_domain_fill_fields(self._dom, mask, _S.sweep_seed(seed, sweep), b.ims, b.kms - 1, b.jms,
                                                          gdims[0] + 2, gdims[1] + 1, gdims[2] + 2))
            if poison and self._halo_sides:
                self._lib.check(self.L.amt_domain_poison_halos(self._dom, self._halo_sides))

    def halo_bytes_per_sweep(self) -> int:
        return int(self._fn("halo_bytes")(self._h))                  # sent + received

    def transport(self) -> str:
        """'rccl', 'ipc', 'external' or 'none' -- what carries this stepper's halos (amt_slab_transport / amt_grid_transport)."""
        return self._fn("transport")(self._h).decode()

    # ``sumflux=n`` (header section 14): every sweep is followed by one accumulation of this rank's own tile into ru_m, rv_m,
    # ww_m, which the library allocates; the counter runs 1..n and wraps.  Nothing is exchanged for it.
    def sumflux_state(self):
        """(n_small_steps, next_iteration); n_small_steps = 0: off."""
        n, nxt = self._ct.c_int(), self._ct.c_int()
        self._lib.check(self.L.amt_domain_sumflux_state(self._dom, self._ct.byref(n), self._ct.byref(nxt)))
        return int(n.value), int(nxt.value)

    def sumflux_arrays(self):
        """ru_m, rv_m, ww_m as torch tensors that view the library's device arrays (valid while the stepper lives)."""
        import torch
        b, t0 = self.patch.bounds, self.patch.arrays["t_1"]
        out = []
        for which in range(3):
            ptr = self.L.amt_domain_sumflux_ptr(self._dom, which)
            if not ptr:
                raise self._lib.AmtError(self._lib.ERR_INVALID_ARG, "the flux averages are off")
            view = self._lib.DeviceView(self, ptr, b.shape("ww"), "<f8" if t0.element_size() == 8 else "<f4")
            out.append(torch.as_tensor(view, device=t0.device))
        return tuple(out)

    # The bracket of a Runge-Kutta stage (header section 15) on this rank's own tile: issued on the domain handle between the
    # stepper's step calls, ordered by the domain's stream; nothing is exchanged for it (the halo exchange carries t_1).
    def set_stage(self, on: bool = True):
        """The library allocates t_old, mu_old, mu_save, mub (``stage_arrays``); False frees them."""
        with self._dev():
            self._lib.check(self.L.amt_domain_set_stage(self._dom, int(bool(on)), None, None, None, None))

    def stage_arrays(self):
        """t_old, mu_old, mu_save, mub as torch tensors that view the library's device arrays (valid while the stepper lives)."""
        import torch
        b, t0 = self.patch.bounds, self.patch.arrays["t_1"]
        out = []
        for which in range(4):
            ptr = self.L.amt_domain_stage_ptr(self._dom, which)
            if not ptr:
                raise self._lib.AmtError(self._lib.ERR_PRECONDITION, "the stage bracket is off")
            view = self._lib.DeviceView(self, ptr, b.shape("t" if which == 0 else "mu"), "<f8" if t0.element_size() == 8 else "<f4")
            out.append(torch.as_tensor(view, device=t0.device))
        return tuple(out)

    def stage_prep(self, rk_step: int):
        with self._dev():
            self._lib.check(self.L.amt_domain_stage_prep(self._dom, int(rk_step)))

    def stage_finish(self, n_small_steps: int, h_diabatic=None):
        with self._dev():
            self._lib.check(self.L.amt_domain_stage_finish(self._dom, int(n_small_steps), self._lib._address(h_diabatic)))

    # The pressure diagnosis that closes an acoustic sub-step (header section 16) on this rank's own tile; it needs
    # ``set_stage``.  With ``per_sweep`` the stepper's step calls enqueue it where the flux accumulation is; nothing is exchanged.
    def set_p_rho(self, mode: int, per_sweep: bool = False, t0: float = 300.0, smdiv: float = 0.0):
        """The library allocates al, p, ph, pm1, alt, c2a, znu, dnw (``p_rho_arrays``); mode 0 frees them."""
        with self._dev():
            self._lib.check(self.L.amt_domain_set_p_rho(self._dom, int(mode), int(bool(per_sweep)), float(t0), float(smdiv),
                                                        *[None] * 8))

    def p_rho_ptr(self, which: int) -> int:
        return int(self.L.amt_domain_p_rho_ptr(self._dom, int(which)) or 0)

    def p_rho_arrays(self):
        """al, p, ph, pm1, alt, c2a, znu, dnw as torch tensors that view the library's device arrays (valid while the stepper
        lives)."""
        import torch
        b, t0 = self.patch.bounds, self.patch.arrays["t_1"]
        out = []
        for which in range(8):
            ptr = self.L.amt_domain_p_rho_ptr(self._dom, which)
            if not ptr:
                raise self._lib.AmtError(self._lib.ERR_PRECONDITION, "the pressure diagnosis is off")
            view = self._lib.DeviceView(self, ptr, b.shape("t" if which < 6 else "dnw"), "<f8" if t0.element_size() == 8 else "<f4")
            out.append(torch.as_tensor(view, device=t0.device))
        return tuple(out)

    def p_rho(self, step: int):
        with self._dev():
            self._lib.check(self.L.amt_domain_p_rho(self._dom, int(step)))

    def set_uv(self, on: bool = True, per_sweep: bool = False, emdiv: float = 0.0, cf1: float = 0.0, cf2: float = 0.0, cf3: float = 0.0):
        """The library allocates ru_tend, rv_tend, pb, php, cqu, cqv, msfux, msfvx, msfvy (``uv_ptr``); off frees them.  With
        ``per_sweep`` the stepper's step calls are refused: the halo exchange of p, al, ph, mu, mudf is not provided."""
        with self._dev():
            self._lib.check(self.L.amt_domain_set_uv(self._dom, int(bool(on)), int(bool(per_sweep)), float(emdiv), float(cf1), float(cf2),
                                                     float(cf3), *[None] * 9))

    def uv_ptr(self, which: int) -> int:
        return int(self.L.amt_domain_uv_ptr(self._dom, int(which)) or 0)

    def uv(self):
        with self._dev():
            self._lib.check(self.L.amt_domain_uv(self._dom))

    def close(self):
        if self._h:
            with self._dev():
                self._fn("destroy")(self._h)
            self._h = self._ct.c_void_p()
        if self._dom:
            self.L.amt_domain_destroy(self._dom)
            self._dom = self._ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _NativeCommStepper(_NativeStepper):
    """The steppers whose halos the library moves itself (RCCL or IPC): whole sweeps in one call."""

    @staticmethod
    def comm_unique_id() -> bytes:
        """Rank 0: a fresh communicator id to hand to every rank (ncclGetUniqueId)."""
        import ctypes
        from . import lib as _lib
        uid = (ctypes.c_char * 128)()
        _lib.check(_lib.load_library().amt_comm_unique_id(uid))
        return bytes(uid)

    def step(self, n_sweeps: int = 1):
        self._call("step", int(n_sweeps))

    def exchange_halos(self):
        self._call("exchange")

    def set_skew_us(self, microseconds: int):
        """Test hook: every later sweep's exchange starts this late on the communication stream (neighbour skew)."""
        self._lib.check(self._fn("set_skew_us")(self._h, int(microseconds)))

    def pull_mode(self) -> str:
        """IPC transport: 'copy engine' or 'fused kernel' (amt_slab_pull_mode / amt_grid_pull_mode); '' with RCCL."""
        return self._fn("pull_mode")(self._h).decode()

    def comm_info(self):
        """(rank, world) as the transport reports them (communicator / ranks attached to the IPC block); (0, 1) without one."""
        r, w = self._ct.c_int(), self._ct.c_int()
        self._lib.check(self._fn("comm_info")(self._h, self._ct.byref(r), self._ct.byref(w)))
        return r.value, w.value


class NativeSlabStepper(_NativeCommStepper):
    """The same j-slab sweep as ``SlabStepper`` driven by the C++ runtime behind the C-ABI
    (``amt_slab_*``, include/amt_advance_mu_t.h section 5): ``ncclSend/ncclRecv`` of the halo rows
    in one RCCL group on a communication stream, the two edge rows behind them on that stream, the
    interior on the patch's stream.  This is the path a Fortran or C host calls
    (fortran/advance_mu_t_slab_driver.f90); Python only hands over pointers.

    ``patch`` holds torch CUDA tensors (they stay the owners: ``amt_domain_wrap``); ``stream`` is
    the torch stream the sweeps are enqueued on; ``unique_id`` are the AMT_UNIQUE_ID_BYTES every rank
    got from rank 0's ``comm_unique_id()`` (None when world == 1 and not loopback).
    ``transport``: "rccl" (ncclSend/ncclRecv), or "ipc" (peer copies between the processes of one node through
    hipIpcMemHandles and a shared-memory mailbox: no RCCL, ranks may share one device).
    Creating it is collective over the ``world`` ranks (ncclCommInitRank / the IPC set-up).
    ``spec_bdy``: every sweep is followed by the boundary-zone update of this rank's own tile (``amt_domain_set_spec_bdy``,
    header section 12; specified / nested domains).
    """

    _HANDLE = "amt_slab"
    _slab = property(lambda self: self._h)

    def __init__(self, patch: Patch, rank: int, world: int, unique_id: Optional[bytes] = None, *,
                 stream=None, overlap: bool = True, variant: int = 0, loopback: bool = False, transport: str = "rccl",
                 cyclic=(False, False), spec_bdy: bool = False, sumflux: int = 0):
        self.rank, self.world = rank, world
        self.cyclic = (bool(cyclic[0]), bool(cyclic[1]))      # AMT_SLAB_CYCLIC_X / _Y: x is a self wrap of the slab, y a torus
        self.below: Optional[int] = rank - 1 if rank > 0 else None
        self.above: Optional[int] = rank + 1 if rank < world - 1 else None
        self._halo_sides = (_S.SIDE_BELOW | _S.SIDE_ABOVE) if loopback else cyclic_sides(0, rank, 1, world, self.cyclic)
        self._open(patch, (rank, world), self.LOOPBACK if loopback else 0, overlap=overlap, stream=stream, variant=variant,
                   spec_bdy=spec_bdy, sumflux=sumflux, transport=transport, unique_id=unique_id)


class NativeGridStepper(_NativeCommStepper):
    """advance_mu_t on patch (ri, rj) of pi x pj driven by the C++ runtime behind the C-ABI (``amt_grid_*``, header section 5b):
    HIP pack / unpack kernels for the strided halo columns, rows and packed columns in ONE exchange (RCCL group or IPC
    pulls), interior cells on the patch's stream beside it, boundary rows and columns behind it on the communication stream.
    Same construction as ``NativeSlabStepper`` (which is its pi = 1 case); rank = rj * pi + ri.
    """

    _grid = property(lambda self: self._h)

    def __init__(self, patch: Patch, ri: int, rj: int, pi: int, pj: int, unique_id: Optional[bytes] = None, *,
                 stream=None, overlap: bool = True, variant: int = 0, loopback: bool = False, transport: str = "rccl",
                 cyclic=(False, False), spec_bdy: bool = False, sumflux: int = 0):
        self.ri, self.rj, self.pi, self.pj = ri, rj, pi, pj
        self.cyclic = (bool(cyclic[0]), bool(cyclic[1]))      # AMT_SLAB_CYCLIC_X / _Y
        self._halo_sides = 15 if loopback else cyclic_sides(ri, rj, pi, pj, self.cyclic)
        self._open(patch, (ri, rj, pi, pj), self.LOOPBACK if loopback else 0, overlap=overlap, stream=stream, variant=variant,
                   spec_bdy=spec_bdy, sumflux=sumflux, transport=transport, unique_id=unique_id)


# ---------------------------------------------------------------------------------------------
# Host-owned halo exchange (include/amt_advance_mu_t.h section 11): the library packs one contiguous
# message per side, the HOST moves the messages (MPI), the library unpacks.
# ---------------------------------------------------------------------------------------------
EXTERNAL_FLAG, HOST_BUFFERS_FLAG = 32, 64       # AMT_SLAB_TRANSPORT_EXTERNAL, AMT_SLAB_EXTERNAL_HOST_BUFFERS
SIDE_ORDER = (_S.SIDE_BELOW, _S.SIDE_ABOVE, _S.SIDE_LEFT, _S.SIDE_RIGHT)      # the order of amt_grid_halo_messages
OPPOSITE_SIDE = {_S.SIDE_BELOW: _S.SIDE_ABOVE, _S.SIDE_ABOVE: _S.SIDE_BELOW, _S.SIDE_LEFT: _S.SIDE_RIGHT, _S.SIDE_RIGHT: _S.SIDE_LEFT}


def halo_layout(bounds, ri: int, rj: int, pi: int, pj: int, cyclic=(False, False)) -> dict:
    """The statement of the message layout: ``{side: {"peer": rank, "send": runs, "recv": runs}}`` for every side of patch
    (ri, rj) of pi x pj that has a neighbour, sides in SIDE_ORDER.  ``runs`` is a list of ``(field, index)``: the message is
    the concatenation, in list order, of ``arrays[field][index]`` flattened in C order -- arrays in the (j, k, i) / (j, i)
    memory layout, every memory level.  Rows: i fastest over ilo..ihi, then k.  Columns: k fastest, then j over jlo..jhi.
    ilo..ihi, jlo..jhi: its..ite, jts..jte; in a cyclic direction the compute window's edges.  ``recv`` names the halo cells
    the message is unpacked into (row jhi+1 / jlo-1, column ihi+1 / ilo-1): what a side sends is what the neighbour's
    opposite side receives."""
    b = bounds
    left, right, below, above, _sends, _recvs = exchange_plan(ri, rj, pi, pj, cyclic)
    c0, c1, r0, r1 = b.its - b.ims, b.ite - b.ims, b.jts - b.jms, b.jte - b.jms
    w0, w1, v0, v1 = _edge_cells(b)
    if cyclic[0]:
        c0, c1 = w0, w1
    if cyclic[1]:
        r0, r1 = v0, v1
    I, J = slice(c0, c1 + 1), slice(r0, r1 + 1)

    def rows(names, r):
        return [(n, (r, slice(None), I) if _S.field_rank(n) == 3 else (r, I)) for n in names]

    def cols(names, c):
        return [(n, (J, slice(None), c) if _S.field_rank(n) == 3 else (J, c)) for n in names]

    out = {}
    if below is not None:
        out[_S.SIDE_BELOW] = dict(peer=below, send=rows(HALO_FROM_ABOVE, r0), recv=rows(HALO_FROM_BELOW, r0 - 1))
    if above is not None:
        out[_S.SIDE_ABOVE] = dict(peer=above, send=rows(HALO_FROM_BELOW, r1), recv=rows(HALO_FROM_ABOVE, r1 + 1))
    if left is not None:
        out[_S.SIDE_LEFT] = dict(peer=left, send=cols(HALO_FROM_RIGHT, c0), recv=cols(HALO_FROM_LEFT, c0 - 1))
    if right is not None:
        out[_S.SIDE_RIGHT] = dict(peer=right, send=cols(HALO_FROM_LEFT, c1), recv=cols(HALO_FROM_RIGHT, c1 + 1))
    return out


class HaloMessageView:
    """One side's messages of an external stepper: ``side`` (synth.SIDE_*), ``peer`` (rank), ``send`` / ``recv`` as byte views
    -- torch uint8 device tensors, or numpy uint8 arrays over page-locked host memory (``on_host``)."""

    def __init__(self, side, peer, send, recv, on_host):
        self.side, self.peer, self.send, self.recv, self.on_host = side, peer, send, recv, on_host


class ExternalGridStepper(_NativeStepper):
    """advance_mu_t on patch (ri, rj) of pi x pj with the HOST as the transport (``AMT_SLAB_TRANSPORT_EXTERNAL``): per sweep
    ``begin()`` (pack + interior), ``halo_wait()``, the host copies every ``send`` into the matching ``recv`` of the peer (an
    MPI host: Isend / Irecv with tag = side), ``end()`` (unpack + boundary cells).  Creation is not collective and needs no
    communicator id; any number of steppers may share a process and a device.  ``host_buffers``: the messages lie in
    page-locked host memory (an MPI that is not GPU-aware).  ``spec_bdy``: ``end()`` is followed by the boundary-zone update of
    this rank's own tile (``amt_domain_set_spec_bdy``; nothing is exchanged for it)."""

    _HANDLE, _SLAB = "amt_grid", False

    def __init__(self, patch: Patch, ri: int, rj: int, pi: int, pj: int, *, cyclic=(False, False), overlap: bool = True,
                 host_buffers: bool = False, stream=None, variant: int = 0, spec_bdy: bool = False, sumflux: int = 0):
        self.ri, self.rj, self.pi, self.pj = ri, rj, pi, pj
        self.rank = rj * pi + ri
        self.cyclic = (bool(cyclic[0]), bool(cyclic[1]))
        self.host_buffers = bool(host_buffers)
        self._halo_sides = cyclic_sides(ri, rj, pi, pj, self.cyclic)
        self._messages = None
        self._open(patch, (rj, pj) if self._SLAB else (ri, rj, pi, pj), EXTERNAL_FLAG | (HOST_BUFFERS_FLAG if host_buffers else 0),
                   overlap=overlap, stream=stream, variant=variant, spec_bdy=spec_bdy, sumflux=sumflux)

    def begin(self):
        """Asynchronous: [self-wrap refresh,] pack, then the interior cells (all of it with ``overlap=False``: nothing)."""
        self._call("step_begin")

    def halo_wait(self):
        """Host wait: this sweep's ``send`` buffers are readable and the ``recv`` buffers may be overwritten."""
        self._call("halo_wait")

    def end(self):
        """Asynchronous; every ``recv`` holds this sweep's message: unpack, then the boundary rows and columns."""
        self._call("step_end")

    def halo_pack(self):
        self._call("halo_pack")

    def halo_unpack(self):
        self._call("halo_unpack")

    def messages(self):
        """The handle's messages (``HaloMessageView``), sides in SIDE_ORDER; made once, the views stay valid until close()."""
        if self._messages is None:
            import numpy as np
            import torch
            ct = self._ct
            raw, n = (self._lib.HaloMessage * 4)(), ct.c_int()
            self._lib.check(self._fn("halo_messages")(self._h, raw, 4, ct.byref(n)))

            def view(ptr, nbytes, on_host):
                if on_host:
                    return np.frombuffer((ct.c_ubyte * nbytes).from_address(ptr), dtype=np.uint8)
                return torch.as_tensor(self._lib.DeviceView(self, ptr, (nbytes,), "|u1"), device=torch.device("cuda", self.device_index))

            with self._dev():
                self._messages = [HaloMessageView(m.side, m.peer, view(m.send, m.send_bytes, m.on_host),
                                                  view(m.recv, m.recv_bytes, m.on_host), bool(m.on_host)) for m in raw[:n.value]]
        return self._messages

    def close(self):
        self._messages = None
        super().close()


class ExternalSlabStepper(ExternalGridStepper):
    """The pi = 1 case through ``amt_slab_*``: j-slab ``rank`` of ``world``."""

    _HANDLE, _SLAB = "amt_slab", True

    def __init__(self, patch: Patch, rank: int, world: int, **kw):
        super().__init__(patch, 0, rank, 1, world, **kw)
