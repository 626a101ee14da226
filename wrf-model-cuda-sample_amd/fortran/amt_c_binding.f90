! amt_c_binding.f90 -- ISO_C_BINDING interfaces of include/amt_advance_mu_t.h.
!
! Arrays cross the boundary as C addresses (c_loc of the first element): the
! C-ABI takes plain pointers and the Fortran-style inclusive bounds unchanged.
MODULE amt_c_binding
   use iso_c_binding
   implicit none

   integer(c_int), parameter :: AMT_OK = 0
   integer(c_int), parameter :: AMT_ERR_PRECONDITION = 2      ! bounds, or a call the handle's settings do not admit
   integer(c_int), parameter :: AMT_ERR_INVALID_ARG = 3       ! a null pointer, a bad id or count
   integer(c_int), parameter :: AMT_ERR_NONFINITE = 7         ! the non-finite guard of header section 10 has a finding
   ! enum amt_variant (amt_*_set_variant, the `variant` argument of amt_advance_mu_t_device_* and its ensemble twin);
   ! AMT_LAUNCH_BESIDE_OTHERS is OR-ed into that argument
   integer(c_int), parameter :: AMT_VARIANT_AUTO = 0, AMT_VARIANT_COLUMN = 1, AMT_VARIANT_MARCH = 2
   integer(c_int), parameter :: AMT_LAUNCH_BESIDE_OTHERS = 256
   ! enum amt_region (amt_domain_field_stats, amt_domain_compare and their ensemble twins)
   integer(c_int), parameter :: AMT_REGION_WINDOW = 0, AMT_REGION_MEMORY = 1

   ! the result records of header section 10; offsets count elements from the member's base
   type, bind(C) :: amt_field_stats
      integer(c_int64_t) :: count, n_nan, n_inf, first_nonfinite
      real(c_double) :: min, max, max_abs, sum
   end type
   type, bind(C) :: amt_field_diff
      integer(c_int64_t) :: count, n_diff, first_diff
      real(c_double) :: max_abs_diff
   end type
   type, bind(C) :: amt_guard_report
      integer(c_int64_t) :: sweeps_checked, sweep
      integer(c_int32_t) :: field, member
      integer(c_int64_t) :: offset, n_nonfinite
   end type
   ! enum amt_slab_flags (amt_slab_create / amt_grid_create)
   integer(c_int), parameter :: AMT_SLAB_NO_OVERLAP = 1, AMT_SLAB_LOOPBACK = 2, AMT_SLAB_TRANSPORT_IPC = 4,  &
                                AMT_SLAB_CYCLIC_X = 8, AMT_SLAB_CYCLIC_Y = 16,                                 &
                                AMT_SLAB_TRANSPORT_EXTERNAL = 32, AMT_SLAB_EXTERNAL_HOST_BUFFERS = 64
   ! one side's messages of a host-owned halo exchange (header section 11): the library owns the buffers, the host moves them
   type, bind(C) :: amt_halo_message
      integer(c_int) :: side, peer                           ! side: AMT_SIDE_* below, also the MPI tag
      type(c_ptr) :: send
      integer(c_size_t) :: send_bytes
      type(c_ptr) :: recv
      integer(c_size_t) :: recv_bytes
      integer(c_int) :: on_host
   end type

   interface
      ! (1) one-shot host drop-ins
      function amt_advance_mu_t_f32(ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv,    &
                                    mudf, t, t_1, t_ave, ft, mu_tend, rdx, rdy, dts, epssm,      &
                                    dnw, fnm, fnp, rdnw, msfuy, msfvx_inv, msftx, msfty,         &
                                    periodic_x, specified, nested,                               &
                                    ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,       &
                                    its, ite, jts, jte, kts, kte) bind(C, name="amt_advance_mu_t_f32") result(rc)
         import :: c_ptr, c_float, c_int
         type(c_ptr), value :: ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv
         type(c_ptr), value :: mudf, t, t_1, t_ave, ft, mu_tend
         real(c_float), value :: rdx, rdy, dts, epssm
         type(c_ptr), value :: dnw, fnm, fnp, rdnw, msfuy, msfvx_inv, msftx, msfty
         integer(c_int), value :: periodic_x, specified, nested
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      function amt_advance_mu_t_f64(ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv,    &
                                    mudf, t, t_1, t_ave, ft, mu_tend, rdx, rdy, dts, epssm,      &
                                    dnw, fnm, fnp, rdnw, msfuy, msfvx_inv, msftx, msfty,         &
                                    periodic_x, specified, nested,                               &
                                    ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,       &
                                    its, ite, jts, jte, kts, kte) bind(C, name="amt_advance_mu_t_f64") result(rc)
         import :: c_ptr, c_double, c_int
         type(c_ptr), value :: ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv
         type(c_ptr), value :: mudf, t, t_1, t_ave, ft, mu_tend
         real(c_double), value :: rdx, rdy, dts, epssm
         type(c_ptr), value :: dnw, fnm, fnp, rdnw, msfuy, msfvx_inv, msftx, msfty
         integer(c_int), value :: periodic_x, specified, nested
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function

      ! page-lock / release a host array so that the one-shot call streams it
      function amt_host_pin(ptr, bytes) bind(C, name="amt_host_pin") result(rc)
         import :: c_ptr, c_size_t, c_int
         type(c_ptr), value :: ptr
         integer(c_size_t), value :: bytes
         integer(c_int) :: rc
      end function
      function amt_host_unpin(ptr) bind(C, name="amt_host_unpin") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: ptr
         integer(c_int) :: rc
      end function
      ! one call, several devices: the one-shot calls of this thread fan their tile's rows jts..jte over n device slots (ids may
      ! repeat), halo rows from the host arrays -- what the reference's own host call does (advance_mu_t_no_async.cu:108-162);
      ! n = 0 turns it off.  AMT_ONESHOT_DEVICES="0,1,2" | "all" in the environment does the same without a call.
      function amt_host_set_devices(n, device_ids) bind(C, name="amt_host_set_devices") result(rc)
         import :: c_int
         integer(c_int), value :: n
         integer(c_int), intent(in) :: device_ids(*)
         integer(c_int) :: rc
      end function
      function amt_host_devices(device_ids, cap) bind(C, name="amt_host_devices") result(n)
         import :: c_int
         integer(c_int), intent(out) :: device_ids(*)
         integer(c_int), value :: cap
         integer(c_int) :: n
      end function
      ! free the device workspace the one-shot calls of this thread keep between calls
      function amt_host_release() bind(C, name="amt_host_release") result(rc)
         import :: c_int
         integer(c_int) :: rc
      end function
      ! residency cache of the one-shot calls of this thread: ww_1, u_1, v_1, t_1, ft stay on the device
      ! between calls (the sub-steps of one Runge-Kutta stage) and go up again only after amt_host_invalidate
      ! (c_null_ptr: all of them -- a new stage); amt_host_cache_check(1): checksum debug mode
      function amt_host_cache_enable(on) bind(C, name="amt_host_cache_enable") result(rc)
         import :: c_int
         integer(c_int), value :: on
         integer(c_int) :: rc
      end function
      function amt_host_cache_check(on) bind(C, name="amt_host_cache_check") result(rc)
         import :: c_int
         integer(c_int), value :: on
         integer(c_int) :: rc
      end function
      function amt_host_invalidate(ptr) bind(C, name="amt_host_invalidate") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: ptr
         integer(c_int) :: rc
      end function
      ! deferred outputs of the one-shot calls of this thread: ww, t, t_ave, mu, muave, muts, mudf (c_null_ptr: all) stay
      ! on the device after a call until amt_host_fetch brings the window's cells down; amt_host_stale: 1 while the device
      ! copy is newer than the host array
      function amt_host_defer(ptr, on) bind(C, name="amt_host_defer") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: ptr
         integer(c_int), value :: on
         integer(c_int) :: rc
      end function
      function amt_host_fetch(ptr) bind(C, name="amt_host_fetch") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: ptr
         integer(c_int) :: rc
      end function
      function amt_host_stale(ptr) bind(C, name="amt_host_stale") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: ptr
         integer(c_int) :: rc
      end function

      ! error text of the calling thread (NUL-terminated C string)
      function amt_last_error() bind(C, name="amt_last_error") result(msg)
         import :: c_ptr
         type(c_ptr) :: msg
      end function
      ! NUL-terminated C strings owned by the library: the build's version line, the text of an amt_status code
      function amt_version() bind(C, name="amt_version") result(msg)
         import :: c_ptr
         type(c_ptr) :: msg
      end function
      function amt_status_string(status) bind(C, name="amt_status_string") result(msg)
         import :: c_ptr, c_int
         integer(c_int), value :: status
         type(c_ptr) :: msg
      end function
      function amt_device_count() bind(C, name="amt_device_count") result(n)
         import :: c_int
         integer(c_int) :: n
      end function

      ! (2) device-resident drop-ins: every array argument is a DEVICE address, the call is enqueued on hip_stream and returns
      ! without synchronising; variant = AMT_VARIANT_* below
      function amt_advance_mu_t_device_f32(hip_stream, variant,                                  &
                                    ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv,    &
                                    mudf, t, t_1, t_ave, ft, mu_tend, rdx, rdy, dts, epssm,      &
                                    dnw, fnm, fnp, rdnw, msfuy, msfvx_inv, msftx, msfty,         &
                                    periodic_x, specified, nested,                               &
                                    ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,       &
                                    its, ite, jts, jte, kts, kte)                                &
            bind(C, name="amt_advance_mu_t_device_f32") result(rc)
         import :: c_ptr, c_float, c_int
         type(c_ptr), value :: hip_stream                    ! hipStream_t, c_null_ptr = the default stream
         integer(c_int), value :: variant
         type(c_ptr), value :: ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv      ! DEVICE addresses
         type(c_ptr), value :: mudf, t, t_1, t_ave, ft, mu_tend
         real(c_float), value :: rdx, rdy, dts, epssm
         type(c_ptr), value :: dnw, fnm, fnp, rdnw, msfuy, msfvx_inv, msftx, msfty
         integer(c_int), value :: periodic_x, specified, nested
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      function amt_advance_mu_t_device_f64(hip_stream, variant,                                  &
                                    ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv,    &
                                    mudf, t, t_1, t_ave, ft, mu_tend, rdx, rdy, dts, epssm,      &
                                    dnw, fnm, fnp, rdnw, msfuy, msfvx_inv, msftx, msfty,         &
                                    periodic_x, specified, nested,                               &
                                    ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,       &
                                    its, ite, jts, jte, kts, kte)                                &
            bind(C, name="amt_advance_mu_t_device_f64") result(rc)
         import :: c_ptr, c_double, c_int
         type(c_ptr), value :: hip_stream                    ! hipStream_t, c_null_ptr = the default stream
         integer(c_int), value :: variant
         type(c_ptr), value :: ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv      ! DEVICE addresses
         type(c_ptr), value :: mudf, t, t_1, t_ave, ft, mu_tend
         real(c_double), value :: rdx, rdy, dts, epssm
         type(c_ptr), value :: dnw, fnm, fnp, rdnw, msfuy, msfvx_inv, msftx, msfty
         integer(c_int), value :: periodic_x, specified, nested
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      ! the compute window the routine updates for these flags and bounds (host arithmetic, no device)
      function amt_compute_window(periodic_x, specified, nested, ids, ide, jds, jde, its, ite, jts, jte, kts, kte,      &
                                  i_start, i_end, j_start, j_end, k_start, k_end) bind(C, name="amt_compute_window") result(rc)
         import :: c_int
         integer(c_int), value :: periodic_x, specified, nested, ids, ide, jds, jde, its, ite, jts, jte, kts, kte
         integer(c_int) :: i_start, i_end, j_start, j_end, k_start, k_end
         integer(c_int) :: rc
      end function

      ! (3) resident domain handle
      function amt_domain_create(handle, dtype_bytes, periodic_x, specified, nested,             &
                                 ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,          &
                                 its, ite, jts, jte, kts, kte) bind(C, name="amt_domain_create") result(rc)
         import :: c_ptr, c_int
         type(c_ptr) :: handle                      ! amt_domain **
         integer(c_int), value :: dtype_bytes, periodic_x, specified, nested
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      ! over device arrays the caller owns: fields(0:25) = the device addresses in amt_field order; nothing is copied or freed
      function amt_domain_wrap(handle, dtype_bytes, periodic_x, specified, nested,               &
                               ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,            &
                               its, ite, jts, jte, kts, kte, fields, hip_stream) bind(C, name="amt_domain_wrap") result(rc)
         import :: c_ptr, c_int
         type(c_ptr) :: handle                      ! amt_domain **
         integer(c_int), value :: dtype_bytes, periodic_x, specified, nested
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         type(c_ptr), intent(in) :: fields(*)
         type(c_ptr), value :: hip_stream           ! c_null_ptr: a stream of the handle's own
         integer(c_int) :: rc
      end function
      function amt_domain_set_variant(handle, variant) bind(C, name="amt_domain_set_variant") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: variant
         integer(c_int) :: rc
      end function
      function amt_domain_field_ptr(handle, field) bind(C, name="amt_domain_field_ptr") result(ptr)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: field
         type(c_ptr) :: ptr                         ! device address, c_null_ptr on error
      end function
      function amt_domain_stream(handle) bind(C, name="amt_domain_stream") result(stream)
         import :: c_ptr
         type(c_ptr), value :: handle
         type(c_ptr) :: stream                      ! hipStream_t
      end function
      function amt_domain_destroy(handle) bind(C, name="amt_domain_destroy") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int) :: rc
      end function
      function amt_domain_set_scalars(handle, rdx, rdy, dts, epssm) bind(C, name="amt_domain_set_scalars") result(rc)
         import :: c_ptr, c_int, c_double
         type(c_ptr), value :: handle
         real(c_double), value :: rdx, rdy, dts, epssm
         integer(c_int) :: rc
      end function
      function amt_domain_upload(handle, field, host) bind(C, name="amt_domain_upload") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle, host
         integer(c_int), value :: field
         integer(c_int) :: rc
      end function
      function amt_domain_download(handle, field, host) bind(C, name="amt_domain_download") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle, host
         integer(c_int), value :: field
         integer(c_int) :: rc
      end function
      ! rows j_lo..j_hi (Fortran indices inside jms:jme) of a rank-3 or rank-2 field; host holds exactly those rows
      function amt_domain_upload_rows(handle, field, j_lo, j_hi, host) bind(C, name="amt_domain_upload_rows") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle, host
         integer(c_int), value :: field, j_lo, j_hi
         integer(c_int) :: rc
      end function
      function amt_domain_download_rows(handle, field, j_lo, j_hi, host) bind(C, name="amt_domain_download_rows") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle, host
         integer(c_int), value :: field, j_lo, j_hi
         integer(c_int) :: rc
      end function
      ! allocations timed by the last placement sampling of this handle (0: none) and their sweep times
      function amt_domain_placement(handle, ms_per_try, cap) bind(C, name="amt_domain_placement") result(n)
         import :: c_ptr, c_int, c_float
         type(c_ptr), value :: handle
         real(c_float) :: ms_per_try(*)
         integer(c_int), value :: cap
         integer(c_int) :: n
      end function
      function amt_domain_step(handle, n_sweeps) bind(C, name="amt_domain_step") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: n_sweeps
         integer(c_int) :: rc
      end function
      ! placement tuning: the handle's arrays allocated `tries` times, two sweeps timed on each set, the fastest kept;
      ! contents unchanged; ms_per_try receives the sweep time of every set
      function amt_domain_tune_placement(handle, tries, ms_per_try) bind(C, name="amt_domain_tune_placement") result(rc)
         import :: c_ptr, c_int, c_float
         type(c_ptr), value :: handle
         integer(c_int), value :: tries
         real(c_float) :: ms_per_try(*)
         integer(c_int) :: rc
      end function
      function amt_domain_step_timed(handle, n_sweeps, ms_total) bind(C, name="amt_domain_step_timed") result(rc)
         import :: c_ptr, c_int, c_float
         type(c_ptr), value :: handle
         integer(c_int), value :: n_sweeps
         real(c_float) :: ms_total
         integer(c_int) :: rc
      end function
      function amt_domain_sync(handle) bind(C, name="amt_domain_sync") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int) :: rc
      end function

      function amt_domain_fill_synthetic(handle, seed, gi0, gk0, gj0, gidim, gkdim, gjdim)        &
            bind(C, name="amt_domain_fill_synthetic") result(rc)
         import :: c_ptr, c_int, c_int64_t, c_long
         type(c_ptr), value :: handle
         integer(c_int64_t), value :: seed
         integer(c_long), value :: gi0, gk0, gj0, gidim, gkdim, gjdim
         integer(c_int) :: rc
      end function

      ! the fields of field_mask only (bit f = field id f; AMT_EXCHANGED_FIELDS below): the stand-in for advance_uv
      ! rewriting u, v before every advance_mu_t call
      function amt_domain_fill_fields(handle, field_mask, seed, gi0, gk0, gj0, gidim, gkdim, gjdim) &
            bind(C, name="amt_domain_fill_fields") result(rc)
         import :: c_ptr, c_int, c_int64_t, c_long
         type(c_ptr), value :: handle
         integer(c_int64_t), value :: field_mask, seed
         integer(c_long), value :: gi0, gk0, gj0, gidim, gkdim, gjdim
         integer(c_int) :: rc
      end function

      ! NaN into what the stencil reads from a neighbour: sides = sum of AMT_SIDE_BELOW / ABOVE / LEFT / RIGHT
      function amt_domain_poison_halos(handle, sides) bind(C, name="amt_domain_poison_halos") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: sides
         integer(c_int) :: rc
      end function

      ! ---- j-slabs over several GPUs, one process per GPU (RCCL halos) ----
      function amt_set_device(device) bind(C, name="amt_set_device") result(rc)
         import :: c_int
         integer(c_int), value :: device
         integer(c_int) :: rc
      end function
      ! rank 0: a fresh communicator id (128 bytes) to hand to every rank, for hosts that broadcast it themselves (MPI_Bcast)
      function amt_comm_unique_id(id_out) bind(C, name="amt_comm_unique_id") result(rc)
         import :: c_char, c_int
         character(kind=c_char), intent(out) :: id_out(128)
         integer(c_int) :: rc
      end function
      ! a value all processes of one launch agree on and two launches do not (an unsigned 64-bit pattern)
      function amt_comm_launch_nonce() bind(C, name="amt_comm_launch_nonce") result(nonce)
         import :: c_int64_t
         integer(c_int64_t) :: nonce
      end function
      function amt_comm_rendezvous_file(path, nonce, rank, world, timeout_s, id_out)              &
            bind(C, name="amt_comm_rendezvous_file") result(rc)
         import :: c_char, c_int, c_double, c_int64_t
         character(kind=c_char), intent(in) :: path(*)      ! NUL-terminated
         integer(c_int64_t), value :: nonce                 ! 0: amt_comm_launch_nonce()
         integer(c_int), value :: rank, world
         real(c_double), value :: timeout_s
         character(kind=c_char), intent(out) :: id_out(128)
         integer(c_int) :: rc
      end function
      function amt_slab_create(slab, domain, rank, world, unique_id, flags) bind(C, name="amt_slab_create") result(rc)
         import :: c_ptr, c_int
         type(c_ptr) :: slab                         ! amt_slab **
         type(c_ptr), value :: domain, unique_id     ! unique_id may be c_null_ptr when world == 1
         integer(c_int), value :: rank, world, flags
         integer(c_int) :: rc
      end function
      function amt_slab_destroy(slab) bind(C, name="amt_slab_destroy") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: slab
         integer(c_int) :: rc
      end function
      function amt_slab_exchange(slab) bind(C, name="amt_slab_exchange") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: slab
         integer(c_int) :: rc
      end function
      ! NUL-terminated C string: "rccl", "ipc", "external" or "none" (no neighbour)
      function amt_slab_transport(slab) bind(C, name="amt_slab_transport") result(msg)
         import :: c_ptr
         type(c_ptr), value :: slab
         type(c_ptr) :: msg
      end function
      function amt_slab_step(slab, n_sweeps) bind(C, name="amt_slab_step") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: slab
         integer(c_int), value :: n_sweeps
         integer(c_int) :: rc
      end function
      function amt_slab_step_timed(slab, n_sweeps, ms_total) bind(C, name="amt_slab_step_timed") result(rc)
         import :: c_ptr, c_int, c_float
         type(c_ptr), value :: slab
         integer(c_int), value :: n_sweeps
         real(c_float) :: ms_total
         integer(c_int) :: rc
      end function
      function amt_slab_sync(slab) bind(C, name="amt_slab_sync") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: slab
         integer(c_int) :: rc
      end function
      function amt_slab_halo_bytes(slab) bind(C, name="amt_slab_halo_bytes") result(n)
         import :: c_ptr, c_long
         type(c_ptr), value :: slab
         integer(c_long) :: n
      end function
      function amt_slab_comm_info(slab, rank, world) bind(C, name="amt_slab_comm_info") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: slab
         integer(c_int) :: rank, world
         integer(c_int) :: rc
      end function
      function amt_slab_barrier(slab) bind(C, name="amt_slab_barrier") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: slab
         integer(c_int) :: rc
      end function
      function amt_slab_max(slab, x) bind(C, name="amt_slab_max") result(rc)
         import :: c_ptr, c_int, c_double
         type(c_ptr), value :: slab
         real(c_double) :: x                                 ! in: this rank's value, out: the maximum
         integer(c_int) :: rc
      end function

      ! (5b) patches in i and j: rank = rj * pi + ri of pi x pj (amt_slab_* is the pi = 1 case)
      function amt_grid_create(grid, domain, ri, rj, pi, pj, unique_id, flags) bind(C, name="amt_grid_create") result(rc)
         import :: c_ptr, c_int
         type(c_ptr) :: grid                         ! amt_grid **
         type(c_ptr), value :: domain, unique_id     ! unique_id may be c_null_ptr when pi * pj == 1
         integer(c_int), value :: ri, rj, pi, pj, flags
         integer(c_int) :: rc
      end function
      function amt_grid_destroy(grid) bind(C, name="amt_grid_destroy") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: grid
         integer(c_int) :: rc
      end function
      function amt_grid_exchange(grid) bind(C, name="amt_grid_exchange") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: grid
         integer(c_int) :: rc
      end function
      function amt_grid_transport(grid) bind(C, name="amt_grid_transport") result(msg)
         import :: c_ptr
         type(c_ptr), value :: grid
         type(c_ptr) :: msg
      end function
      function amt_grid_step(grid, n_sweeps) bind(C, name="amt_grid_step") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: grid
         integer(c_int), value :: n_sweeps
         integer(c_int) :: rc
      end function
      function amt_grid_step_timed(grid, n_sweeps, ms_total) bind(C, name="amt_grid_step_timed") result(rc)
         import :: c_ptr, c_int, c_float
         type(c_ptr), value :: grid
         integer(c_int), value :: n_sweeps
         real(c_float) :: ms_total
         integer(c_int) :: rc
      end function
      function amt_grid_sync(grid) bind(C, name="amt_grid_sync") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: grid
         integer(c_int) :: rc
      end function
      function amt_grid_halo_bytes(grid) bind(C, name="amt_grid_halo_bytes") result(n)
         import :: c_ptr, c_long
         type(c_ptr), value :: grid
         integer(c_long) :: n
      end function
      function amt_grid_comm_info(grid, rank, world) bind(C, name="amt_grid_comm_info") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: grid
         integer(c_int) :: rank, world
         integer(c_int) :: rc
      end function
      function amt_grid_barrier(grid) bind(C, name="amt_grid_barrier") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: grid
         integer(c_int) :: rc
      end function
      function amt_grid_max(grid, x) bind(C, name="amt_grid_max") result(rc)
         import :: c_ptr, c_int, c_double
         type(c_ptr), value :: grid
         real(c_double) :: x                                 ! in: this rank's value, out: the maximum
         integer(c_int) :: rc
      end function
      ! (11) host-owned halo exchange (AMT_SLAB_TRANSPORT_EXTERNAL): per sweep step_begin, halo_wait, the host's sends and
      !      receives (tag = side), step_end
      function amt_grid_halo_messages(grid, out, cap, n) bind(C, name="amt_grid_halo_messages") result(rc)
         import :: c_ptr, c_int, amt_halo_message
         type(c_ptr), value :: grid
         type(amt_halo_message) :: out(*)                    ! room for cap messages (at most 4)
         integer(c_int), value :: cap
         integer(c_int) :: n
         integer(c_int) :: rc
      end function
      function amt_grid_step_begin(grid) bind(C, name="amt_grid_step_begin") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: grid
         integer(c_int) :: rc
      end function
      function amt_grid_halo_wait(grid) bind(C, name="amt_grid_halo_wait") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: grid
         integer(c_int) :: rc
      end function
      function amt_grid_step_end(grid) bind(C, name="amt_grid_step_end") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: grid
         integer(c_int) :: rc
      end function
      function amt_grid_halo_pack(grid) bind(C, name="amt_grid_halo_pack") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: grid
         integer(c_int) :: rc
      end function
      function amt_grid_halo_unpack(grid) bind(C, name="amt_grid_halo_unpack") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: grid
         integer(c_int) :: rc
      end function
      function amt_slab_halo_messages(slab, out, cap, n) bind(C, name="amt_slab_halo_messages") result(rc)
         import :: c_ptr, c_int, amt_halo_message
         type(c_ptr), value :: slab
         type(amt_halo_message) :: out(*)                    ! room for cap messages (at most 4)
         integer(c_int), value :: cap
         integer(c_int) :: n
         integer(c_int) :: rc
      end function
      function amt_slab_step_begin(slab) bind(C, name="amt_slab_step_begin") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: slab
         integer(c_int) :: rc
      end function
      function amt_slab_halo_wait(slab) bind(C, name="amt_slab_halo_wait") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: slab
         integer(c_int) :: rc
      end function
      function amt_slab_step_end(slab) bind(C, name="amt_slab_step_end") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: slab
         integer(c_int) :: rc
      end function
      function amt_slab_halo_pack(slab) bind(C, name="amt_slab_halo_pack") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: slab
         integer(c_int) :: rc
      end function
      function amt_slab_halo_unpack(slab) bind(C, name="amt_slab_halo_unpack") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: slab
         integer(c_int) :: rc
      end function
      function amt_halo_plan(dtype_bytes, periodic_x, specified, nested, ids, ide, jds, jde, kde, ims, ime, jms, jme,   &
                             kms, kme, its, ite, jts, jte, kts, kte, ri, rj, pi, pj, flags, out, cap, n)             &
                             bind(C, name="amt_halo_plan") result(rc)
         import :: c_int, amt_halo_message
         integer(c_int), value :: dtype_bytes, periodic_x, specified, nested, ids, ide, jds, jde, kde, ims, ime, jms, jme
         integer(c_int), value :: kms, kme, its, ite, jts, jte, kts, kte, ri, rj, pi, pj, flags, cap
         type(amt_halo_message) :: out(*)
         integer(c_int) :: n
         integer(c_int) :: rc
      end function

      ! (4) synthetic inputs
      function amt_synth_fill_host(field, dtype_bytes, dst, seed, idim, kdim, jdim, gi0, gk0, gj0, &
                                   gidim, gkdim, gjdim) bind(C, name="amt_synth_fill_host") result(rc)
         import :: c_ptr, c_int, c_long, c_int64_t
         integer(c_int), value :: field, dtype_bytes
         type(c_ptr), value :: dst
         integer(c_int64_t), value :: seed
         integer(c_long), value :: idim, kdim, jdim, gi0, gk0, gj0, gidim, gkdim, gjdim
         integer(c_int) :: rc
      end function

      ! the same generator on the device: dst_device is a DEVICE address, asynchronous on hip_stream; identical bits
      function amt_synth_fill_device(hip_stream, field, dtype_bytes, dst_device, seed, idim, kdim, jdim, gi0, gk0, gj0, &
                                     gidim, gkdim, gjdim) bind(C, name="amt_synth_fill_device") result(rc)
         import :: c_ptr, c_int, c_long, c_int64_t
         type(c_ptr), value :: hip_stream
         integer(c_int), value :: field, dtype_bytes
         type(c_ptr), value :: dst_device
         integer(c_int64_t), value :: seed
         integer(c_long), value :: idim, kdim, jdim, gi0, gk0, gj0, gidim, gkdim, gjdim
         integer(c_int) :: rc
      end function
      ! rows per workgroup of a single patch's launch (host arithmetic; amt_march_rows_for_members with members = 1)
      function amt_march_rows_for(ntile_i, nj, cus, max_rows, wbytes, hl) bind(C, name="amt_march_rows_for") result(rows)
         import :: c_int, c_long
         integer(c_long), value :: ntile_i, max_rows
         integer(c_int), value :: nj, cus, wbytes, hl
         integer(c_int) :: rows
      end function

      ! (8) ensembles: `members` patches of one shape, every 3-D and 2-D array with one more, slowest, dimension --
      ! u(ims:ime, kms:kme, jms:jme, 1:members), mu(ims:ime, jms:jme, 1:members) -- bounds, flags, scalars and the four 1-D
      ! metric arrays shared; ONE launch per sweep
      function amt_advance_mu_t_ensemble_device_f32(hip_stream, variant, members,                     &
                                    ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv,    &
                                    mudf, t, t_1, t_ave, ft, mu_tend, rdx, rdy, dts, epssm,      &
                                    dnw, fnm, fnp, rdnw, msfuy, msfvx_inv, msftx, msfty,         &
                                    periodic_x, specified, nested,                               &
                                    ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,       &
                                    its, ite, jts, jte, kts, kte)                                &
            bind(C, name="amt_advance_mu_t_ensemble_device_f32") result(rc)
         import :: c_ptr, c_float, c_int
         type(c_ptr), value :: hip_stream                    ! hipStream_t, c_null_ptr = the default stream
         integer(c_int), value :: variant, members
         type(c_ptr), value :: ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv      ! DEVICE addresses, member-stacked
         type(c_ptr), value :: mudf, t, t_1, t_ave, ft, mu_tend
         real(c_float), value :: rdx, rdy, dts, epssm
         type(c_ptr), value :: dnw, fnm, fnp, rdnw, msfuy, msfvx_inv, msftx, msfty           ! dnw .. rdnw: shared, kdim elements
         integer(c_int), value :: periodic_x, specified, nested
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      function amt_advance_mu_t_ensemble_device_f64(hip_stream, variant, members,                     &
                                    ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv,    &
                                    mudf, t, t_1, t_ave, ft, mu_tend, rdx, rdy, dts, epssm,      &
                                    dnw, fnm, fnp, rdnw, msfuy, msfvx_inv, msftx, msfty,         &
                                    periodic_x, specified, nested,                               &
                                    ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,       &
                                    its, ite, jts, jte, kts, kte)                                &
            bind(C, name="amt_advance_mu_t_ensemble_device_f64") result(rc)
         import :: c_ptr, c_double, c_int
         type(c_ptr), value :: hip_stream                    ! hipStream_t, c_null_ptr = the default stream
         integer(c_int), value :: variant, members
         type(c_ptr), value :: ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv      ! DEVICE addresses, member-stacked
         type(c_ptr), value :: mudf, t, t_1, t_ave, ft, mu_tend
         real(c_double), value :: rdx, rdy, dts, epssm
         type(c_ptr), value :: dnw, fnm, fnp, rdnw, msfuy, msfvx_inv, msftx, msfty           ! dnw .. rdnw: shared, kdim elements
         integer(c_int), value :: periodic_x, specified, nested
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      function amt_ensemble_create(handle, members, dtype_bytes, periodic_x, specified, nested,  &
                                   ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,        &
                                   its, ite, jts, jte, kts, kte) bind(C, name="amt_ensemble_create") result(rc)
         import :: c_ptr, c_int
         type(c_ptr) :: handle                      ! amt_ensemble **
         integer(c_int), value :: members, dtype_bytes, periodic_x, specified, nested
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      ! over device arrays the caller owns: fields(0:25) = the bases of the member-stacked arrays in amt_field order
      function amt_ensemble_wrap(handle, members, dtype_bytes, periodic_x, specified, nested,    &
                                 ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,          &
                                 its, ite, jts, jte, kts, kte, fields, hip_stream) bind(C, name="amt_ensemble_wrap") result(rc)
         import :: c_ptr, c_int
         type(c_ptr) :: handle                      ! amt_ensemble **
         integer(c_int), value :: members, dtype_bytes, periodic_x, specified, nested
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         type(c_ptr), intent(in) :: fields(*)
         type(c_ptr), value :: hip_stream           ! c_null_ptr: a stream of the handle's own
         integer(c_int) :: rc
      end function
      function amt_ensemble_destroy(handle) bind(C, name="amt_ensemble_destroy") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int) :: rc
      end function
      function amt_ensemble_set_scalars(handle, rdx, rdy, dts, epssm) bind(C, name="amt_ensemble_set_scalars") result(rc)
         import :: c_ptr, c_int, c_double
         type(c_ptr), value :: handle
         real(c_double), value :: rdx, rdy, dts, epssm
         integer(c_int) :: rc
      end function
      function amt_ensemble_set_variant(handle, variant) bind(C, name="amt_ensemble_set_variant") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: variant
         integer(c_int) :: rc
      end function
      function amt_ensemble_members(handle) bind(C, name="amt_ensemble_members") result(n)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int) :: n
      end function
      ! ONE member (0-based) of a field; host holds that member in the single-patch layout (ims:ime[,kms:kme],jms:jme)
      function amt_ensemble_upload_member(handle, field, member, host) bind(C, name="amt_ensemble_upload_member") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle, host
         integer(c_int), value :: field, member
         integer(c_int) :: rc
      end function
      function amt_ensemble_download_member(handle, field, member, host) bind(C, name="amt_ensemble_download_member") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle, host
         integer(c_int), value :: field, member
         integer(c_int) :: rc
      end function
      ! member m as amt_domain_fill_synthetic(seed + m, ...) fills a single patch
      function amt_ensemble_fill_synthetic(handle, seed, gi0, gk0, gj0, gidim, gkdim, gjdim)      &
            bind(C, name="amt_ensemble_fill_synthetic") result(rc)
         import :: c_ptr, c_int, c_int64_t, c_long
         type(c_ptr), value :: handle
         integer(c_int64_t), value :: seed
         integer(c_long), value :: gi0, gk0, gj0, gidim, gkdim, gjdim
         integer(c_int) :: rc
      end function
      function amt_ensemble_step(handle, n_sweeps) bind(C, name="amt_ensemble_step") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: n_sweeps
         integer(c_int) :: rc
      end function
      function amt_ensemble_step_timed(handle, n_sweeps, ms_total) bind(C, name="amt_ensemble_step_timed") result(rc)
         import :: c_ptr, c_int, c_float
         type(c_ptr), value :: handle
         integer(c_int), value :: n_sweeps
         real(c_float) :: ms_total
         integer(c_int) :: rc
      end function
      function amt_ensemble_sync(handle) bind(C, name="amt_ensemble_sync") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int) :: rc
      end function
      function amt_ensemble_field_ptr(handle, field) bind(C, name="amt_ensemble_field_ptr") result(ptr)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: field
         type(c_ptr) :: ptr
      end function
      function amt_ensemble_stream(handle) bind(C, name="amt_ensemble_stream") result(stream)
         import :: c_ptr
         type(c_ptr), value :: handle
         type(c_ptr) :: stream
      end function
      ! rows per workgroup of an ensemble launch (host arithmetic; members = 1: the single patch's)
      function amt_march_rows_for_members(ntile_i, members, nj, cus, max_rows, wbytes, hl)        &
            bind(C, name="amt_march_rows_for_members") result(rows)
         import :: c_int, c_long
         integer(c_long), value :: ntile_i, max_rows
         integer(c_int), value :: members, nj, cus, wbytes, hl
         integer(c_int) :: rows
      end function
      ! cyclic (periodic) lateral boundaries (header section 9): axes = AMT_CYCLIC_X, AMT_CYCLIC_Y or their sum.  Pointer level, for
      ! hosts that keep their own device arrays (members = 1 for a single patch); asynchronous on hip_stream
      function amt_cyclic_fill_device_f32(hip_stream, axes, members, u, u_1, v, v_1, t_1, muu, muv, msfuy, msfvx_inv,   &
                                          periodic_x, specified, nested,                                                &
                                          ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,                        &
                                          its, ite, jts, jte, kts, kte) bind(C, name="amt_cyclic_fill_device_f32") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: hip_stream
         integer(c_int), value :: axes, members
         type(c_ptr), value :: u, u_1, v, v_1, t_1, muu, muv, msfuy, msfvx_inv      ! device pointers
         integer(c_int), value :: periodic_x, specified, nested
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      function amt_cyclic_fill_device_f64(hip_stream, axes, members, u, u_1, v, v_1, t_1, muu, muv, msfuy, msfvx_inv,   &
                                          periodic_x, specified, nested,                                                &
                                          ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,                        &
                                          its, ite, jts, jte, kts, kte) bind(C, name="amt_cyclic_fill_device_f64") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: hip_stream
         integer(c_int), value :: axes, members
         type(c_ptr), value :: u, u_1, v, v_1, t_1, muu, muv, msfuy, msfvx_inv      ! device pointers
         integer(c_int), value :: periodic_x, specified, nested
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      ! one refresh now, on the handle's stream
      function amt_domain_cyclic_fill(handle, axes) bind(C, name="amt_domain_cyclic_fill") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: axes
         integer(c_int) :: rc
      end function
      ! 0 = off; otherwise every sweep of amt_domain_step / amt_domain_step_timed is preceded by a refresh
      function amt_domain_set_cyclic(handle, axes) bind(C, name="amt_domain_set_cyclic") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: axes
         integer(c_int) :: rc
      end function
      function amt_domain_cyclic(handle) bind(C, name="amt_domain_cyclic") result(axes)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int) :: axes
      end function
      function amt_ensemble_cyclic_fill(handle, axes) bind(C, name="amt_ensemble_cyclic_fill") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: axes
         integer(c_int) :: rc
      end function
      function amt_ensemble_set_cyclic(handle, axes) bind(C, name="amt_ensemble_set_cyclic") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: axes
         integer(c_int) :: rc
      end function
      function amt_ensemble_cyclic(handle) bind(C, name="amt_ensemble_cyclic") result(axes)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int) :: axes
      end function
      ! (10) statistics, bit comparison and the non-finite guard.  Pointer level: a, b are device pointers, out is a HOST array
      ! of `members` records; the call waits for hip_stream
      function amt_stats_device_f32(hip_stream, a, rank, members, ims, ime, jms, jme, kms, kme,                         &
                                    i0, i1, k0, k1, j0, j1, out) bind(C, name="amt_stats_device_f32") result(rc)
         import :: c_ptr, c_int, amt_field_stats
         type(c_ptr), value :: hip_stream, a
         integer(c_int), value :: rank, members, ims, ime, jms, jme, kms, kme, i0, i1, k0, k1, j0, j1
         type(amt_field_stats), intent(inout) :: out(*)
         integer(c_int) :: rc
      end function
      function amt_stats_device_f64(hip_stream, a, rank, members, ims, ime, jms, jme, kms, kme,                         &
                                    i0, i1, k0, k1, j0, j1, out) bind(C, name="amt_stats_device_f64") result(rc)
         import :: c_ptr, c_int, amt_field_stats
         type(c_ptr), value :: hip_stream, a
         integer(c_int), value :: rank, members, ims, ime, jms, jme, kms, kme, i0, i1, k0, k1, j0, j1
         type(amt_field_stats), intent(inout) :: out(*)
         integer(c_int) :: rc
      end function
      function amt_compare_device_f32(hip_stream, a, b, rank, members, ims, ime, jms, jme, kms, kme,                    &
                                      i0, i1, k0, k1, j0, j1, out) bind(C, name="amt_compare_device_f32") result(rc)
         import :: c_ptr, c_int, amt_field_diff
         type(c_ptr), value :: hip_stream, a, b
         integer(c_int), value :: rank, members, ims, ime, jms, jme, kms, kme, i0, i1, k0, k1, j0, j1
         type(amt_field_diff), intent(inout) :: out(*)
         integer(c_int) :: rc
      end function
      function amt_compare_device_f64(hip_stream, a, b, rank, members, ims, ime, jms, jme, kms, kme,                    &
                                      i0, i1, k0, k1, j0, j1, out) bind(C, name="amt_compare_device_f64") result(rc)
         import :: c_ptr, c_int, amt_field_diff
         type(c_ptr), value :: hip_stream, a, b
         integer(c_int), value :: rank, members, ims, ime, jms, jme, kms, kme, i0, i1, k0, k1, j0, j1
         type(amt_field_diff), intent(inout) :: out(*)
         integer(c_int) :: rc
      end function
      ! handle level: region = AMT_REGION_WINDOW or AMT_REGION_MEMORY; an ensemble fills one record per member
      function amt_domain_field_stats(handle, field, region, out) bind(C, name="amt_domain_field_stats") result(rc)
         import :: c_ptr, c_int, amt_field_stats
         type(c_ptr), value :: handle
         integer(c_int), value :: field, region
         type(amt_field_stats), intent(inout) :: out(*)
         integer(c_int) :: rc
      end function
      function amt_ensemble_field_stats(handle, field, region, out) bind(C, name="amt_ensemble_field_stats") result(rc)
         import :: c_ptr, c_int, amt_field_stats
         type(c_ptr), value :: handle
         integer(c_int), value :: field, region
         type(amt_field_stats), intent(inout) :: out(*)
         integer(c_int) :: rc
      end function
      function amt_domain_compare(handle_a, handle_b, field, region, out) bind(C, name="amt_domain_compare") result(rc)
         import :: c_ptr, c_int, amt_field_diff
         type(c_ptr), value :: handle_a, handle_b
         integer(c_int), value :: field, region
         type(amt_field_diff), intent(inout) :: out(*)
         integer(c_int) :: rc
      end function
      function amt_ensemble_compare(handle_a, handle_b, field, region, out) bind(C, name="amt_ensemble_compare") result(rc)
         import :: c_ptr, c_int, amt_field_diff
         type(c_ptr), value :: handle_a, handle_b
         integer(c_int), value :: field, region
         type(amt_field_diff), intent(inout) :: out(*)
         integer(c_int) :: rc
      end function
      ! every = 0: off; n >= 1: ww, t and mu are checked after every n-th sweep of amt_*_step; a finding makes amt_*_sync,
      ! amt_*_step_timed and the next amt_*_step return AMT_ERR_NONFINITE
      function amt_domain_set_guard(handle, every) bind(C, name="amt_domain_set_guard") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: every
         integer(c_int) :: rc
      end function
      function amt_ensemble_set_guard(handle, every) bind(C, name="amt_ensemble_set_guard") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: every
         integer(c_int) :: rc
      end function
      function amt_domain_guard_report(handle, out) bind(C, name="amt_domain_guard_report") result(rc)
         import :: c_ptr, c_int, amt_guard_report
         type(c_ptr), value :: handle
         type(amt_guard_report), intent(inout) :: out
         integer(c_int) :: rc
      end function
      function amt_ensemble_guard_report(handle, out) bind(C, name="amt_ensemble_guard_report") result(rc)
         import :: c_ptr, c_int, amt_guard_report
         type(c_ptr), value :: handle
         type(amt_guard_report), intent(inout) :: out
         integer(c_int) :: rc
      end function
      ! (12) specified / nested lateral boundaries: the boundary-zone update t += dts*ft, mu += dts*mu_tend, muts += dts*mu_tend
      ! over the tile's cells outside the compute window (WRF: three spec_bdyupdate calls behind every advance_mu_t call).
      ! Pointer level (members = 1 for a single patch), asynchronous on hip_stream
      function amt_spec_bdy_update_device_f32(hip_stream, members, t, ft, mu, muts, mu_tend, dts,                          &
                                              periodic_x, specified, nested,                                            &
                                              ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,                    &
                                              its, ite, jts, jte, kts, kte) bind(C, name="amt_spec_bdy_update_device_f32") result(rc)
         import :: c_ptr, c_int, c_float
         type(c_ptr), value :: hip_stream
         integer(c_int), value :: members
         type(c_ptr), value :: t, ft, mu, muts, mu_tend                              ! device pointers
         real(c_float), value :: dts
         integer(c_int), value :: periodic_x, specified, nested
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      function amt_spec_bdy_update_device_f64(hip_stream, members, t, ft, mu, muts, mu_tend, dts,                          &
                                              periodic_x, specified, nested,                                            &
                                              ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,                    &
                                              its, ite, jts, jte, kts, kte) bind(C, name="amt_spec_bdy_update_device_f64") result(rc)
         import :: c_ptr, c_int, c_double
         type(c_ptr), value :: hip_stream
         integer(c_int), value :: members
         type(c_ptr), value :: t, ft, mu, muts, mu_tend                              ! device pointers
         real(c_double), value :: dts
         integer(c_int), value :: periodic_x, specified, nested
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      ! one update now on the handle's stream; set: 1 = every sweep of the handle's stepping (amt_domain_step, amt_slab_step,
      ! amt_grid_step, amt_*_step_end ...) is followed by one, 0 = off (the default)
      function amt_domain_spec_bdy_update(handle) bind(C, name="amt_domain_spec_bdy_update") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int) :: rc
      end function
      function amt_domain_set_spec_bdy(handle, on) bind(C, name="amt_domain_set_spec_bdy") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: on
         integer(c_int) :: rc
      end function
      function amt_domain_spec_bdy(handle) bind(C, name="amt_domain_spec_bdy") result(on)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int) :: on
      end function
      function amt_ensemble_spec_bdy_update(handle) bind(C, name="amt_ensemble_spec_bdy_update") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int) :: rc
      end function
      function amt_ensemble_set_spec_bdy(handle, on) bind(C, name="amt_ensemble_set_spec_bdy") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: on
         integer(c_int) :: rc
      end function
      function amt_ensemble_spec_bdy(handle) bind(C, name="amt_ensemble_spec_bdy") result(on)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int) :: on
      end function
      ! (13) ensemble mean, sample variance and envelope over the members of a member-stacked field.  Pointer level: a and the
      ! four outputs are DEVICE pointers; an output of ONE member's extents each, c_null_ptr = not wanted (at least one is);
      ! asynchronous on hip_stream
      function amt_moments_device_f32(hip_stream, a, rank, members, ims, ime, jms, jme, kms, kme,                       &
                                      i0, i1, k0, k1, j0, j1, mean, var, lo, hi) bind(C, name="amt_moments_device_f32") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: hip_stream, a
         integer(c_int), value :: rank, members, ims, ime, jms, jme, kms, kme, i0, i1, k0, k1, j0, j1
         type(c_ptr), value :: mean, var, lo, hi
         integer(c_int) :: rc
      end function
      function amt_moments_device_f64(hip_stream, a, rank, members, ims, ime, jms, jme, kms, kme,                       &
                                      i0, i1, k0, k1, j0, j1, mean, var, lo, hi) bind(C, name="amt_moments_device_f64") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: hip_stream, a
         integer(c_int), value :: rank, members, ims, ime, jms, jme, kms, kme, i0, i1, k0, k1, j0, j1
         type(c_ptr), value :: mean, var, lo, hi
         integer(c_int) :: rc
      end function
      ! handle level: region = AMT_REGION_WINDOW or AMT_REGION_MEMORY; asynchronous on the ensemble's stream (amt_ensemble_sync
      ! waits for it); the outputs are device arrays of one member's extents, e.g. amt_domain_field_ptr of a same-shaped domain
      function amt_ensemble_moments(handle, field, region, mean, var, lo, hi) bind(C, name="amt_ensemble_moments") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: field, region
         type(c_ptr), value :: mean, var, lo, hi
         integer(c_int) :: rc
      end function
      ! (14) the acoustic loop's flux averages ru_m, rv_m, ww_m (WRF's sumflux): sub-step `iteration` of n_small_steps adds u, v,
      ! ww into the accumulators, the last one turns the sums into the averages.  Pointer level (members = 1 for a single
      ! patch): every array is a DEVICE pointer; asynchronous on hip_stream
      function amt_sumflux_device_f32(hip_stream, members, ru_m, rv_m, ww_m, u, v, ww, u_1, v_1, ww_1,                      &
                                      muu, muv, msfuy, msfvx_inv, iteration, n_small_steps,                              &
                                      ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,                            &
                                      its, ite, jts, jte, kts, kte) bind(C, name="amt_sumflux_device_f32") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: hip_stream
         integer(c_int), value :: members
         type(c_ptr), value :: ru_m, rv_m, ww_m, u, v, ww, u_1, v_1, ww_1, muu, muv, msfuy, msfvx_inv   ! device pointers
         integer(c_int), value :: iteration, n_small_steps
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      function amt_sumflux_device_f64(hip_stream, members, ru_m, rv_m, ww_m, u, v, ww, u_1, v_1, ww_1,                      &
                                      muu, muv, msfuy, msfvx_inv, iteration, n_small_steps,                              &
                                      ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,                            &
                                      its, ite, jts, jte, kts, kte) bind(C, name="amt_sumflux_device_f64") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: hip_stream
         integer(c_int), value :: members
         type(c_ptr), value :: ru_m, rv_m, ww_m, u, v, ww, u_1, v_1, ww_1, muu, muv, msfuy, msfvx_inv   ! device pointers
         integer(c_int), value :: iteration, n_small_steps
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      ! set: n_small_steps = 0 off (the default); >= 1 with three c_null_ptr: the library allocates the accumulators, with
      ! three device pointers: the caller's.  Every sweep of the handle's stepping (amt_domain_step, amt_slab_step,
      ! amt_grid_step, amt_*_step_end ...) is then followed by one accumulation; the iteration counter runs 1..n and wraps
      function amt_domain_set_sumflux(handle, n_small_steps, ru_m, rv_m, ww_m) bind(C, name="amt_domain_set_sumflux") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: n_small_steps
         type(c_ptr), value :: ru_m, rv_m, ww_m
         integer(c_int) :: rc
      end function
      function amt_domain_sumflux_accumulate(handle) bind(C, name="amt_domain_sumflux_accumulate") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int) :: rc
      end function
      function amt_domain_sumflux_state(handle, n, next_iteration) bind(C, name="amt_domain_sumflux_state") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), intent(out) :: n, next_iteration
         integer(c_int) :: rc
      end function
      function amt_domain_sumflux_ptr(handle, which) bind(C, name="amt_domain_sumflux_ptr") result(ptr)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: which                                              ! 0 ru_m, 1 rv_m, 2 ww_m
         type(c_ptr) :: ptr
      end function
      function amt_ensemble_set_sumflux(handle, n_small_steps, ru_m, rv_m, ww_m) bind(C, name="amt_ensemble_set_sumflux") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: n_small_steps
         type(c_ptr), value :: ru_m, rv_m, ww_m
         integer(c_int) :: rc
      end function
      function amt_ensemble_sumflux_accumulate(handle) bind(C, name="amt_ensemble_sumflux_accumulate") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int) :: rc
      end function
      function amt_ensemble_sumflux_state(handle, n, next_iteration) bind(C, name="amt_ensemble_sumflux_state") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), intent(out) :: n, next_iteration
         integer(c_int) :: rc
      end function
      function amt_ensemble_sumflux_ptr(handle, which) bind(C, name="amt_ensemble_sumflux_ptr") result(ptr)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: which
         type(c_ptr) :: ptr
      end function
      ! (15) the bracket of a Runge-Kutta stage: small_step_prep in front of a stage's acoustic loop, small_step_finish behind it.
      ! Pointer level (members = 1 for a single patch): every array is a DEVICE pointer; asynchronous on hip_stream.  t_old,
      ! mu_old, mu_save, mub and h_diabatic are not AMT_F_* fields; mudf may be c_null_ptr at rk_step > 1
      function amt_stage_prep_device_f32(hip_stream, members, t, t_1, t_old, ww, ww_1, mu, mu_old, mu_save, muts, mudf,     &
                                         mut, mub, rk_step, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,       &
                                         its, ite, jts, jte, kts, kte) bind(C, name="amt_stage_prep_device_f32") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: hip_stream
         integer(c_int), value :: members
         type(c_ptr), value :: t, t_1, t_old, ww, ww_1, mu, mu_old, mu_save, muts, mudf, mut, mub        ! device pointers
         integer(c_int), value :: rk_step
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      function amt_stage_prep_device_f64(hip_stream, members, t, t_1, t_old, ww, ww_1, mu, mu_old, mu_save, muts, mudf,     &
                                         mut, mub, rk_step, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,       &
                                         its, ite, jts, jte, kts, kte) bind(C, name="amt_stage_prep_device_f64") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: hip_stream
         integer(c_int), value :: members
         type(c_ptr), value :: t, t_1, t_old, ww, ww_1, mu, mu_old, mu_save, muts, mudf, mut, mub        ! device pointers
         integer(c_int), value :: rk_step
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      function amt_stage_finish_device_f32(hip_stream, members, t, t_1, ww, ww_1, mu, mu_save, muts, mut, dts,             &
                                           n_small_steps, h_diabatic, ids, ide, jds, jde, kde, ims, ime, jms, jme,       &
                                           kms, kme, its, ite, jts, jte, kts, kte)                                       &
                                           bind(C, name="amt_stage_finish_device_f32") result(rc)
         import :: c_ptr, c_int, c_float
         type(c_ptr), value :: hip_stream
         integer(c_int), value :: members
         type(c_ptr), value :: t, t_1, ww, ww_1, mu, mu_save, muts, mut                                  ! device pointers
         real(c_float), value :: dts
         integer(c_int), value :: n_small_steps
         type(c_ptr), value :: h_diabatic                                                                ! device pointer or c_null_ptr
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      function amt_stage_finish_device_f64(hip_stream, members, t, t_1, ww, ww_1, mu, mu_save, muts, mut, dts,             &
                                           n_small_steps, h_diabatic, ids, ide, jds, jde, kde, ims, ime, jms, jme,       &
                                           kms, kme, its, ite, jts, jte, kts, kte)                                       &
                                           bind(C, name="amt_stage_finish_device_f64") result(rc)
         import :: c_ptr, c_int, c_double
         type(c_ptr), value :: hip_stream
         integer(c_int), value :: members
         type(c_ptr), value :: t, t_1, ww, ww_1, mu, mu_save, muts, mut                                  ! device pointers
         real(c_double), value :: dts
         integer(c_int), value :: n_small_steps
         type(c_ptr), value :: h_diabatic                                                                ! device pointer or c_null_ptr
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      ! set: on = 0 off (the default); on = 1 with four c_null_ptr: the library allocates t_old, mu_old, mu_save, mub (the host
      ! fills mub through amt_domain_stage_ptr), with four device pointers: the caller's.  prep and finish are then issued on the
      ! handle around the stage's sweeps (amt_domain_step, amt_slab_step, amt_grid_step ...); finish uses the handle's dts
      function amt_domain_set_stage(handle, on, t_old, mu_old, mu_save, mub) bind(C, name="amt_domain_set_stage") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: on
         type(c_ptr), value :: t_old, mu_old, mu_save, mub
         integer(c_int) :: rc
      end function
      function amt_domain_stage_ptr(handle, which) bind(C, name="amt_domain_stage_ptr") result(ptr)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: which                                              ! 0 t_old, 1 mu_old, 2 mu_save, 3 mub
         type(c_ptr) :: ptr
      end function
      function amt_domain_stage_prep(handle, rk_step) bind(C, name="amt_domain_stage_prep") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: rk_step
         integer(c_int) :: rc
      end function
      function amt_domain_stage_finish(handle, n_small_steps, h_diabatic) bind(C, name="amt_domain_stage_finish") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: n_small_steps
         type(c_ptr), value :: h_diabatic                                            ! device pointer or c_null_ptr
         integer(c_int) :: rc
      end function
      function amt_ensemble_set_stage(handle, on, t_old, mu_old, mu_save, mub) bind(C, name="amt_ensemble_set_stage") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: on
         type(c_ptr), value :: t_old, mu_old, mu_save, mub
         integer(c_int) :: rc
      end function
      function amt_ensemble_stage_ptr(handle, which) bind(C, name="amt_ensemble_stage_ptr") result(ptr)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: which                                              ! 0 t_old, 1 mu_old, 2 mu_save, 3 mub
         type(c_ptr) :: ptr
      end function
      function amt_ensemble_stage_prep(handle, rk_step) bind(C, name="amt_ensemble_stage_prep") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: rk_step
         integer(c_int) :: rc
      end function
      function amt_ensemble_stage_finish(handle, n_small_steps, h_diabatic) bind(C, name="amt_ensemble_stage_finish") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: n_small_steps
         type(c_ptr), value :: h_diabatic                                            ! device pointer or c_null_ptr
         integer(c_int) :: rc
      end function
      ! (16) the pressure diagnosis that closes an acoustic sub-step: calc_p_rho.  Pointer level (members = 1 for a single
      ! patch): every array is a DEVICE pointer; asynchronous on hip_stream.  mode 1 non-hydrostatic (ph is read), 2 hydrostatic
      ! (ph is integrated up the column); step 0 behind small_step_prep, step /= 0 behind a sub-step (p is damped against pm1)
      function amt_p_rho_device_f32(hip_stream, members, mode, step, al, p, ph, pm1, alt, c2a, t, t_old, mu, muts, rdnw,  &
                                    znu, dnw, t0, smdiv, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,           &
                                    its, ite, jts, jte, kts, kte) bind(C, name="amt_p_rho_device_f32") result(rc)
         import :: c_ptr, c_int, c_float
         type(c_ptr), value :: hip_stream
         integer(c_int), value :: members, mode, step
         type(c_ptr), value :: al, p, ph, pm1, alt, c2a, t, t_old, mu, muts, rdnw, znu, dnw               ! device pointers
         real(c_float), value :: t0, smdiv
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      function amt_p_rho_device_f64(hip_stream, members, mode, step, al, p, ph, pm1, alt, c2a, t, t_old, mu, muts, rdnw,  &
                                    znu, dnw, t0, smdiv, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,           &
                                    its, ite, jts, jte, kts, kte) bind(C, name="amt_p_rho_device_f64") result(rc)
         import :: c_ptr, c_int, c_double
         type(c_ptr), value :: hip_stream
         integer(c_int), value :: members, mode, step
         type(c_ptr), value :: al, p, ph, pm1, alt, c2a, t, t_old, mu, muts, rdnw, znu, dnw               ! device pointers
         real(c_double), value :: t0, smdiv
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      ! (17) the momentum update that opens an acoustic sub-step: advance_uv.  Pointer level (members = 1 for a single patch):
      ! every array is a DEVICE pointer; asynchronous on hip_stream.  u and v are advanced in place; the mass cells at i_start-1
      ! and j_start-1 are the caller's to fill; non_hydrostatic /= 0 adds the vertical pressure term (kde >= 4)
      function amt_advance_uv_device_f32(hip_stream, members, non_hydrostatic, u, v, ru_tend, rv_tend, p, pb, ph, php, alt, al,   &
                                         mu, muu, muv, mudf, cqu, cqv, msfux, msfuy, msfvx, msfvx_inv, msfvy, fnm, fnp, rdnw, &
                                         rdx, rdy, dts, cf1, cf2, cf3, emdiv, periodic_x, specified, nested,                 &
                                         ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,                              &
                                         its, ite, jts, jte, kts, kte) bind(C, name="amt_advance_uv_device_f32") result(rc)
         import :: c_ptr, c_int, c_float
         type(c_ptr), value :: hip_stream
         integer(c_int), value :: members, non_hydrostatic
         type(c_ptr), value :: u, v, ru_tend, rv_tend, p, pb, ph, php, alt, al, mu, muu, muv, mudf, cqu, cqv   ! device pointers
         type(c_ptr), value :: msfux, msfuy, msfvx, msfvx_inv, msfvy, fnm, fnp, rdnw                           ! device pointers
         real(c_float), value :: rdx, rdy, dts, cf1, cf2, cf3, emdiv
         integer(c_int), value :: periodic_x, specified, nested
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      function amt_advance_uv_device_f64(hip_stream, members, non_hydrostatic, u, v, ru_tend, rv_tend, p, pb, ph, php, alt, al,   &
                                         mu, muu, muv, mudf, cqu, cqv, msfux, msfuy, msfvx, msfvx_inv, msfvy, fnm, fnp, rdnw, &
                                         rdx, rdy, dts, cf1, cf2, cf3, emdiv, periodic_x, specified, nested,                 &
                                         ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,                              &
                                         its, ite, jts, jte, kts, kte) bind(C, name="amt_advance_uv_device_f64") result(rc)
         import :: c_ptr, c_int, c_double
         type(c_ptr), value :: hip_stream
         integer(c_int), value :: members, non_hydrostatic
         type(c_ptr), value :: u, v, ru_tend, rv_tend, p, pb, ph, php, alt, al, mu, muu, muv, mudf, cqu, cqv   ! device pointers
         type(c_ptr), value :: msfux, msfuy, msfvx, msfvx_inv, msfvy, fnm, fnp, rdnw                           ! device pointers
         real(c_double), value :: rdx, rdy, dts, cf1, cf2, cf3, emdiv
         integer(c_int), value :: periodic_x, specified, nested
         integer(c_int), value :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme
         integer(c_int), value :: its, ite, jts, jte, kts, kte
         integer(c_int) :: rc
      end function
      ! (17) on a handle: on = 0 off (the default); on /= 0 with nine c_null_ptr: the library allocates ru_tend, rv_tend, pb, php,
      ! cqu, cqv, msfux, msfvx, msfvy (filled through amt_domain_uv_ptr), with nine device pointers: the caller's.  It needs
      ! amt_domain_set_p_rho.  per_sweep /= 0: one update precedes every sweep of amt_domain_step; amt_domain_uv runs one now
      function amt_domain_set_uv(handle, on, per_sweep, emdiv, cf1, cf2, cf3, ru_tend, rv_tend, pb, php, cqu, cqv, msfux, msfvx,    &
                                 msfvy) bind(C, name="amt_domain_set_uv") result(rc)
         import :: c_ptr, c_int, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: on, per_sweep
         real(c_double), value :: emdiv, cf1, cf2, cf3
         type(c_ptr), value :: ru_tend, rv_tend, pb, php, cqu, cqv, msfux, msfvx, msfvy      ! device pointers, all or none
         integer(c_int) :: rc
      end function
      function amt_domain_uv_ptr(handle, which) bind(C, name="amt_domain_uv_ptr") result(ptr)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: which
         type(c_ptr) :: ptr
      end function
      function amt_domain_uv(handle) bind(C, name="amt_domain_uv") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int) :: rc
      end function
      function amt_ensemble_set_uv(handle, on, per_sweep, emdiv, cf1, cf2, cf3, ru_tend, rv_tend, pb, php, cqu, cqv, msfux, msfvx,    &
                                 msfvy) bind(C, name="amt_ensemble_set_uv") result(rc)
         import :: c_ptr, c_int, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: on, per_sweep
         real(c_double), value :: emdiv, cf1, cf2, cf3
         type(c_ptr), value :: ru_tend, rv_tend, pb, php, cqu, cqv, msfux, msfvx, msfvy      ! device pointers, all or none
         integer(c_int) :: rc
      end function
      function amt_ensemble_uv_ptr(handle, which) bind(C, name="amt_ensemble_uv_ptr") result(ptr)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: which
         type(c_ptr) :: ptr
      end function
      function amt_ensemble_uv(handle) bind(C, name="amt_ensemble_uv") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int) :: rc
      end function
      ! set: mode = 0 off (the default); mode = 1 or 2 with eight c_null_ptr: the library allocates al, p, ph, pm1, alt, c2a, znu,
      ! dnw (the host fills alt, c2a, ph, znu, dnw through amt_domain_p_rho_ptr), with eight device pointers: the caller's.  It
      ! needs amt_domain_set_stage.  per_sweep /= 0: one diagnosis follows every sweep of amt_domain_step, amt_slab_step,
      ! amt_grid_step ...; amt_domain_p_rho runs one now (step = 0 behind amt_domain_stage_prep)
      function amt_domain_set_p_rho(handle, mode, per_sweep, t0, smdiv, al, p, ph, pm1, alt, c2a, znu, dnw)                   &
                                    bind(C, name="amt_domain_set_p_rho") result(rc)
         import :: c_ptr, c_int, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: mode, per_sweep
         real(c_double), value :: t0, smdiv
         type(c_ptr), value :: al, p, ph, pm1, alt, c2a, znu, dnw
         integer(c_int) :: rc
      end function
      function amt_domain_p_rho_ptr(handle, which) bind(C, name="amt_domain_p_rho_ptr") result(ptr)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: which                         ! 0 al, 1 p, 2 ph, 3 pm1, 4 alt, 5 c2a, 6 znu, 7 dnw
         type(c_ptr) :: ptr
      end function
      function amt_domain_p_rho(handle, step) bind(C, name="amt_domain_p_rho") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: step
         integer(c_int) :: rc
      end function
      function amt_ensemble_set_p_rho(handle, mode, per_sweep, t0, smdiv, al, p, ph, pm1, alt, c2a, znu, dnw)                   &
                                    bind(C, name="amt_ensemble_set_p_rho") result(rc)
         import :: c_ptr, c_int, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: mode, per_sweep
         real(c_double), value :: t0, smdiv
         type(c_ptr), value :: al, p, ph, pm1, alt, c2a, znu, dnw
         integer(c_int) :: rc
      end function
      function amt_ensemble_p_rho_ptr(handle, which) bind(C, name="amt_ensemble_p_rho_ptr") result(ptr)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: which                         ! 0 al, 1 p, 2 ph, 3 pm1, 4 alt, 5 c2a, 6 znu, 7 dnw
         type(c_ptr) :: ptr
      end function
      function amt_ensemble_p_rho(handle, step) bind(C, name="amt_ensemble_p_rho") result(rc)
         import :: c_ptr, c_int
         type(c_ptr), value :: handle
         integer(c_int), value :: step
         integer(c_int) :: rc
      end function
   end interface

   ! enum amt_field (include/amt_synth.h): the Fortran argument order
   integer(c_int), parameter :: AMT_F_WW = 0, AMT_F_WW_1 = 1, AMT_F_U = 2, AMT_F_U_1 = 3, AMT_F_V = 4,      &
      AMT_F_V_1 = 5, AMT_F_MU = 6, AMT_F_MUT = 7, AMT_F_MUAVE = 8, AMT_F_MUTS = 9, AMT_F_MUU = 10,          &
      AMT_F_MUV = 11, AMT_F_MUDF = 12, AMT_F_T = 13, AMT_F_T_1 = 14, AMT_F_T_AVE = 15, AMT_F_FT = 16,       &
      AMT_F_MU_TEND = 17, AMT_F_DNW = 18, AMT_F_FNM = 19, AMT_F_FNP = 20, AMT_F_RDNW = 21,                  &
      AMT_F_MSFUY = 22, AMT_F_MSFVX_INV = 23, AMT_F_MSFTX = 24, AMT_F_MSFTY = 25
   ! AMT_EXCHANGED_FIELDS: u, u_1, v, v_1, t_1, muu, muv, msfuy, msfvx_inv -- what crosses a patch boundary
   integer(c_int64_t), parameter :: AMT_EXCHANGED_FIELDS = ior(ior(ior(ishft(1_c_int64_t, 2), ishft(1_c_int64_t, 3)),       &
      ior(ishft(1_c_int64_t, 4), ishft(1_c_int64_t, 5))), ior(ior(ishft(1_c_int64_t, 14), ishft(1_c_int64_t, 10)),          &
      ior(ishft(1_c_int64_t, 11), ior(ishft(1_c_int64_t, 22), ishft(1_c_int64_t, 23)))))
   ! enum amt_sides (amt_domain_poison_halos)
   integer(c_int), parameter :: AMT_SIDE_BELOW = 1, AMT_SIDE_ABOVE = 2, AMT_SIDE_LEFT = 4, AMT_SIDE_RIGHT = 8
   ! enum amt_cyclic_axes (amt_cyclic_fill_device_*, amt_domain_set_cyclic, amt_ensemble_set_cyclic)
   integer(c_int), parameter :: AMT_CYCLIC_X = 1, AMT_CYCLIC_Y = 2

CONTAINS

   subroutine amt_check(rc, what)
      integer(c_int), intent(in) :: rc
      character(len=*), intent(in) :: what
      character(kind=c_char), pointer :: cmsg(:)
      character(len=512) :: msg
      integer :: n
      if (rc == AMT_OK) return
      call c_f_pointer(amt_last_error(), cmsg, [512])
      msg = ' '
      do n = 1, 512
         if (cmsg(n) == c_null_char) exit
         msg(n:n) = cmsg(n)
      end do
      write (*, '(a,a,a,i0,a,a)') 'amt: ', what, ' failed with status ', rc, ': ', trim(msg)
      error stop 1
   end subroutine amt_check

END MODULE amt_c_binding
