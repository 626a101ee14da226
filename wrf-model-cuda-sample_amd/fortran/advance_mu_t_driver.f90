! advance_mu_t_driver.f90 -- Fortran-90 host driver of the MI355X advance_mu_t path.
!
! Mirrors the flow of the reference driver (advance_mu_t_driver.f90: read the
! dimensions and the 26 arrays, time one CALL advance_mu_t, compare the 8
! outputs), with two differences: the inputs are the seeded synthetic fields of
! include/amt_synth.h (the reference's /data2/... dump is not shipped), and the
! CALL goes to the drop-in module_small_step_em of this directory, i.e. through
! ISO_C_BINDING into the HIP library.  It then repeats the sweep on the resident
! domain handle (device arrays kept across calls -- the kernel-only time the
! reference reports) and checks that both paths agree bit for bit.
!
!   advance_mu_t_driver [NI NK NJ [nsweeps [outdir [flags [placements [members [nsmall [bracket [pressure [momentum]]]]]]]]]]
!     flags: 0 none, 1 specified, 2 nested, 3 specified+periodic_x
!     placements: > 1 samples that many allocations of the resident state and keeps the fastest (amt_domain_tune_placement)
!     members: > 0 adds an ensemble of that many members of the same shape (amt_ensemble_fill_synthetic, seeds seed + m),
!              stepped nsweeps times, and its mean / variance / envelope over the members (header section 13)
!     nsmall: > 0 adds an acoustic loop of that many sub-steps on a resident handle with the flux averages ru_m, rv_m, ww_m
!             accumulated on the device behind every sweep (header section 14), on a single patch and on an ensemble
!     bracket: 1 with nsmall > 0 adds two Runge-Kutta stages on a resident handle whose acoustic loops of nsmall sub-steps run
!              between small_step_prep and small_step_finish on the device (header section 15); 0 (the default): nothing more
!     pressure: 1 with nsmall > 0 adds a Runge-Kutta stage whose sub-steps are each closed by calc_p_rho on the device (header
!              section 16): hydrostatic on a domain handle, non-hydrostatic on an ensemble; 0 (the default): nothing more
!     momentum: 1 adds advance_uv on the device (header section 17): through the pointer-level call, hydrostatic and, with at
!              least three levels, non-hydrostatic, on the arrays of two resident handles, then as a handle setting on a domain
!              (in front of a sweep) and on an ensemble; 0 (the default): nothing more
!   With outdir the 7 updated arrays are written there as raw native-endian
!   streams <name>.bin for an external checker; with members the moments as ens_<field>_<mean|var|lo|hi>.bin:
!   ww over the whole memory, mu over the compute window, t over the memory less one cell on every side (zero outside).
program advance_mu_t_driver
  use iso_c_binding
  use amt_c_binding
  use module_configure, only : grid_config_rec_type
  use module_small_step_em, only : advance_mu_t
  implicit none

  integer, parameter :: wp = kind(1.0)          ! default REAL: fp32, or fp64 with -fdefault-real-8
  integer :: ni, nk, nj, nsweeps, iflag
  integer :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte
  character(len=256) :: arg, outdir
  type(grid_config_rec_type) :: config_flags
  real(wp), allocatable, target, dimension(:,:,:) :: ww, ww_1, u, u_1, v, v_1, t, t_1, t_ave, ft
  real(wp), allocatable, target, dimension(:,:,:) :: ww_r, t_r, t_ave_r
  real(wp), allocatable, target, dimension(:,:)   :: mu, mut, muave, muts, muu, muv, mudf, mu_tend
  real(wp), allocatable, target, dimension(:,:)   :: msfuy, msfvx_inv, msftx, msfty
  real(wp), allocatable, target, dimension(:,:)   :: mu_r, muave_r, muts_r, mudf_r
  real(wp), allocatable, target, dimension(:)     :: dnw, fnm, fnp, rdnw
  real(wp) :: rdx, rdy, dts, epssm
  integer(c_int64_t), parameter :: seed = 12345_c_int64_t
  integer(c_int) :: rc
  type(c_ptr) :: dom
  real(c_float) :: ms
  integer(kind=8) :: c0, c1, cmid, hz
  real(kind=8) :: cells, secs
  integer :: nbad, ndef, ntune, members, nsmall, bracket, pressure, momentum
  integer(c_int) :: nslots, slot_ids(16)
  real(c_float) :: tune_ms(8)

  ni = 64; nk = 40; nj = 64; nsweeps = 5; outdir = ' '; iflag = 0      ! BASELINE.json configs[0]
  if (command_argument_count() >= 3) then
     call get_command_argument(1, arg); read (arg, *) ni
     call get_command_argument(2, arg); read (arg, *) nk
     call get_command_argument(3, arg); read (arg, *) nj
  end if
  if (command_argument_count() >= 4) then
     call get_command_argument(4, arg); read (arg, *) nsweeps
  end if
  if (command_argument_count() >= 5) call get_command_argument(5, outdir)
  if (command_argument_count() >= 6) then
     call get_command_argument(6, arg); read (arg, *) iflag
  end if
  ntune = 0
  if (command_argument_count() >= 7) then
     call get_command_argument(7, arg); read (arg, *) ntune
     ntune = min(ntune, 8)
  end if
  members = 0
  if (command_argument_count() >= 8) then
     call get_command_argument(8, arg); read (arg, *) members
  end if
  nsmall = 0
  if (command_argument_count() >= 9) then
     call get_command_argument(9, arg); read (arg, *) nsmall
  end if
  bracket = 0
  if (command_argument_count() >= 10) then
     call get_command_argument(10, arg); read (arg, *) bracket
  end if
  pressure = 0
  if (command_argument_count() >= 11) then
     call get_command_argument(11, arg); read (arg, *) pressure
  end if
  momentum = 0
  if (command_argument_count() >= 12) then
     call get_command_argument(12, arg); read (arg, *) momentum
  end if
  config_flags%specified  = (iflag == 1 .or. iflag == 3)
  config_flags%nested     = (iflag == 2)
  config_flags%periodic_x = (iflag == 3)

  ! single-patch domain, SURVEY.md section 8 convention
  ids = 1; ide = ni + 1; jds = 1; jde = nj + 1; kde = nk + 1
  ims = 0; ime = ni + 1; jms = 0; jme = nj + 1; kms = 1; kme = nk + 1
  its = 1; ite = ide;    jts = 1; jte = jde;    kts = 1; kte = kde
  rdx = 1.0e-3_wp; rdy = 1.25e-3_wp; dts = 2.0_wp; epssm = 0.1_wp      ! AMT_SYNTH_* of amt_synth.h

  allocate (ww(ims:ime,kms:kme,jms:jme), ww_1(ims:ime,kms:kme,jms:jme), u(ims:ime,kms:kme,jms:jme))
  allocate (u_1(ims:ime,kms:kme,jms:jme), v(ims:ime,kms:kme,jms:jme), v_1(ims:ime,kms:kme,jms:jme))
  allocate (t(ims:ime,kms:kme,jms:jme), t_1(ims:ime,kms:kme,jms:jme), t_ave(ims:ime,kms:kme,jms:jme))
  allocate (ft(ims:ime,kms:kme,jms:jme))
  allocate (ww_r(ims:ime,kms:kme,jms:jme), t_r(ims:ime,kms:kme,jms:jme), t_ave_r(ims:ime,kms:kme,jms:jme))
  allocate (mu(ims:ime,jms:jme), mut(ims:ime,jms:jme), muave(ims:ime,jms:jme), muts(ims:ime,jms:jme))
  allocate (muu(ims:ime,jms:jme), muv(ims:ime,jms:jme), mudf(ims:ime,jms:jme), mu_tend(ims:ime,jms:jme))
  allocate (msfuy(ims:ime,jms:jme), msfvx_inv(ims:ime,jms:jme), msftx(ims:ime,jms:jme), msfty(ims:ime,jms:jme))
  allocate (mu_r(ims:ime,jms:jme), muave_r(ims:ime,jms:jme), muts_r(ims:ime,jms:jme), mudf_r(ims:ime,jms:jme))
  allocate (dnw(kms:kme), fnm(kms:kme), fnp(kms:kme), rdnw(kms:kme))

  call fill3(AMT_F_WW, ww);   call fill3(AMT_F_WW_1, ww_1); call fill3(AMT_F_U, u);   call fill3(AMT_F_U_1, u_1)
  call fill3(AMT_F_V, v);     call fill3(AMT_F_V_1, v_1);   call fill3(AMT_F_T, t);   call fill3(AMT_F_T_1, t_1)
  call fill3(AMT_F_T_AVE, t_ave); call fill3(AMT_F_FT, ft)
  call fill2(AMT_F_MU, mu);   call fill2(AMT_F_MUT, mut);   call fill2(AMT_F_MUAVE, muave); call fill2(AMT_F_MUTS, muts)
  call fill2(AMT_F_MUU, muu); call fill2(AMT_F_MUV, muv);   call fill2(AMT_F_MUDF, mudf);   call fill2(AMT_F_MU_TEND, mu_tend)
  call fill2(AMT_F_MSFUY, msfuy); call fill2(AMT_F_MSFVX_INV, msfvx_inv)
  call fill2(AMT_F_MSFTX, msftx); call fill2(AMT_F_MSFTY, msfty)
  call fill1(AMT_F_DNW, dnw); call fill1(AMT_F_FNM, fnm);   call fill1(AMT_F_FNP, fnp);     call fill1(AMT_F_RDNW, rdnw)

  print '(a,i0,a,i0,a,i0,a,i0,a,i0)', 'advance_mu_t ', ni, 'x', nk, 'x', nj, ' real*', storage_size(rdx)/8, &
        '  HIP devices: ', amt_device_count()

  ! ---- resident path first (it needs the un-updated inputs) ----
  rc = amt_domain_create(dom, int(storage_size(rdx)/8, c_int),                                 &
                         merge(1_c_int, 0_c_int, config_flags%periodic_x),                      &
                         merge(1_c_int, 0_c_int, config_flags%specified),                       &
                         merge(1_c_int, 0_c_int, config_flags%nested),                          &
                         ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)
  call amt_check(rc, 'amt_domain_create')
  call amt_check(amt_domain_set_scalars(dom, real(rdx, c_double), real(rdy, c_double), real(dts, c_double), &
                                        real(epssm, c_double)), 'amt_domain_set_scalars')
  ! one untimed sweep on whatever the fresh buffers hold: loads the kernel's code object, so that the
  ! timed sweeps below are kernel time only; every array is uploaded after it
  call amt_check(amt_domain_step(dom, 1_c_int), 'amt_domain_step (warm-up)')
  call amt_check(amt_domain_sync(dom), 'amt_domain_sync')
  call up(AMT_F_WW, c_loc(ww));     call up(AMT_F_WW_1, c_loc(ww_1)); call up(AMT_F_U, c_loc(u))
  call up(AMT_F_U_1, c_loc(u_1));   call up(AMT_F_V, c_loc(v));       call up(AMT_F_V_1, c_loc(v_1))
  call up(AMT_F_T, c_loc(t));       call up(AMT_F_T_1, c_loc(t_1));   call up(AMT_F_T_AVE, c_loc(t_ave))
  call up(AMT_F_FT, c_loc(ft));     call up(AMT_F_MU, c_loc(mu));     call up(AMT_F_MUT, c_loc(mut))
  call up(AMT_F_MUAVE, c_loc(muave)); call up(AMT_F_MUTS, c_loc(muts)); call up(AMT_F_MUU, c_loc(muu))
  call up(AMT_F_MUV, c_loc(muv));   call up(AMT_F_MUDF, c_loc(mudf)); call up(AMT_F_MU_TEND, c_loc(mu_tend))
  call up(AMT_F_MSFUY, c_loc(msfuy)); call up(AMT_F_MSFVX_INV, c_loc(msfvx_inv))
  call up(AMT_F_MSFTX, c_loc(msftx)); call up(AMT_F_MSFTY, c_loc(msfty))
  call up(AMT_F_DNW, c_loc(dnw));   call up(AMT_F_FNM, c_loc(fnm));   call up(AMT_F_FNP, c_loc(fnp))
  call up(AMT_F_RDNW, c_loc(rdnw))
  ! placement of the arrays' pages (+-3 % of a sweep, DESIGN.md section 4.3): sampled by the library, contents kept
  if (ntune > 1) then
     call amt_check(amt_domain_tune_placement(dom, int(ntune, c_int), tune_ms), 'amt_domain_tune_placement')
     print '(a,i0,a,8f9.4)', 'placement tuning, ', ntune, ' allocations, ms/sweep each: ', tune_ms(1:ntune)
  end if
  call amt_check(amt_domain_step_timed(dom, int(nsweeps, c_int), ms), 'amt_domain_step_timed')
  cells = real(ni, 8) * real(nk, 8) * real(nj, 8)
  print '(a,i0,a,f10.4,a,f12.1,a)', 'resident device path: ', nsweeps, ' sweeps, ', ms / nsweeps, &
        ' ms/sweep (kernel only), ', cells * nsweeps / (ms * 1.0d-3) / 1.0d6, ' Mcells/s'
  call dn(AMT_F_WW, c_loc(ww_r));   call dn(AMT_F_T, c_loc(t_r));     call dn(AMT_F_T_AVE, c_loc(t_ave_r))
  call dn(AMT_F_MU, c_loc(mu_r));   call dn(AMT_F_MUAVE, c_loc(muave_r)); call dn(AMT_F_MUTS, c_loc(muts_r))
  call dn(AMT_F_MUDF, c_loc(mudf_r))
  call amt_check(amt_domain_destroy(dom), 'amt_domain_destroy')

  ! ---- one-shot drop-in: the reference driver's CALL (advance_mu_t_driver.f90:193-205), nsweeps times ----
  call system_clock(count_rate=hz)
  call system_clock(count=c0)
  block
    integer :: s
    do s = 1, nsweeps
      CALL advance_mu_t( ww, ww_1, u, u_1, v, v_1,            &
                         mu, mut, muave, muts, muu, muv,      &
                         mudf, t, t_1,                        &
                         t_ave, ft, mu_tend,                  &
                         rdx, rdy, dts, epssm,                &
                         dnw, fnm, fnp, rdnw,                 &
                         msfuy, msfvx_inv,                    &
                         msftx, msfty,                        &
                         config_flags,                        &
                         ids, ide, jds, jde, kde,             &
                         ims, ime, jms, jme, kms, kme,        &
                         its, ite, jts, jte, kts, kte )
      if (s == 1) call system_clock(count=cmid)
    end do
  end block
  call system_clock(count=c1)
  ! the first call creates this thread's device workspace (streams, events, arena), which later calls reuse
  secs = real(cmid - c0, 8) / real(hz, 8)
  print '(a,f10.4,a)', 'one-shot host path:   first call ', secs * 1.0d3, ' ms (creates the device workspace)'
  nslots = amt_host_devices(slot_ids, 16_c_int)             ! AMT_ONESHOT_DEVICES="0,1,..." | "all": one call, several devices
  if (nslots > 0) print '(a,i0,a,16(1x,i0))', 'one-shot host path:   every call fans its rows over ', nslots, ' device slot(s):', slot_ids(1:nslots)
  if (nsweeps > 1) then
     secs = real(c1 - cmid, 8) / real(hz, 8)
     print '(a,i0,a,f10.4,a,f12.1,a)', 'one-shot host path:   ', nsweeps - 1, ' calls,  ', secs * 1.0d3 / (nsweeps - 1), &
           ' ms/call  (H2D+kernel+D2H), ', cells * (nsweeps - 1) / secs / 1.0d6, ' Mcells/s'
  end if

  ! ---- the same calls with the ten 3-D arrays page-locked once (the reference driver allocates its
  !      host buffers pinned, advance_mu_t_driver.cu:97-167): the library then streams the window in
  !      j chunks (H2D / kernel / D2H overlapped on three streams).  Timing only: the arrays have
  !      already been advanced nsweeps times, these extra sweeps are undone by nothing and the
  !      comparison below is therefore made BEFORE them.
  nbad = 0
  nbad = nbad + count(transfer(ww, 1_1, size(ww) * storage_size(rdx) / 8) /= transfer(ww_r, 1_1, size(ww) * storage_size(rdx) / 8))
  nbad = nbad + count(t /= t_r) + count(t_ave /= t_ave_r) + count(mu /= mu_r)
  nbad = nbad + count(muave /= muave_r) + count(muts /= muts_r) + count(mudf /= mudf_r)
  if (len_trim(outdir) > 0) then
     call dump3('ww', ww); call dump3('t', t); call dump3('t_ave', t_ave)
     call dump2('mu', mu); call dump2('muave', muave); call dump2('muts', muts); call dump2('mudf', mudf)
  end if
  print '(a,4es24.16)', 'checksums ww t mu muave: ', sum(real(ww, 8)), sum(real(t, 8)), sum(real(mu, 8)), sum(real(muave, 8))
  call pin3(ww); call pin3(ww_1); call pin3(u); call pin3(u_1); call pin3(v); call pin3(v_1)
  call pin3(t); call pin3(t_1); call pin3(t_ave); call pin3(ft)
  call system_clock(count=c0)
  block
    integer :: s
    do s = 1, nsweeps
      CALL advance_mu_t( ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv, mudf, t, t_1,        &
                         t_ave, ft, mu_tend, rdx, rdy, dts, epssm, dnw, fnm, fnp, rdnw,                 &
                         msfuy, msfvx_inv, msftx, msfty, config_flags,                                  &
                         ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte )
    end do
  end block
  call system_clock(count=c1)
  secs = real(c1 - c0, 8) / real(hz, 8)
  print '(a,i0,a,f10.4,a,f12.1,a)', 'one-shot, pinned host: ', nsweeps, ' calls, ', secs * 1.0d3 / nsweeps, &
        ' ms/call  (streamed in j chunks),  ', cells * nsweeps / secs / 1.0d6, ' Mcells/s'
  ! ---- the acoustic loop of one Runge-Kutta stage: the linearisation state ww_1, u_1, v_1, t_1 and the tendency
  !      ft do not change between the sub-steps, so with the residency cache on they are uploaded by the first call
  !      only (amt_host_invalidate(c_null_ptr) when the next stage has rewritten them).  Timing only, as above.
  ww_r = ww; t_r = t; mu_r = mu                       ! the state this loop starts from (the deferred loop below repeats it)
  call amt_check(amt_host_cache_enable(1_c_int), 'amt_host_cache_enable')
  CALL advance_mu_t( ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv, mudf, t, t_1,            &
                     t_ave, ft, mu_tend, rdx, rdy, dts, epssm, dnw, fnm, fnp, rdnw,                     &
                     msfuy, msfvx_inv, msftx, msfty, config_flags,                                      &
                     ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte )
  call system_clock(count=c0)
  block
    integer :: s
    do s = 1, nsweeps
      CALL advance_mu_t( ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv, mudf, t, t_1,        &
                         t_ave, ft, mu_tend, rdx, rdy, dts, epssm, dnw, fnm, fnp, rdnw,                 &
                         msfuy, msfvx_inv, msftx, msfty, config_flags,                                  &
                         ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte )
    end do
  end block
  call system_clock(count=c1)
  secs = real(c1 - c0, 8) / real(hz, 8)
  print '(a,i0,a,f10.4,a,f12.1,a)', 'one-shot, pinned, constants resident: ', nsweeps, ' calls, ', secs * 1.0d3 / nsweeps, &
        ' ms/call,  ', cells * nsweeps / secs / 1.0d6, ' Mcells/s'
  ! ---- the same loop with the OUTPUTS deferred as well (amt_host_defer): ww, t, t_ave, mu, muave, muts, mudf stay on the
  !      device from sub-step to sub-step -- in WRF the next routine of the acoustic loop would take them there -- and come
  !      down once, when the loop is over (amt_host_fetch); a sub-step then uploads u, v and the 2-D / 1-D inputs only.
  !      Starts from the state the loop above started from and must end with its bits.
  call swap3(ww, ww_r); call swap3(t, t_r); call swap2(mu, mu_r)
  t_ave_r = t_ave; muave_r = muave; muts_r = muts; mudf_r = mudf
  call amt_check(amt_host_defer(c_null_ptr, 1_c_int), 'amt_host_defer')
  CALL advance_mu_t( ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv, mudf, t, t_1,            &
                     t_ave, ft, mu_tend, rdx, rdy, dts, epssm, dnw, fnm, fnp, rdnw,                     &
                     msfuy, msfvx_inv, msftx, msfty, config_flags,                                      &
                     ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte )
  call system_clock(count=c0)
  block
    integer :: s
    do s = 1, nsweeps
      CALL advance_mu_t( ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu, muv, mudf, t, t_1,        &
                         t_ave, ft, mu_tend, rdx, rdy, dts, epssm, dnw, fnm, fnp, rdnw,                 &
                         msfuy, msfvx_inv, msftx, msfty, config_flags,                                  &
                         ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte )
    end do
  end block
  call system_clock(count=c1)
  secs = real(c1 - c0, 8) / real(hz, 8)
  print '(a,i0,a,f10.4,a,f12.1,a)', 'one-shot, pinned, constants resident, outputs deferred: ', nsweeps, ' calls, ', &
        secs * 1.0d3 / nsweeps, ' ms/call,  ', cells * nsweeps / secs / 1.0d6, ' Mcells/s'
  if (amt_host_stale(c_loc(t)) /= 1) error stop 3
  call system_clock(count=c0)
  call amt_check(amt_host_fetch(c_null_ptr), 'amt_host_fetch')
  call system_clock(count=c1)
  print '(a,f10.4,a)', 'amt_host_fetch of the seven outputs, once per loop: ', real(c1 - c0, 8) / real(hz, 8) * 1.0d3, ' ms'
  if (amt_host_stale(c_null_ptr) /= 0) error stop 4
  call amt_check(amt_host_defer(c_null_ptr, 0_c_int), 'amt_host_defer')
  ndef = 0
  ndef = ndef + count(transfer(ww, 1_1, size(ww) * storage_size(rdx) / 8) /= transfer(ww_r, 1_1, size(ww) * storage_size(rdx) / 8))
  ndef = ndef + count(t /= t_r) + count(t_ave /= t_ave_r) + count(mu /= mu_r)
  ndef = ndef + count(muave /= muave_r) + count(muts /= muts_r) + count(mudf /= mudf_r)
  print '(a,i0)', 'deferred loop vs plain loop: differing elements = ', ndef
  call amt_check(amt_host_cache_enable(0_c_int), 'amt_host_cache_enable')
  call unpin3(ww); call unpin3(ww_1); call unpin3(u); call unpin3(u_1); call unpin3(v); call unpin3(v_1)
  call unpin3(t); call unpin3(t_1); call unpin3(t_ave); call unpin3(ft)

  ! ---- both paths must agree bit for bit (compared above, before the pinned timing run) ----
  print '(a,i0)', 'one-shot vs resident: differing elements = ', nbad
  if (nbad /= 0) error stop 2
  if (ndef /= 0) error stop 5

  if (members > 0) call ensemble_moments()
  if (nsmall > 0) call flux_averages()
  if (nsmall > 0 .and. bracket == 1) call stage_bracket()
  if (nsmall > 0 .and. pressure == 1) call pressure_diagnosis()
  if (momentum == 1) call momentum_update()

contains

  ! One Runge-Kutta stage whose acoustic loop of nsmall sub-steps runs with calc_p_rho on the device: step 0 behind
  ! small_step_prep, then one diagnosis behind every sweep (per_sweep).  The stage bracket's four arrays are fields of a second
  ! handle as in stage_bracket; al, p, ph, pm1, alt, c2a, znu, dnw are fields of a third one (ww, ww_1, u, u_1, v, v_1, fnm, dnw;
  ! filled from the generator, they come down with amt_domain_download).  Hydrostatic (mode 2) on the domain handle, where the
  ! pointer-level call repeats the step-0 diagnosis and must give the same bits; non-hydrostatic (mode 1) on an ensemble.
  subroutine pressure_diagnosis()
    type(c_ptr) :: d, ex, px, own, e, eex, epx
    real(wp), allocatable, target :: a3(:,:,:), b3(:,:,:)
    integer(c_int) :: wb, mm, k
    integer(c_int), parameter :: xf(4) = [AMT_F_T, AMT_F_MU, AMT_F_MUAVE, AMT_F_MUT]      ! of `ex`: t_old, mu_old, mu_save, mub
    ! of `px`: al, p, ph, pm1, alt, c2a, znu, dnw
    integer(c_int), parameter :: pf(8) = [AMT_F_WW, AMT_F_WW_1, AMT_F_U, AMT_F_U_1, AMT_F_V, AMT_F_V_1, AMT_F_FNM, AMT_F_DNW]
    real(c_double), parameter :: t0 = 300.0_c_double, smdiv = 0.1_c_double
    wb = int(storage_size(rdx)/8, c_int)
    mm = int(max(members, 1), c_int)
    allocate (a3(ims:ime,kms:kme,jms:jme), b3(ims:ime,kms:kme,jms:jme))
    call make_domain(d, seed)
    call make_domain(ex, seed + 1_c_int64_t)
    call make_domain(px, seed + 2_c_int64_t)
    call make_domain(own, seed)
    ! off until set; the setting needs the stage bracket; a mix of given and missing arrays is refused
    if (c_associated(amt_domain_p_rho_ptr(d, 0_c_int))) error stop 10
    if (amt_domain_p_rho(d, 0_c_int) /= AMT_ERR_PRECONDITION) error stop 10
    if (amt_domain_set_p_rho(d, 2_c_int, 1_c_int, t0, smdiv, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr,     &
                             c_null_ptr, c_null_ptr, c_null_ptr) /= AMT_ERR_PRECONDITION) error stop 10
    call amt_check(amt_domain_set_stage(d, 1_c_int, amt_domain_field_ptr(ex, xf(1)), amt_domain_field_ptr(ex, xf(2)),       &
                   amt_domain_field_ptr(ex, xf(3)), amt_domain_field_ptr(ex, xf(4))), 'amt_domain_set_stage')
    if (amt_domain_set_p_rho(d, 2_c_int, 1_c_int, t0, smdiv, amt_domain_field_ptr(px, pf(1)), c_null_ptr, c_null_ptr,       &
                             c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr) /= AMT_ERR_INVALID_ARG) error stop 10
    call amt_check(amt_domain_set_p_rho(d, 2_c_int, 1_c_int, t0, smdiv, amt_domain_field_ptr(px, pf(1)),                    &
                   amt_domain_field_ptr(px, pf(2)), amt_domain_field_ptr(px, pf(3)), amt_domain_field_ptr(px, pf(4)),       &
                   amt_domain_field_ptr(px, pf(5)), amt_domain_field_ptr(px, pf(6)), amt_domain_field_ptr(px, pf(7)),       &
                   amt_domain_field_ptr(px, pf(8))), 'amt_domain_set_p_rho')
    if (.not. c_associated(amt_domain_p_rho_ptr(d, 7_c_int), amt_domain_field_ptr(px, pf(8)))) error stop 10
    ! the library's own eight arrays on another handle: allocated, named, freed
    call amt_check(amt_domain_set_stage(own, 1_c_int, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr), 'amt_domain_set_stage')
    call amt_check(amt_domain_set_p_rho(own, 1_c_int, 0_c_int, t0, smdiv, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr,   &
                   c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr), 'amt_domain_set_p_rho')
    do k = 0, 7
       if (.not. c_associated(amt_domain_p_rho_ptr(own, k))) error stop 10
    end do
    call amt_check(amt_domain_set_p_rho(own, 0_c_int, 0_c_int, t0, smdiv, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr,   &
                   c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr), 'amt_domain_set_p_rho')
    if (c_associated(amt_domain_p_rho_ptr(own, 0_c_int))) error stop 10
    call amt_check(amt_domain_destroy(own), 'amt_domain_destroy')
    ! the stage: prep, the step-0 diagnosis -- by the handle, then once more by the pointer-level call: the same bits --, the
    ! sub-steps with one diagnosis behind each, finish
    call amt_check(amt_domain_stage_prep(d, 1_c_int), 'amt_domain_stage_prep')
    call amt_check(amt_domain_p_rho(d, 0_c_int), 'amt_domain_p_rho')
    call amt_check(amt_domain_download(px, pf(2), c_loc(a3)), 'amt_domain_download')
    call p_rho_device(d, ex, px)
    call amt_check(amt_domain_sync(d), 'amt_domain_sync')
    call amt_check(amt_domain_download(px, pf(2), c_loc(b3)), 'amt_domain_download')
    if (any(transfer(a3, 1_c_int8_t, size(a3) * wb) /= transfer(b3, 1_c_int8_t, size(b3) * wb))) error stop 11
    call amt_check(amt_domain_step(d, int(nsmall, c_int)), 'amt_domain_step')
    call amt_check(amt_domain_stage_finish(d, int(nsmall, c_int), c_null_ptr), 'amt_domain_stage_finish')
    call amt_check(amt_domain_sync(d), 'amt_domain_sync')
    call amt_check(amt_domain_download(px, pf(2), c_loc(a3)), 'amt_domain_download')
    if (len_trim(outdir) > 0) call dump3('p_rho_p', a3)
    ! an ensemble, non-hydrostatic: every member's diagnosis in one launch, the arrays member-stacked in two more ensembles
    call make_ensemble(e, mm, seed)
    call make_ensemble(eex, mm, seed + 1_c_int64_t)
    call make_ensemble(epx, mm, seed + 2_c_int64_t)
    call amt_check(amt_ensemble_set_stage(e, 1_c_int, amt_ensemble_field_ptr(eex, xf(1)), amt_ensemble_field_ptr(eex, xf(2)),  &
                   amt_ensemble_field_ptr(eex, xf(3)), amt_ensemble_field_ptr(eex, xf(4))), 'amt_ensemble_set_stage')
    call amt_check(amt_ensemble_set_p_rho(e, 1_c_int, 1_c_int, t0, smdiv, amt_ensemble_field_ptr(epx, pf(1)),               &
                   amt_ensemble_field_ptr(epx, pf(2)), amt_ensemble_field_ptr(epx, pf(3)), amt_ensemble_field_ptr(epx, pf(4)), &
                   amt_ensemble_field_ptr(epx, pf(5)), amt_ensemble_field_ptr(epx, pf(6)), amt_ensemble_field_ptr(epx, pf(7)), &
                   amt_ensemble_field_ptr(epx, pf(8))), 'amt_ensemble_set_p_rho')
    if (.not. c_associated(amt_ensemble_p_rho_ptr(e, 1_c_int), amt_ensemble_field_ptr(epx, pf(2)))) error stop 10
    call amt_check(amt_ensemble_stage_prep(e, 1_c_int), 'amt_ensemble_stage_prep')
    call amt_check(amt_ensemble_p_rho(e, 0_c_int), 'amt_ensemble_p_rho')
    call amt_check(amt_ensemble_step(e, int(nsmall, c_int)), 'amt_ensemble_step')
    call amt_check(amt_ensemble_stage_finish(e, int(nsmall, c_int), c_null_ptr), 'amt_ensemble_stage_finish')
    call amt_check(amt_ensemble_sync(e), 'amt_ensemble_sync')
    print '(a,i0,a,i0,a,es24.16)', 'calc_p_rho behind each of ', nsmall, ' sub-steps on the device, hydrostatic on a domain and '// &
       'non-hydrostatic on an ensemble of ', mm, ' members; checksum of p: ', sum(real(a3(its:ite-1, kts:kte-1, jts:jte-1), 8))
    call amt_check(amt_ensemble_destroy(e), 'amt_ensemble_destroy')
    call amt_check(amt_ensemble_destroy(eex), 'amt_ensemble_destroy')
    call amt_check(amt_ensemble_destroy(epx), 'amt_ensemble_destroy')
    call amt_check(amt_domain_set_p_rho(d, 0_c_int, 0_c_int, t0, smdiv, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr,     &
                   c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr), 'amt_domain_set_p_rho')
    call amt_check(amt_domain_destroy(d), 'amt_domain_destroy')
    call amt_check(amt_domain_destroy(ex), 'amt_domain_destroy')
    call amt_check(amt_domain_destroy(px), 'amt_domain_destroy')
  end subroutine

  ! the step-0 diagnosis of handle h, hydrostatic, with the pointer-level call on h's stream: t_old of `ex`, the eight of `px`
  subroutine p_rho_device(h, ex, px)
    type(c_ptr), intent(in) :: h, ex, px
    type(c_ptr) :: stream
    stream = amt_domain_stream(h)
    if (storage_size(rdx) == 64) then
       rc = amt_p_rho_device_f64(stream, 1_c_int, 2_c_int, 0_c_int, amt_domain_field_ptr(px, AMT_F_WW),                      &
                                 amt_domain_field_ptr(px, AMT_F_WW_1), amt_domain_field_ptr(px, AMT_F_U),                   &
                                 amt_domain_field_ptr(px, AMT_F_U_1), amt_domain_field_ptr(px, AMT_F_V),                    &
                                 amt_domain_field_ptr(px, AMT_F_V_1), amt_domain_field_ptr(h, AMT_F_T),                     &
                                 amt_domain_field_ptr(ex, AMT_F_T), amt_domain_field_ptr(h, AMT_F_MU),                      &
                                 amt_domain_field_ptr(h, AMT_F_MUTS), amt_domain_field_ptr(h, AMT_F_RDNW),                  &
                                 amt_domain_field_ptr(px, AMT_F_FNM), amt_domain_field_ptr(px, AMT_F_DNW),                  &
                                 300.0_c_double, 0.1_c_double,                                                              &
                                 ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)
    else
       rc = amt_p_rho_device_f32(stream, 1_c_int, 2_c_int, 0_c_int, amt_domain_field_ptr(px, AMT_F_WW),                      &
                                 amt_domain_field_ptr(px, AMT_F_WW_1), amt_domain_field_ptr(px, AMT_F_U),                   &
                                 amt_domain_field_ptr(px, AMT_F_U_1), amt_domain_field_ptr(px, AMT_F_V),                    &
                                 amt_domain_field_ptr(px, AMT_F_V_1), amt_domain_field_ptr(h, AMT_F_T),                     &
                                 amt_domain_field_ptr(ex, AMT_F_T), amt_domain_field_ptr(h, AMT_F_MU),                      &
                                 amt_domain_field_ptr(h, AMT_F_MUTS), amt_domain_field_ptr(h, AMT_F_RDNW),                  &
                                 amt_domain_field_ptr(px, AMT_F_FNM), amt_domain_field_ptr(px, AMT_F_DNW),                  &
                                 300.0_c_float, 0.1_c_float,                                                                &
                                 ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)
    end if
    call amt_check(rc, 'amt_p_rho_device')
  end subroutine

  ! One advance_uv through the pointer-level call on the stream of a resident handle `d`, whose u and v it advances: the other
  ! arrays are fields of `d` and of a second handle `px` (p, pb, ph, php, alt, al are its ww, ww_1, u, u_1, v, v_1), filled by the
  ! generator.  Hydrostatic, then non-hydrostatic where the column has three levels of p; u must have moved and stay finite.
  subroutine momentum_update()
    type(c_ptr) :: d, px
    real(wp), allocatable, target :: a3(:,:,:), b3(:,:,:)
    integer(c_int) :: nh
    integer :: moved
    allocate (a3(ims:ime,kms:kme,jms:jme), b3(ims:ime,kms:kme,jms:jme))
    call make_domain(d, seed)
    call make_domain(px, seed + 3_c_int64_t)
    do nh = 0, merge(1, 0, kde >= 4)
       call amt_check(amt_domain_download(d, AMT_F_U, c_loc(a3)), 'amt_domain_download')
       call uv_device(d, px, nh)
       call amt_check(amt_domain_sync(d), 'amt_domain_sync')
       call amt_check(amt_domain_download(d, AMT_F_U, c_loc(b3)), 'amt_domain_download')
       moved = count(a3 /= b3)
       if (moved == 0 .or. any(b3 /= b3)) error stop 11
       print '(a,i0,a,i0,a,es24.16)', 'advance_uv on the device, non_hydrostatic = ', nh, ': ', moved, ' elements of u moved, sum = ', &
             sum(real(b3, kind=8))
    end do
    call amt_check(amt_domain_destroy(d), 'amt_domain_destroy')
    call amt_check(amt_domain_destroy(px), 'amt_domain_destroy')
    call uv_on_handles()
  end subroutine

  ! The same update as a handle setting: hydrostatic on a domain handle, in front of a sweep (per_sweep) and once by the call;
  ! non-hydrostatic (where the column has three levels of p) on an ensemble.  The stage bracket's arrays are fields of `ex`, the
  ! pressure diagnosis's of `px` as in pressure_diagnosis, the update's nine -- ru_tend, rv_tend, pb, php, cqu, cqv, msfux, msfvx,
  ! msfvy -- fields of `qx`.
  subroutine uv_on_handles()
    type(c_ptr) :: d, ex, px, qx, own, e, eex, epx, eqx
    real(wp), allocatable, target :: a3(:,:,:), b3(:,:,:)
    integer(c_int) :: mm, k, mode
    integer(c_int), parameter :: xf(4) = [AMT_F_T, AMT_F_MU, AMT_F_MUAVE, AMT_F_MUT]
    integer(c_int), parameter :: pf(8) = [AMT_F_WW, AMT_F_WW_1, AMT_F_U, AMT_F_U_1, AMT_F_V, AMT_F_V_1, AMT_F_FNM, AMT_F_DNW]
    integer(c_int), parameter :: qf(9) = [AMT_F_FT, AMT_F_T_AVE, AMT_F_WW_1, AMT_F_U_1, AMT_F_T, AMT_F_T_1, AMT_F_MSFTX, AMT_F_MSFTY, &
                                          AMT_F_MSFUY]
    real(c_double), parameter :: t0 = 300.0_c_double, smdiv = 0.1_c_double, emdiv = 0.01_c_double
    real(c_double), parameter :: cf1 = 1.5_c_double, cf2 = -0.75_c_double, cf3 = 0.25_c_double
    mm = int(max(members, 1), c_int)
    allocate (a3(ims:ime,kms:kme,jms:jme), b3(ims:ime,kms:kme,jms:jme))
    call make_domain(d, seed)
    call make_domain(ex, seed + 1_c_int64_t)
    call make_domain(px, seed + 2_c_int64_t)
    call make_domain(qx, seed + 3_c_int64_t)
    call make_domain(own, seed)
    ! off until set; the setting needs the pressure diagnosis; a mix of given and missing arrays is refused
    if (c_associated(amt_domain_uv_ptr(d, 0_c_int))) error stop 12
    if (amt_domain_uv(d) /= AMT_ERR_PRECONDITION) error stop 12
    if (amt_domain_set_uv(d, 1_c_int, 1_c_int, emdiv, cf1, cf2, cf3, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
                          c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr) /= AMT_ERR_PRECONDITION) error stop 12
    call amt_check(amt_domain_set_stage(d, 1_c_int, amt_domain_field_ptr(ex, xf(1)), amt_domain_field_ptr(ex, xf(2)),        &
                   amt_domain_field_ptr(ex, xf(3)), amt_domain_field_ptr(ex, xf(4))), 'amt_domain_set_stage')
    call amt_check(amt_domain_set_p_rho(d, 2_c_int, 0_c_int, t0, smdiv, amt_domain_field_ptr(px, pf(1)),                     &
                   amt_domain_field_ptr(px, pf(2)), amt_domain_field_ptr(px, pf(3)), amt_domain_field_ptr(px, pf(4)),        &
                   amt_domain_field_ptr(px, pf(5)), amt_domain_field_ptr(px, pf(6)), amt_domain_field_ptr(px, pf(7)),        &
                   amt_domain_field_ptr(px, pf(8))), 'amt_domain_set_p_rho')
    if (amt_domain_set_uv(d, 1_c_int, 1_c_int, emdiv, cf1, cf2, cf3, amt_domain_field_ptr(qx, qf(1)), c_null_ptr, c_null_ptr,   &
                          c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr) /= AMT_ERR_INVALID_ARG) error stop 12
    call amt_check(amt_domain_set_uv(d, 1_c_int, 1_c_int, emdiv, cf1, cf2, cf3, amt_domain_field_ptr(qx, qf(1)),              &
                   amt_domain_field_ptr(qx, qf(2)), amt_domain_field_ptr(qx, qf(3)), amt_domain_field_ptr(qx, qf(4)),        &
                   amt_domain_field_ptr(qx, qf(5)), amt_domain_field_ptr(qx, qf(6)), amt_domain_field_ptr(qx, qf(7)),        &
                   amt_domain_field_ptr(qx, qf(8)), amt_domain_field_ptr(qx, qf(9))), 'amt_domain_set_uv')
    if (.not. c_associated(amt_domain_uv_ptr(d, 8_c_int), amt_domain_field_ptr(qx, qf(9)))) error stop 12
    ! the library's own nine arrays on another handle: allocated, named, freed
    call amt_check(amt_domain_set_stage(own, 1_c_int, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr), 'amt_domain_set_stage')
    call amt_check(amt_domain_set_p_rho(own, 2_c_int, 0_c_int, t0, smdiv, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr,   &
                   c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr), 'amt_domain_set_p_rho')
    call amt_check(amt_domain_set_uv(own, 1_c_int, 0_c_int, emdiv, cf1, cf2, cf3, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
                   c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr), 'amt_domain_set_uv')
    do k = 0, 8
       if (.not. c_associated(amt_domain_uv_ptr(own, k))) error stop 12
    end do
    call amt_check(amt_domain_set_uv(own, 0_c_int, 0_c_int, emdiv, cf1, cf2, cf3, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
                   c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr), 'amt_domain_set_uv')
    if (c_associated(amt_domain_uv_ptr(own, 0_c_int))) error stop 12
    call amt_check(amt_domain_destroy(own), 'amt_domain_destroy')
    ! prep, the step-0 diagnosis, one update by the call, then one more in front of the sweep
    call amt_check(amt_domain_stage_prep(d, 1_c_int), 'amt_domain_stage_prep')
    call amt_check(amt_domain_p_rho(d, 0_c_int), 'amt_domain_p_rho')
    call amt_check(amt_domain_download(d, AMT_F_U, c_loc(a3)), 'amt_domain_download')
    call amt_check(amt_domain_uv(d), 'amt_domain_uv')
    call amt_check(amt_domain_download(d, AMT_F_U, c_loc(b3)), 'amt_domain_download')
    if (count(a3 /= b3) == 0) error stop 12
    call amt_check(amt_domain_step(d, 1_c_int), 'amt_domain_step')
    call amt_check(amt_domain_download(d, AMT_F_U, c_loc(a3)), 'amt_domain_download')
    if (count(a3 /= b3) == 0) error stop 12
    ! an ensemble: every member's update in one launch
    mode = merge(1_c_int, 2_c_int, kde >= 4)
    call make_ensemble(e, mm, seed)
    call make_ensemble(eex, mm, seed + 1_c_int64_t)
    call make_ensemble(epx, mm, seed + 2_c_int64_t)
    call make_ensemble(eqx, mm, seed + 3_c_int64_t)
    call amt_check(amt_ensemble_set_stage(e, 1_c_int, amt_ensemble_field_ptr(eex, xf(1)), amt_ensemble_field_ptr(eex, xf(2)),  &
                   amt_ensemble_field_ptr(eex, xf(3)), amt_ensemble_field_ptr(eex, xf(4))), 'amt_ensemble_set_stage')
    call amt_check(amt_ensemble_set_p_rho(e, mode, 0_c_int, t0, smdiv, amt_ensemble_field_ptr(epx, pf(1)),                  &
                   amt_ensemble_field_ptr(epx, pf(2)), amt_ensemble_field_ptr(epx, pf(3)), amt_ensemble_field_ptr(epx, pf(4)), &
                   amt_ensemble_field_ptr(epx, pf(5)), amt_ensemble_field_ptr(epx, pf(6)), amt_ensemble_field_ptr(epx, pf(7)), &
                   amt_ensemble_field_ptr(epx, pf(8))), 'amt_ensemble_set_p_rho')
    call amt_check(amt_ensemble_set_uv(e, 1_c_int, 0_c_int, emdiv, cf1, cf2, cf3, amt_ensemble_field_ptr(eqx, qf(1)),         &
                   amt_ensemble_field_ptr(eqx, qf(2)), amt_ensemble_field_ptr(eqx, qf(3)), amt_ensemble_field_ptr(eqx, qf(4)), &
                   amt_ensemble_field_ptr(eqx, qf(5)), amt_ensemble_field_ptr(eqx, qf(6)), amt_ensemble_field_ptr(eqx, qf(7)), &
                   amt_ensemble_field_ptr(eqx, qf(8)), amt_ensemble_field_ptr(eqx, qf(9))), 'amt_ensemble_set_uv')
    if (.not. c_associated(amt_ensemble_uv_ptr(e, 2_c_int), amt_ensemble_field_ptr(eqx, qf(3)))) error stop 12
    call amt_check(amt_ensemble_stage_prep(e, 1_c_int), 'amt_ensemble_stage_prep')
    call amt_check(amt_ensemble_p_rho(e, 0_c_int), 'amt_ensemble_p_rho')
    call amt_check(amt_ensemble_uv(e), 'amt_ensemble_uv')
    call amt_check(amt_ensemble_sync(e), 'amt_ensemble_sync')
    print '(a,i0,a,es24.16)', 'advance_uv as a handle setting, on a domain in front of a sweep and on an ensemble of ', mm,      &
       ' members; checksum of u: ', sum(real(a3(its:ite, kts:kte-1, jts:jte-1), 8))
    call amt_check(amt_ensemble_destroy(e), 'amt_ensemble_destroy')
    call amt_check(amt_ensemble_destroy(eex), 'amt_ensemble_destroy')
    call amt_check(amt_ensemble_destroy(epx), 'amt_ensemble_destroy')
    call amt_check(amt_ensemble_destroy(eqx), 'amt_ensemble_destroy')
    call amt_check(amt_domain_destroy(d), 'amt_domain_destroy')
    call amt_check(amt_domain_destroy(ex), 'amt_domain_destroy')
    call amt_check(amt_domain_destroy(px), 'amt_domain_destroy')
    call amt_check(amt_domain_destroy(qx), 'amt_domain_destroy')
  end subroutine

  subroutine uv_device(h, px, nh)
    type(c_ptr), intent(in) :: h, px
    integer(c_int), intent(in) :: nh
    type(c_ptr) :: stream
    integer(c_int) :: fl(3)
    stream = amt_domain_stream(h)
    fl = [merge(1_c_int, 0_c_int, config_flags%periodic_x), merge(1_c_int, 0_c_int, config_flags%specified),               &
          merge(1_c_int, 0_c_int, config_flags%nested)]
    if (storage_size(rdx) == 64) then
       rc = amt_advance_uv_device_f64(stream, 1_c_int, nh, amt_domain_field_ptr(h, AMT_F_U), amt_domain_field_ptr(h, AMT_F_V),       &
               amt_domain_field_ptr(h, AMT_F_FT), amt_domain_field_ptr(h, AMT_F_FT), amt_domain_field_ptr(px, AMT_F_WW),          &
               amt_domain_field_ptr(px, AMT_F_WW_1), amt_domain_field_ptr(px, AMT_F_U), amt_domain_field_ptr(px, AMT_F_U_1),      &
               amt_domain_field_ptr(px, AMT_F_V), amt_domain_field_ptr(px, AMT_F_V_1), amt_domain_field_ptr(h, AMT_F_MU),         &
               amt_domain_field_ptr(h, AMT_F_MUU), amt_domain_field_ptr(h, AMT_F_MUV), amt_domain_field_ptr(h, AMT_F_MU_TEND),    &
               amt_domain_field_ptr(h, AMT_F_T), amt_domain_field_ptr(h, AMT_F_T_1), amt_domain_field_ptr(h, AMT_F_MSFTX),        &
               amt_domain_field_ptr(h, AMT_F_MSFUY), amt_domain_field_ptr(h, AMT_F_MSFTY),                                        &
               amt_domain_field_ptr(h, AMT_F_MSFVX_INV), amt_domain_field_ptr(h, AMT_F_MSFTY), amt_domain_field_ptr(h, AMT_F_FNM), &
               amt_domain_field_ptr(h, AMT_F_FNP), amt_domain_field_ptr(h, AMT_F_RDNW), real(rdx, c_double), real(rdy, c_double), &
               real(dts, c_double), 1.5_c_double, -0.75_c_double, 0.25_c_double, 0.01_c_double, fl(1), fl(2), fl(3),              &
               ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)
    else
       rc = amt_advance_uv_device_f32(stream, 1_c_int, nh, amt_domain_field_ptr(h, AMT_F_U), amt_domain_field_ptr(h, AMT_F_V),       &
               amt_domain_field_ptr(h, AMT_F_FT), amt_domain_field_ptr(h, AMT_F_FT), amt_domain_field_ptr(px, AMT_F_WW),          &
               amt_domain_field_ptr(px, AMT_F_WW_1), amt_domain_field_ptr(px, AMT_F_U), amt_domain_field_ptr(px, AMT_F_U_1),      &
               amt_domain_field_ptr(px, AMT_F_V), amt_domain_field_ptr(px, AMT_F_V_1), amt_domain_field_ptr(h, AMT_F_MU),         &
               amt_domain_field_ptr(h, AMT_F_MUU), amt_domain_field_ptr(h, AMT_F_MUV), amt_domain_field_ptr(h, AMT_F_MU_TEND),    &
               amt_domain_field_ptr(h, AMT_F_T), amt_domain_field_ptr(h, AMT_F_T_1), amt_domain_field_ptr(h, AMT_F_MSFTX),        &
               amt_domain_field_ptr(h, AMT_F_MSFUY), amt_domain_field_ptr(h, AMT_F_MSFTY),                                        &
               amt_domain_field_ptr(h, AMT_F_MSFVX_INV), amt_domain_field_ptr(h, AMT_F_MSFTY), amt_domain_field_ptr(h, AMT_F_FNM), &
               amt_domain_field_ptr(h, AMT_F_FNP), amt_domain_field_ptr(h, AMT_F_RDNW), real(rdx, c_float), real(rdy, c_float),   &
               real(dts, c_float), 1.5_c_float, -0.75_c_float, 0.25_c_float, 0.01_c_float, fl(1), fl(2), fl(3),                   &
               ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)
    end if
    call amt_check(rc, 'amt_advance_uv_device')
  end subroutine

  ! Two Runge-Kutta stages (rk_step 1 without, rk_step 2 with a diabatic heating) whose acoustic loops of nsmall sub-steps run
  ! between small_step_prep and small_step_finish on the device.  t_old, mu_old, mu_save, mub and h_diabatic are the caller's:
  ! arrays of a second handle of the same shape serve (filled from the generator, they come down with amt_domain_download).
  ! The same two stages are repeated with the pointer-level calls on a third handle and must give the same bits, and run on an
  ! ensemble with member-stacked arrays.
  subroutine stage_bracket()
    type(c_ptr) :: d, d2, ex, e, eex
    real(wp), allocatable, target :: a3(:,:,:), b3(:,:,:), a2(:,:), b2(:,:)
    integer(c_int) :: wb, px, sp, ne, mm, rk, k
    integer(c_int), parameter :: xf(4) = [AMT_F_T, AMT_F_MU, AMT_F_MUAVE, AMT_F_MUT]      ! of `ex`: t_old, mu_old, mu_save, mub
    integer(c_int), parameter :: f3(4) = [AMT_F_T, AMT_F_WW, AMT_F_T_1, AMT_F_WW_1], f2(2) = [AMT_F_MU, AMT_F_MUTS]
    character(len=4), parameter :: n3(4) = ['t   ', 'ww  ', 't_1 ', 'ww_1'], n2(2) = ['mu  ', 'muts']
    character(len=7), parameter :: nx(4) = ['t_old  ', 'mu_old ', 'mu_save', 'mub    ']
    wb = int(storage_size(rdx)/8, c_int)
    px = merge(1_c_int, 0_c_int, config_flags%periodic_x)
    sp = merge(1_c_int, 0_c_int, config_flags%specified)
    ne = merge(1_c_int, 0_c_int, config_flags%nested)
    mm = int(max(members, 1), c_int)
    allocate (a3(ims:ime,kms:kme,jms:jme), b3(ims:ime,kms:kme,jms:jme), a2(ims:ime,jms:jme), b2(ims:ime,jms:jme))
    call make_domain(d, seed)
    call make_domain(d2, seed)
    call make_domain(ex, seed + 1_c_int64_t)
    ! handle level: off until set, a mix of given and missing arrays is refused, then the caller's four
    if (c_associated(amt_domain_stage_ptr(d, 0_c_int))) error stop 8
    if (amt_domain_stage_prep(d, 1_c_int) /= AMT_ERR_PRECONDITION) error stop 8
    if (amt_domain_set_stage(d, 1_c_int, amt_domain_field_ptr(ex, xf(1)), c_null_ptr, c_null_ptr, c_null_ptr) /= AMT_ERR_INVALID_ARG) &
       error stop 8
    call amt_check(amt_domain_set_stage(d, 1_c_int, amt_domain_field_ptr(ex, xf(1)), amt_domain_field_ptr(ex, xf(2)),       &
                   amt_domain_field_ptr(ex, xf(3)), amt_domain_field_ptr(ex, xf(4))), 'amt_domain_set_stage')
    if (.not. c_associated(amt_domain_stage_ptr(d, 3_c_int), amt_domain_field_ptr(ex, xf(4)))) error stop 8
    do rk = 1, 2
       call amt_check(amt_domain_stage_prep(d, rk), 'amt_domain_stage_prep')
       call amt_check(amt_domain_step(d, int(nsmall, c_int)), 'amt_domain_step')
       call amt_check(amt_domain_stage_finish(d, int(nsmall, c_int), merge(amt_domain_field_ptr(ex, AMT_F_FT), c_null_ptr, rk == 2)), &
                      'amt_domain_stage_finish')
    end do
    call amt_check(amt_domain_sync(d), 'amt_domain_sync')
    ! pointer level on the third handle's arrays and stream: the same two stages
    do rk = 1, 2
       call stage_device(d2, ex, rk)
    end do
    call amt_check(amt_domain_sync(d2), 'amt_domain_sync')
    print '(a,i0,a)', 'two Runge-Kutta stages of ', nsmall, ' sub-steps between small_step_prep and small_step_finish on the device'
    do k = 1, 4
       call amt_check(amt_domain_download(d, f3(k), c_loc(a3)), 'amt_domain_download')
       call amt_check(amt_domain_download(d2, f3(k), c_loc(b3)), 'amt_domain_download')
       if (any(transfer(a3, 1_c_int8_t, size(a3) * wb) /= transfer(b3, 1_c_int8_t, size(b3) * wb))) error stop 9
       print '(a,a,a,es24.16)', 'checksum of ', n3(k), ' after the stages: ', sum(real(a3(its:ite-1, kts:kte-1, jts:jte-1), 8))
       if (len_trim(outdir) > 0) call dump3('stage_'//trim(n3(k)), a3)
    end do
    do k = 1, 2
       call amt_check(amt_domain_download(d, f2(k), c_loc(a2)), 'amt_domain_download')
       call amt_check(amt_domain_download(d2, f2(k), c_loc(b2)), 'amt_domain_download')
       if (any(transfer(a2, 1_c_int8_t, size(a2) * wb) /= transfer(b2, 1_c_int8_t, size(b2) * wb))) error stop 9
       if (len_trim(outdir) > 0) call dump2('stage_'//trim(n2(k)), a2)
    end do
    if (len_trim(outdir) > 0) then
       call amt_check(amt_domain_download(ex, xf(1), c_loc(a3)), 'amt_domain_download')
       call dump3('stage_'//trim(nx(1)), a3)
       do k = 2, 4
          call amt_check(amt_domain_download(ex, xf(k), c_loc(a2)), 'amt_domain_download')
          call dump2('stage_'//trim(nx(k)), a2)
       end do
    end if
    call amt_check(amt_domain_set_stage(d, 0_c_int, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr), 'amt_domain_set_stage')
    if (c_associated(amt_domain_stage_ptr(d, 3_c_int))) error stop 8
    call amt_check(amt_domain_destroy(d), 'amt_domain_destroy')
    call amt_check(amt_domain_destroy(d2), 'amt_domain_destroy')
    call amt_check(amt_domain_destroy(ex), 'amt_domain_destroy')
    ! an ensemble: every member's prep and finish in one launch each, the four arrays member-stacked in a second ensemble
    call make_ensemble(e, mm, seed)
    call make_ensemble(eex, mm, seed + 1_c_int64_t)
    call amt_check(amt_ensemble_set_stage(e, 1_c_int, amt_ensemble_field_ptr(eex, xf(1)), amt_ensemble_field_ptr(eex, xf(2)),  &
                   amt_ensemble_field_ptr(eex, xf(3)), amt_ensemble_field_ptr(eex, xf(4))), 'amt_ensemble_set_stage')
    if (.not. c_associated(amt_ensemble_stage_ptr(e, 0_c_int), amt_ensemble_field_ptr(eex, xf(1)))) error stop 8
    call amt_check(amt_ensemble_stage_prep(e, 1_c_int), 'amt_ensemble_stage_prep')
    call amt_check(amt_ensemble_step(e, int(nsmall, c_int)), 'amt_ensemble_step')
    call amt_check(amt_ensemble_stage_finish(e, int(nsmall, c_int), amt_ensemble_field_ptr(eex, AMT_F_FT)), 'amt_ensemble_stage_finish')
    call amt_check(amt_ensemble_sync(e), 'amt_ensemble_sync')
    print '(a,i0,a)', 'a Runge-Kutta stage of an ensemble of ', mm, ' members: one launch per pass'
    call amt_check(amt_ensemble_destroy(e), 'amt_ensemble_destroy')
    call amt_check(amt_ensemble_destroy(eex), 'amt_ensemble_destroy')
  end subroutine

  subroutine make_domain(h, fill_seed)
    type(c_ptr), intent(out) :: h
    integer(c_int64_t), intent(in) :: fill_seed
    call amt_check(amt_domain_create(h, int(storage_size(rdx)/8, c_int), merge(1_c_int, 0_c_int, config_flags%periodic_x),     &
                   merge(1_c_int, 0_c_int, config_flags%specified), merge(1_c_int, 0_c_int, config_flags%nested),            &
                   ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte), 'amt_domain_create')
    call amt_check(amt_domain_set_scalars(h, real(rdx, c_double), real(rdy, c_double), real(dts, c_double),                  &
                                          real(epssm, c_double)), 'amt_domain_set_scalars')
    call amt_check(amt_domain_fill_synthetic(h, fill_seed, int(ims, c_long), int(kms-1, c_long), int(jms, c_long),            &
                   int(ni+2, c_long), int(nk+1, c_long), int(nj+2, c_long)), 'amt_domain_fill_synthetic')
  end subroutine

  subroutine make_ensemble(h, mm, fill_seed)
    type(c_ptr), intent(out) :: h
    integer(c_int), intent(in) :: mm
    integer(c_int64_t), intent(in) :: fill_seed
    call amt_check(amt_ensemble_create(h, mm, int(storage_size(rdx)/8, c_int), merge(1_c_int, 0_c_int, config_flags%periodic_x), &
                   merge(1_c_int, 0_c_int, config_flags%specified), merge(1_c_int, 0_c_int, config_flags%nested),            &
                   ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte), 'amt_ensemble_create')
    call amt_check(amt_ensemble_set_scalars(h, real(rdx, c_double), real(rdy, c_double), real(dts, c_double),                &
                                            real(epssm, c_double)), 'amt_ensemble_set_scalars')
    call amt_check(amt_ensemble_fill_synthetic(h, fill_seed, int(ims, c_long), int(kms-1, c_long), int(jms, c_long),          &
                   int(ni+2, c_long), int(nk+1, c_long), int(nj+2, c_long)), 'amt_ensemble_fill_synthetic')
  end subroutine

  ! one stage on handle h's arrays with the pointer-level calls, on h's stream: prep, nsmall sweeps of the handle, finish
  subroutine stage_device(h, ex, rk)
    type(c_ptr), intent(in) :: h, ex
    integer(c_int), intent(in) :: rk
    type(c_ptr) :: p(0:25), stream, heat
    integer(c_int) :: f
    do f = 0, 25
       p(f) = amt_domain_field_ptr(h, f)
    end do
    stream = amt_domain_stream(h)
    heat = merge(amt_domain_field_ptr(ex, AMT_F_FT), c_null_ptr, rk == 2)
    if (storage_size(rdx) == 64) then
       rc = amt_stage_prep_device_f64(stream, 1_c_int, p(AMT_F_T), p(AMT_F_T_1), amt_domain_field_ptr(ex, AMT_F_T), p(AMT_F_WW), &
                                      p(AMT_F_WW_1), p(AMT_F_MU), amt_domain_field_ptr(ex, AMT_F_MU),                       &
                                      amt_domain_field_ptr(ex, AMT_F_MUAVE), p(AMT_F_MUTS), p(AMT_F_MUDF), p(AMT_F_MUT),      &
                                      amt_domain_field_ptr(ex, AMT_F_MUT), rk,                                              &
                                      ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)
    else
       rc = amt_stage_prep_device_f32(stream, 1_c_int, p(AMT_F_T), p(AMT_F_T_1), amt_domain_field_ptr(ex, AMT_F_T), p(AMT_F_WW), &
                                      p(AMT_F_WW_1), p(AMT_F_MU), amt_domain_field_ptr(ex, AMT_F_MU),                       &
                                      amt_domain_field_ptr(ex, AMT_F_MUAVE), p(AMT_F_MUTS), p(AMT_F_MUDF), p(AMT_F_MUT),      &
                                      amt_domain_field_ptr(ex, AMT_F_MUT), rk,                                              &
                                      ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)
    end if
    call amt_check(rc, 'amt_stage_prep_device')
    call amt_check(amt_domain_step(h, int(nsmall, c_int)), 'amt_domain_step')
    if (storage_size(rdx) == 64) then
       rc = amt_stage_finish_device_f64(stream, 1_c_int, p(AMT_F_T), p(AMT_F_T_1), p(AMT_F_WW), p(AMT_F_WW_1), p(AMT_F_MU),    &
                                        amt_domain_field_ptr(ex, AMT_F_MUAVE), p(AMT_F_MUTS), p(AMT_F_MUT),                  &
                                        real(dts, c_double), int(nsmall, c_int), heat,                                      &
                                        ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)
    else
       rc = amt_stage_finish_device_f32(stream, 1_c_int, p(AMT_F_T), p(AMT_F_T_1), p(AMT_F_WW), p(AMT_F_WW_1), p(AMT_F_MU),    &
                                        amt_domain_field_ptr(ex, AMT_F_MUAVE), p(AMT_F_MUTS), p(AMT_F_MUT),                  &
                                        real(dts, c_float), int(nsmall, c_int), heat,                                       &
                                        ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)
    end if
    call amt_check(rc, 'amt_stage_finish_device')
  end subroutine

  ! One acoustic loop of nsmall sub-steps with the flux averages kept on the device: the handle accumulates behind every sweep
  ! into arrays the library allocates; the same loop is then repeated with the pointer-level call into caller-owned arrays (the
  ! 3-D fields of a second handle of the same shape serve, and come down with amt_domain_download), and on an ensemble.
  subroutine flux_averages()
    type(c_ptr) :: d, e, outs, stream
    real(wp), allocatable, target :: o3(:,:,:)
    integer(c_int) :: wb, px, sp, ne, n, nxt, mm, it, acc(3)
    character(len=4), parameter :: aname(3) = ['ru_m', 'rv_m', 'ww_m']
    integer :: k
    wb = int(storage_size(rdx)/8, c_int)
    px = merge(1_c_int, 0_c_int, config_flags%periodic_x)
    sp = merge(1_c_int, 0_c_int, config_flags%specified)
    ne = merge(1_c_int, 0_c_int, config_flags%nested)
    mm = int(max(members, 1), c_int)
    acc = [AMT_F_T, AMT_F_T_AVE, AMT_F_FT]                      ! the caller-owned accumulators: three 3-D arrays of `outs`
    allocate (o3(ims:ime,kms:kme,jms:jme))
    call amt_check(amt_domain_create(d, wb, px, sp, ne, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,             &
                                     its, ite, jts, jte, kts, kte), 'amt_domain_create')
    call amt_check(amt_domain_create(outs, wb, px, sp, ne, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,          &
                                     its, ite, jts, jte, kts, kte), 'amt_domain_create')
    call amt_check(amt_domain_set_scalars(d, real(rdx, c_double), real(rdy, c_double), real(dts, c_double),              &
                                          real(epssm, c_double)), 'amt_domain_set_scalars')
    call amt_check(amt_domain_fill_synthetic(d, seed, int(ims, c_long), int(kms-1, c_long), int(jms, c_long),            &
                   int(ni+2, c_long), int(nk+1, c_long), int(nj+2, c_long)), 'amt_domain_fill_synthetic')
    o3 = 0.0_wp                                                 ! what a cell outside the tile box keeps
    do k = 1, 3
       call amt_check(amt_domain_upload(outs, acc(k), c_loc(o3)), 'amt_domain_upload')
    end do
    ! handle level, library-owned accumulators: one accumulation behind every sweep, the counter wraps after nsmall
    call amt_check(amt_domain_set_sumflux(d, int(nsmall, c_int), c_null_ptr, c_null_ptr, c_null_ptr), 'amt_domain_set_sumflux')
    call amt_check(amt_domain_step(d, int(nsmall, c_int)), 'amt_domain_step')
    call amt_check(amt_domain_sumflux_state(d, n, nxt), 'amt_domain_sumflux_state')
    if (n /= nsmall .or. nxt /= 1 .or. .not. c_associated(amt_domain_sumflux_ptr(d, 2_c_int))) error stop 6
    ! the caller's arrays: the same loop accumulated by hand, then by the pointer-level call on the handle's stream
    call amt_check(amt_domain_set_sumflux(d, int(nsmall, c_int), amt_domain_field_ptr(outs, acc(1)),                     &
                   amt_domain_field_ptr(outs, acc(2)), amt_domain_field_ptr(outs, acc(3))), 'amt_domain_set_sumflux')
    do it = 1, int(nsmall, c_int)
       call amt_check(amt_domain_sumflux_accumulate(d), 'amt_domain_sumflux_accumulate')
    end do
    call amt_check(amt_domain_set_sumflux(d, 0_c_int, c_null_ptr, c_null_ptr, c_null_ptr), 'amt_domain_set_sumflux')
    stream = amt_domain_stream(d)
    do it = 1, int(nsmall, c_int)
       call sumflux_device(stream, 1_c_int, it, amt_domain_field_ptr(outs, acc(1)), amt_domain_field_ptr(outs, acc(2)),    &
                           amt_domain_field_ptr(outs, acc(3)), d, .false.)
    end do
    call amt_check(amt_domain_sync(d), 'amt_domain_sync')
    print '(a,i0,a)', 'flux averages over ', nsmall, ' sub-steps on the device (ru_m, rv_m, ww_m)'
    do k = 1, 3
       call amt_check(amt_domain_download(outs, acc(k), c_loc(o3)), 'amt_domain_download')
       print '(a,a,a,es24.16)', 'checksum of ', aname(k), ' over the tile: ', sum(real(o3(its:ite, kts:kte, jts:jte), 8))
       if (len_trim(outdir) > 0) call dump3(aname(k), o3)
    end do
    call amt_check(amt_domain_destroy(d), 'amt_domain_destroy')
    call amt_check(amt_domain_destroy(outs), 'amt_domain_destroy')
    ! an ensemble: every member's accumulation in one launch
    call amt_check(amt_ensemble_create(e, mm, wb, px, sp, ne, ids, ide, jds, jde, kde,                                     &
                                       ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte), 'amt_ensemble_create')
    call amt_check(amt_ensemble_set_scalars(e, real(rdx, c_double), real(rdy, c_double), real(dts, c_double),            &
                                            real(epssm, c_double)), 'amt_ensemble_set_scalars')
    call amt_check(amt_ensemble_fill_synthetic(e, seed, int(ims, c_long), int(kms-1, c_long), int(jms, c_long),          &
                   int(ni+2, c_long), int(nk+1, c_long), int(nj+2, c_long)), 'amt_ensemble_fill_synthetic')
    call amt_check(amt_ensemble_set_sumflux(e, int(nsmall, c_int), c_null_ptr, c_null_ptr, c_null_ptr), 'amt_ensemble_set_sumflux')
    call amt_check(amt_ensemble_step(e, int(nsmall, c_int)), 'amt_ensemble_step')
    call amt_check(amt_ensemble_sumflux_accumulate(e), 'amt_ensemble_sumflux_accumulate')      ! iteration 1 of the next loop
    call amt_check(amt_ensemble_sumflux_state(e, n, nxt), 'amt_ensemble_sumflux_state')
    if (n /= nsmall .or. nxt /= merge(1, 2, nsmall == 1)) error stop 7
    ! pointer level on the member-stacked arrays, into the library's accumulators: iteration 1 once more (acc is not read)
    call sumflux_device(amt_ensemble_stream(e), mm, 1_c_int, amt_ensemble_sumflux_ptr(e, 0_c_int),                          &
                        amt_ensemble_sumflux_ptr(e, 1_c_int), amt_ensemble_sumflux_ptr(e, 2_c_int), e, .true.)
    call amt_check(amt_ensemble_sync(e), 'amt_ensemble_sync')
    print '(a,i0,a)', 'flux averages of an ensemble of ', mm, ' members: one launch per sub-step'
    call amt_check(amt_ensemble_destroy(e), 'amt_ensemble_destroy')
  end subroutine

  subroutine sumflux_device(stream, mm, it, ru_m, rv_m, ww_m, h, is_ensemble)
    type(c_ptr), intent(in) :: stream, ru_m, rv_m, ww_m, h
    integer(c_int), intent(in) :: mm, it
    logical, intent(in) :: is_ensemble
    type(c_ptr) :: p(0:25)
    integer(c_int) :: f
    do f = 0, 25
       if (is_ensemble) then
          p(f) = amt_ensemble_field_ptr(h, f)
       else
          p(f) = amt_domain_field_ptr(h, f)
       end if
    end do
    if (storage_size(rdx) == 64) then
       rc = amt_sumflux_device_f64(stream, mm, ru_m, rv_m, ww_m, p(AMT_F_U), p(AMT_F_V), p(AMT_F_WW), p(AMT_F_U_1),        &
                                   p(AMT_F_V_1), p(AMT_F_WW_1), p(AMT_F_MUU), p(AMT_F_MUV), p(AMT_F_MSFUY),               &
                                   p(AMT_F_MSFVX_INV), it, int(nsmall, c_int),                                            &
                                   ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)
    else
       rc = amt_sumflux_device_f32(stream, mm, ru_m, rv_m, ww_m, p(AMT_F_U), p(AMT_F_V), p(AMT_F_WW), p(AMT_F_U_1),        &
                                   p(AMT_F_V_1), p(AMT_F_WW_1), p(AMT_F_MUU), p(AMT_F_MUV), p(AMT_F_MSFUY),               &
                                   p(AMT_F_MSFVX_INV), it, int(nsmall, c_int),                                            &
                                   ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)
    end if
    call amt_check(rc, 'amt_sumflux_device')
  end subroutine

  ! An ensemble of `members` members of this shape, stepped nsweeps times, and what a host asks of it at an output time: the
  ! mean, the sample variance and the envelope over the members, computed where the members live.  The outputs are arrays of
  ! ONE member's extents: those of a second amt_domain of the same shape serve, and come down with amt_domain_download.
  subroutine ensemble_moments()
    type(c_ptr) :: ens, outs, stream
    real(wp), allocatable, target :: o3(:,:,:), o2(:,:)
    integer(c_int) :: wb, px, sp, ne, fw(4), ft4(4), fm(4)
    character(len=4), parameter :: mname(4) = ['mean', 'var ', 'lo  ', 'hi  ']
    integer :: k
    wb = int(storage_size(rdx)/8, c_int)
    px = merge(1_c_int, 0_c_int, config_flags%periodic_x)
    sp = merge(1_c_int, 0_c_int, config_flags%specified)
    ne = merge(1_c_int, 0_c_int, config_flags%nested)
    fw = [AMT_F_WW, AMT_F_WW_1, AMT_F_U, AMT_F_U_1]          ! the output arrays: four rank-3 fields each for ww and t,
    ft4 = [AMT_F_T, AMT_F_T_1, AMT_F_T_AVE, AMT_F_FT]        ! four rank-2 fields for mu
    fm = [AMT_F_MU, AMT_F_MUT, AMT_F_MUAVE, AMT_F_MUTS]
    allocate (o3(ims:ime,kms:kme,jms:jme), o2(ims:ime,jms:jme))
    call amt_check(amt_ensemble_create(ens, int(members, c_int), wb, px, sp, ne, ids, ide, jds, jde, kde,                  &
                                       ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte), 'amt_ensemble_create')
    call amt_check(amt_ensemble_set_scalars(ens, real(rdx, c_double), real(rdy, c_double), real(dts, c_double),          &
                                            real(epssm, c_double)), 'amt_ensemble_set_scalars')
    call amt_check(amt_ensemble_fill_synthetic(ens, seed, int(ims, c_long), int(kms-1, c_long), int(jms, c_long),        &
                   int(ni+2, c_long), int(nk+1, c_long), int(nj+2, c_long)), 'amt_ensemble_fill_synthetic')
    call amt_check(amt_ensemble_step(ens, int(nsweeps, c_int)), 'amt_ensemble_step')
    call amt_check(amt_domain_create(outs, wb, px, sp, ne, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,         &
                                     its, ite, jts, jte, kts, kte), 'amt_domain_create')
    o3 = 0.0_wp; o2 = 0.0_wp                                  ! what a cell outside the box keeps
    do k = 1, 4
       call amt_check(amt_domain_upload(outs, fw(k), c_loc(o3)), 'amt_domain_upload')
       call amt_check(amt_domain_upload(outs, ft4(k), c_loc(o3)), 'amt_domain_upload')
       call amt_check(amt_domain_upload(outs, fm(k), c_loc(o2)), 'amt_domain_upload')
    end do
    ! handle level, on the ensemble's stream behind the sweeps: no wait in between
    call amt_check(amt_ensemble_moments(ens, AMT_F_WW, AMT_REGION_MEMORY, amt_domain_field_ptr(outs, fw(1)),             &
                   amt_domain_field_ptr(outs, fw(2)), amt_domain_field_ptr(outs, fw(3)), amt_domain_field_ptr(outs, fw(4))), &
                   'amt_ensemble_moments (ww)')
    call amt_check(amt_ensemble_moments(ens, AMT_F_MU, AMT_REGION_WINDOW, amt_domain_field_ptr(outs, fm(1)),             &
                   amt_domain_field_ptr(outs, fm(2)), amt_domain_field_ptr(outs, fm(3)), amt_domain_field_ptr(outs, fm(4))), &
                   'amt_ensemble_moments (mu)')
    ! pointer level, for a host that keeps its own stacked arrays: a box one cell inside the memory, on the same stream
    stream = amt_ensemble_stream(ens)
    if (wb == 8) then
       rc = amt_moments_device_f64(stream, amt_ensemble_field_ptr(ens, AMT_F_T), 3_c_int, int(members, c_int),           &
                                   ims, ime, jms, jme, kms, kme, ims + 1, ime - 1, kms + 1, kme - 1, jms + 1, jme - 1,   &
                                   amt_domain_field_ptr(outs, ft4(1)), amt_domain_field_ptr(outs, ft4(2)),                &
                                   amt_domain_field_ptr(outs, ft4(3)), amt_domain_field_ptr(outs, ft4(4)))
    else
       rc = amt_moments_device_f32(stream, amt_ensemble_field_ptr(ens, AMT_F_T), 3_c_int, int(members, c_int),           &
                                   ims, ime, jms, jme, kms, kme, ims + 1, ime - 1, kms + 1, kme - 1, jms + 1, jme - 1,   &
                                   amt_domain_field_ptr(outs, ft4(1)), amt_domain_field_ptr(outs, ft4(2)),                &
                                   amt_domain_field_ptr(outs, ft4(3)), amt_domain_field_ptr(outs, ft4(4)))
    end if
    call amt_check(rc, 'amt_moments_device')
    call amt_check(amt_ensemble_sync(ens), 'amt_ensemble_sync')
    print '(a,i0,a,i0,a)', 'ensemble of ', members, ' members, ', nsweeps, ' sweeps: mean / var / lo / hi of ww, mu and t on the device'
    do k = 1, 4
       call amt_check(amt_domain_download(outs, fw(k), c_loc(o3)), 'amt_domain_download')
       if (k == 1) print '(a,es24.16)', 'checksum of the ensemble-mean ww: ', sum(real(o3, 8))
       if (len_trim(outdir) > 0) call dump3('ens_ww_'//trim(mname(k)), o3)
       call amt_check(amt_domain_download(outs, ft4(k), c_loc(o3)), 'amt_domain_download')
       if (len_trim(outdir) > 0) call dump3('ens_t_'//trim(mname(k)), o3)
       call amt_check(amt_domain_download(outs, fm(k), c_loc(o2)), 'amt_domain_download')
       if (len_trim(outdir) > 0) call dump2('ens_mu_'//trim(mname(k)), o2)
    end do
    call amt_check(amt_domain_destroy(outs), 'amt_domain_destroy')
    call amt_check(amt_ensemble_destroy(ens), 'amt_ensemble_destroy')
  end subroutine

  subroutine fill3(field, a)
    integer(c_int), intent(in) :: field
    real(wp), target, intent(inout) :: a(ims:, kms:, jms:)
    call amt_check(amt_synth_fill_host(field, int(storage_size(rdx)/8, c_int), c_loc(a), seed,         &
         int(ime-ims+1, c_long), int(kme-kms+1, c_long), int(jme-jms+1, c_long),                        &
         int(ims, c_long), int(kms-1, c_long), int(jms, c_long),                                        &
         int(ni+2, c_long), int(nk+1, c_long), int(nj+2, c_long)), 'amt_synth_fill_host')
  end subroutine
  subroutine fill2(field, a)
    integer(c_int), intent(in) :: field
    real(wp), target, intent(inout) :: a(ims:, jms:)
    call amt_check(amt_synth_fill_host(field, int(storage_size(rdx)/8, c_int), c_loc(a), seed,         &
         int(ime-ims+1, c_long), 1_c_long, int(jme-jms+1, c_long),                                      &
         int(ims, c_long), 0_c_long, int(jms, c_long),                                                  &
         int(ni+2, c_long), int(nk+1, c_long), int(nj+2, c_long)), 'amt_synth_fill_host')
  end subroutine
  subroutine fill1(field, a)
    integer(c_int), intent(in) :: field
    real(wp), target, intent(inout) :: a(kms:)
    call amt_check(amt_synth_fill_host(field, int(storage_size(rdx)/8, c_int), c_loc(a), seed,         &
         1_c_long, int(kme-kms+1, c_long), 1_c_long, 0_c_long, int(kms-1, c_long), 0_c_long,            &
         int(ni+2, c_long), int(nk+1, c_long), int(nj+2, c_long)), 'amt_synth_fill_host')
  end subroutine
  subroutine up(field, host)
    integer(c_int), intent(in) :: field
    type(c_ptr), intent(in) :: host
    call amt_check(amt_domain_upload(dom, field, host), 'amt_domain_upload')
  end subroutine
  subroutine dn(field, host)
    integer(c_int), intent(in) :: field
    type(c_ptr), intent(in) :: host
    call amt_check(amt_domain_download(dom, field, host), 'amt_domain_download')
  end subroutine
  subroutine swap3(a, b)
    real(wp), intent(inout) :: a(:,:,:), b(:,:,:)
    real(wp) :: x
    integer :: i, k, j
    do j = 1, size(a, 3)
      do k = 1, size(a, 2)
        do i = 1, size(a, 1)
          x = a(i, k, j); a(i, k, j) = b(i, k, j); b(i, k, j) = x
        end do
      end do
    end do
  end subroutine
  subroutine swap2(a, b)
    real(wp), intent(inout) :: a(:,:), b(:,:)
    real(wp) :: x
    integer :: i, j
    do j = 1, size(a, 2)
      do i = 1, size(a, 1)
        x = a(i, j); a(i, j) = b(i, j); b(i, j) = x
      end do
    end do
  end subroutine
  subroutine pin3(a)
    real(wp), target, intent(inout) :: a(:,:,:)
    call amt_check(amt_host_pin(c_loc(a), int(size(a), c_size_t) * int(storage_size(rdx) / 8, c_size_t)), 'amt_host_pin')
  end subroutine
  subroutine unpin3(a)
    real(wp), target, intent(inout) :: a(:,:,:)
    call amt_check(amt_host_unpin(c_loc(a)), 'amt_host_unpin')
  end subroutine
  subroutine dump3(name, a)
    character(len=*), intent(in) :: name
    real(wp), intent(in) :: a(:,:,:)
    integer :: un
    open (newunit=un, file=trim(outdir)//'/'//name//'.bin', access='stream', form='unformatted', status='replace')
    write (un) a
    close (un)
  end subroutine
  subroutine dump2(name, a)
    character(len=*), intent(in) :: name
    real(wp), intent(in) :: a(:,:)
    integer :: un
    open (newunit=un, file=trim(outdir)//'/'//name//'.bin', access='stream', form='unformatted', status='replace')
    write (un) a
    close (un)
  end subroutine

end program advance_mu_t_driver
