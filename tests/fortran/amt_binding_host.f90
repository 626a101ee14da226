! amt_binding_host.f90 -- a Fortran host that calls the interfaces of amt_c_binding.f90 the three drivers do not reach:
! ensembles, cyclic refresh, the boundary zone, statistics / compare / guard, the host-owned halo exchange, the pointer-level
! device calls and the planners.  One sub-command per scenario; raw arrays go to <outdir>/<stage>_<field>.bin, records and
! read-backs to <outdir>/records.txt as text (doubles as their 64-bit patterns).  tests/test_gpu_21b_fortran_bindings.py and
! tests/test_fortran_binding_contract.py run it and compare everything with the oracle and the numpy references.
!
!   amt_binding_host CMD OUTDIR MEMBERS VARIANT PX SP NE  IDS IDE JDS JDE KDE IMS IME JMS JME KMS KME ITS ITE JTS JTE KTS KTE
!                    GNI GNK GNJ SEED RDX RDY DTS EPSSM [PI PJ [FLAGS]]
!   CMD: ensemble | cyclic | specbdy | diag | halo | oneshot | plan
!   Built twice: default REAL is fp32, or fp64 with -fdefault-real-8 (as the drivers are).
program amt_binding_host
  use iso_c_binding
  use, intrinsic :: ieee_arithmetic
  use amt_c_binding
  implicit none

  integer, parameter :: wp = kind(1.0)
  integer(c_int), parameter :: wb = storage_size(1.0_wp) / 8
  integer, parameter :: NF = 26
  character(len=9), parameter :: fname(0:NF-1) = [character(len=9) :: 'ww', 'ww_1', 'u', 'u_1', 'v', 'v_1', 'mu', 'mut',   &
     'muave', 'muts', 'muu', 'muv', 'mudf', 't', 't_1', 't_ave', 'ft', 'mu_tend', 'dnw', 'fnm', 'fnp', 'rdnw', 'msfuy',       &
     'msfvx_inv', 'msftx', 'msfty']
  type field_t
     real(wp), allocatable :: a(:)              ! member-stacked: u(ims:ime, kms:kme, jms:jme, members) flattened
  end type
  type(field_t), target :: f(0:NF-1)
  real(wp), allocatable, target :: tmp(:)

  character(len=512) :: cmd, outdir, arg
  integer(c_int) :: members, variant, px, sp, ne
  integer(c_int) :: ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte
  integer :: gni, gnk, gnj, pi, pj, pflags
  integer(c_int) :: gids, gide, gjds, gjde      ! the whole domain's, while ims .. jte hold one patch's (halo, plan)
  integer(c_int) :: rb(8, 0:1)                  ! ims, ime, jms, jme, its, ite, jts, jte of the two ranks of the halo scenario
  integer(c_int64_t) :: seed
  real(c_double) :: rdx, rdy, dts, epssm
  integer :: ru

  if (command_argument_count() < 32) then
     print '(a)', 'usage: amt_binding_host CMD OUTDIR MEMBERS VARIANT PX SP NE <17 bounds> GNI GNK GNJ SEED RDX RDY DTS EPSSM [PI PJ [FLAGS]]'
     error stop 2
  end if
  call get_command_argument(1, cmd)
  call get_command_argument(2, outdir)
  members = iarg(3); variant = iarg(4); px = iarg(5); sp = iarg(6); ne = iarg(7)
  ids = iarg(8);  ide = iarg(9);  jds = iarg(10); jde = iarg(11); kde = iarg(12)
  ims = iarg(13); ime = iarg(14); jms = iarg(15); jme = iarg(16); kms = iarg(17); kme = iarg(18)
  its = iarg(19); ite = iarg(20); jts = iarg(21); jte = iarg(22); kts = iarg(23); kte = iarg(24)
  gni = iarg(25); gnk = iarg(26); gnj = iarg(27)
  call get_command_argument(28, arg); read (arg, *) seed
  rdx = darg(29); rdy = darg(30); dts = darg(31); epssm = darg(32)
  pi = 1; pj = 1; pflags = 0
  if (command_argument_count() >= 34) then
     pi = iarg(33); pj = iarg(34)
  end if
  if (command_argument_count() >= 35) pflags = iarg(35)
  open (newunit=ru, file=trim(outdir)//'/records.txt', status='replace', action='write')
  write (ru, '(a,i0)') 'real_bytes ', wb

  select case (trim(cmd))
  case ('ensemble'); call run_ensemble()
  case ('cyclic');   call run_cyclic()
  case ('specbdy');  call run_specbdy()
  case ('diag');     call run_diag()
  case ('halo');     call run_halo()
  case ('oneshot');  call run_oneshot()
  case ('plan');     call run_plan()
  case default
     print '(a,a)', 'unknown command ', trim(cmd)
     error stop 2
  end select
  write (ru, '(a)') 'done'
  close (ru)

contains

  ! ------------------------------------------------------------------------------------------------------------------
  ! arguments, shapes, host arrays
  ! ------------------------------------------------------------------------------------------------------------------
  integer function iarg(n)
    integer, intent(in) :: n
    character(len=64) :: s
    call get_command_argument(n, s); read (s, *) iarg
  end function
  real(c_double) function darg(n)
    integer, intent(in) :: n
    character(len=64) :: s
    call get_command_argument(n, s); read (s, *) darg
  end function
  integer function frank(fid)
    integer, intent(in) :: fid
    select case (fid)
    case (AMT_F_WW, AMT_F_WW_1, AMT_F_U, AMT_F_U_1, AMT_F_V, AMT_F_V_1, AMT_F_T, AMT_F_T_1, AMT_F_T_AVE, AMT_F_FT); frank = 3
    case (AMT_F_DNW, AMT_F_FNM, AMT_F_FNP, AMT_F_RDNW); frank = 1
    case default; frank = 2
    end select
  end function
  integer function fsize(fid)                 ! elements of ONE member
    integer, intent(in) :: fid
    integer :: idim, kdim, jdim
    idim = ime - ims + 1; kdim = kme - kms + 1; jdim = jme - jms + 1
    select case (frank(fid))
    case (3); fsize = idim * kdim * jdim
    case (2); fsize = idim * jdim
    case default; fsize = kdim
    end select
  end function
  integer function fmembers(fid, mm)          ! the 1-D metric arrays are shared
    integer, intent(in) :: fid, mm
    fmembers = merge(1, mm, frank(fid) == 1)
  end function

  subroutine alloc_fields(mm)
    integer, intent(in) :: mm
    integer :: fid
    do fid = 0, NF - 1
       if (allocated(f(fid)%a)) deallocate (f(fid)%a)
       allocate (f(fid)%a(fsize(fid) * fmembers(fid, mm)))
    end do
    if (allocated(tmp)) deallocate (tmp)
    allocate (tmp(fsize(AMT_F_WW) * mm))
  end subroutine

  ! member m (0-based) of every field from the generator with seed s0 + m, as amt_ensemble_fill_synthetic does on the device
  subroutine fill_fields_host(mm, s0)
    integer, intent(in) :: mm
    integer(c_int64_t), intent(in) :: s0
    integer :: fid, m
    do fid = 0, NF - 1
       do m = 0, fmembers(fid, mm) - 1
          call amt_check(amt_synth_fill_host(int(fid, c_int), wb, c_loc(f(fid)%a(m * fsize(fid) + 1)), s0 + m,             &
               int(ime-ims+1, c_long), int(kme-kms+1, c_long), int(jme-jms+1, c_long),                                     &
               int(ims, c_long), int(kms-1, c_long), int(jms, c_long),                                                     &
               int(gni+2, c_long), int(gnk+1, c_long), int(gnj+2, c_long)), 'amt_synth_fill_host')
       end do
    end do
  end subroutine

  subroutine write_bin(stage, fid, n, a)
    character(len=*), intent(in) :: stage
    integer, intent(in) :: fid, n
    real(wp), intent(in) :: a(*)
    integer :: un
    open (newunit=un, file=trim(outdir)//'/'//stage//'_'//trim(fname(fid))//'.bin', access='stream', form='unformatted', &
          status='replace')
    write (un) a(1:n)
    close (un)
  end subroutine

  integer(c_int64_t) function bits(x)
    real(c_double), intent(in) :: x
    bits = transfer(x, 1_c_int64_t)
  end function

  real(wp) function nan_payload()
    if (wb == 8) then
       nan_payload = transfer(int(z'7ff800000000beef', c_int64_t), 1.0_wp)
    else
       nan_payload = transfer(int(z'7fc0beef', c_int32_t), 1.0_wp)
    end if
  end function

  ! one value into cell (i, k, j) of every member of a rank-3 field / (i, j) of a rank-2 field, through the 4-D / 3-D view
  subroutine set3(fid, i, k, j, x, only_member)
    integer, intent(in) :: fid, i, k, j
    real(wp), intent(in) :: x
    integer, intent(in), optional :: only_member
    real(wp), pointer :: a4(:,:,:,:)
    integer :: mm
    mm = size(f(fid)%a) / fsize(fid)
    a4(ims:ime, kms:kme, jms:jme, 1:mm) => f(fid)%a
    if (present(only_member)) then
       a4(i, k, j, only_member + 1) = x
    else
       a4(i, k, j, :) = x
    end if
  end subroutine
  subroutine set2(fid, i, j, x, only_member)
    integer, intent(in) :: fid, i, j
    real(wp), intent(in) :: x
    integer, intent(in), optional :: only_member
    real(wp), pointer :: a3(:,:,:)
    integer :: mm
    mm = size(f(fid)%a) / fsize(fid)
    a3(ims:ime, jms:jme, 1:mm) => f(fid)%a
    if (present(only_member)) then
       a3(i, j, only_member + 1) = x
    else
       a3(i, j, :) = x
    end if
  end subroutine
  real(wp) function get3(fid, i, k, j, m)     ! member m, 0-based
    integer, intent(in) :: fid, i, k, j, m
    real(wp), pointer :: a4(:,:,:,:)
    integer :: mm
    mm = size(f(fid)%a) / fsize(fid)
    a4(ims:ime, kms:kme, jms:jme, 1:mm) => f(fid)%a
    get3 = a4(i, k, j, m + 1)
  end function
  real(wp) function get2(fid, i, j, m)
    integer, intent(in) :: fid, i, j, m
    real(wp), pointer :: a3(:,:,:)
    integer :: mm
    mm = size(f(fid)%a) / fsize(fid)
    a3(ims:ime, jms:jme, 1:mm) => f(fid)%a
    get2 = a3(i, j, m + 1)
  end function
  ! whole column i / whole row j (every level, every member) of a field
  subroutine plant_col(fid, i, x)
    integer, intent(in) :: fid, i
    real(wp), intent(in) :: x
    real(wp), pointer :: a4(:,:,:,:), a3(:,:,:)
    integer :: mm
    mm = size(f(fid)%a) / fsize(fid)
    if (frank(fid) == 3) then
       a4(ims:ime, kms:kme, jms:jme, 1:mm) => f(fid)%a
       a4(i, :, :, :) = x
    else
       a3(ims:ime, jms:jme, 1:mm) => f(fid)%a
       a3(i, :, :) = x
    end if
  end subroutine
  subroutine plant_row(fid, j, x)
    integer, intent(in) :: fid, j
    real(wp), intent(in) :: x
    real(wp), pointer :: a4(:,:,:,:), a3(:,:,:)
    integer :: mm
    mm = size(f(fid)%a) / fsize(fid)
    if (frank(fid) == 3) then
       a4(ims:ime, kms:kme, jms:jme, 1:mm) => f(fid)%a
       a4(:, :, j, :) = x
    else
       a3(ims:ime, jms:jme, 1:mm) => f(fid)%a
       a3(:, j, :) = x
    end if
  end subroutine

  ! ------------------------------------------------------------------------------------------------------------------
  ! handles: create, upload, dump
  ! ------------------------------------------------------------------------------------------------------------------
  subroutine dom_create(d)
    type(c_ptr), intent(out) :: d
    call amt_check(amt_domain_create(d, wb, px, sp, ne, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,             &
                                     its, ite, jts, jte, kts, kte), 'amt_domain_create')
    call amt_check(amt_domain_set_scalars(d, rdx, rdy, dts, epssm), 'amt_domain_set_scalars')
    call amt_check(amt_domain_set_variant(d, variant), 'amt_domain_set_variant')
  end subroutine
  subroutine ens_create(e)
    type(c_ptr), intent(out) :: e
    call amt_check(amt_ensemble_create(e, members, wb, px, sp, ne, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,  &
                                       its, ite, jts, jte, kts, kte), 'amt_ensemble_create')
    call amt_check(amt_ensemble_set_scalars(e, rdx, rdy, dts, epssm), 'amt_ensemble_set_scalars')
    call amt_check(amt_ensemble_set_variant(e, variant), 'amt_ensemble_set_variant')
  end subroutine
  ! member m (0-based) of the host arrays into a domain handle; by_rows: the rank-3 and rank-2 fields through
  ! amt_domain_upload_rows over jms..jme
  subroutine dom_upload_all(d, m, by_rows)
    type(c_ptr), intent(in) :: d
    integer, intent(in) :: m
    logical, intent(in), optional :: by_rows
    integer :: fid, off
    logical :: rows
    rows = .false.
    if (present(by_rows)) rows = by_rows
    do fid = 0, NF - 1
       off = merge(0, m, frank(fid) == 1) * fsize(fid) + 1
       if (rows .and. frank(fid) > 1) then
          call amt_check(amt_domain_upload_rows(d, int(fid, c_int), jms, jme, c_loc(f(fid)%a(off))), 'amt_domain_upload_rows')
       else
          call amt_check(amt_domain_upload(d, int(fid, c_int), c_loc(f(fid)%a(off))), 'amt_domain_upload')
       end if
    end do
  end subroutine
  subroutine dom_dump_all(d, stage, by_rows)
    type(c_ptr), intent(in) :: d
    character(len=*), intent(in) :: stage
    logical, intent(in), optional :: by_rows
    integer :: fid
    logical :: rows
    rows = .false.
    if (present(by_rows)) rows = by_rows
    do fid = 0, NF - 1
       if (rows .and. frank(fid) > 1) then
          call amt_check(amt_domain_download_rows(d, int(fid, c_int), jms, jme, c_loc(tmp)), 'amt_domain_download_rows')
       else
          call amt_check(amt_domain_download(d, int(fid, c_int), c_loc(tmp)), 'amt_domain_download')
       end if
       call write_bin(stage, fid, fsize(fid), tmp)
    end do
  end subroutine
  ! every member of every field, each from its slice of the 4-D / 3-D host array
  subroutine ens_upload_all(e)
    type(c_ptr), intent(in) :: e
    real(wp), pointer :: a4(:,:,:,:), a3(:,:,:)
    integer :: fid, m
    do fid = 0, NF - 1
       do m = 0, members - 1
          select case (frank(fid))
          case (3)
             a4(ims:ime, kms:kme, jms:jme, 1:members) => f(fid)%a
             call amt_check(amt_ensemble_upload_member(e, int(fid, c_int), int(m, c_int), c_loc(a4(ims, kms, jms, m + 1))),  &
                            'amt_ensemble_upload_member')
          case (2)
             a3(ims:ime, jms:jme, 1:members) => f(fid)%a
             call amt_check(amt_ensemble_upload_member(e, int(fid, c_int), int(m, c_int), c_loc(a3(ims, jms, m + 1))),       &
                            'amt_ensemble_upload_member')
          case default
             call amt_check(amt_ensemble_upload_member(e, int(fid, c_int), int(m, c_int), c_loc(f(fid)%a)),                 &
                            'amt_ensemble_upload_member')
          end select
       end do
    end do
  end subroutine
  subroutine ens_dump_all(e, stage)
    type(c_ptr), intent(in) :: e
    character(len=*), intent(in) :: stage
    integer :: fid, m, mm
    do fid = 0, NF - 1
       mm = fmembers(fid, int(members))
       do m = 0, mm - 1
          call amt_check(amt_ensemble_download_member(e, int(fid, c_int), int(m, c_int), c_loc(tmp(m * fsize(fid) + 1))),   &
                         'amt_ensemble_download_member')
       end do
       call write_bin(stage, fid, fsize(fid) * mm, tmp)
    end do
  end subroutine
  subroutine dom_ptrs(d, p)
    type(c_ptr), intent(in) :: d
    type(c_ptr), intent(out) :: p(0:NF-1)
    integer :: fid
    do fid = 0, NF - 1
       p(fid) = amt_domain_field_ptr(d, int(fid, c_int))
       if (.not. c_associated(p(fid))) error stop 3
    end do
  end subroutine
  subroutine ens_ptrs(e, p)
    type(c_ptr), intent(in) :: e
    type(c_ptr), intent(out) :: p(0:NF-1)
    integer :: fid
    do fid = 0, NF - 1
       p(fid) = amt_ensemble_field_ptr(e, int(fid, c_int))
       if (.not. c_associated(p(fid))) error stop 3
    end do
  end subroutine

  ! ------------------------------------------------------------------------------------------------------------------
  ! the pointer-level calls, fp32 or fp64 by this build's REAL; mm = 0: the single-patch interface
  ! ------------------------------------------------------------------------------------------------------------------
  subroutine advance_device(stream, mm, p)
    type(c_ptr), intent(in) :: stream, p(0:NF-1)
    integer(c_int), intent(in) :: mm
    integer(c_int) :: rc
    if (wb == 8 .and. mm == 0) then
       rc = amt_advance_mu_t_device_f64(stream, variant, p(0), p(1), p(2), p(3), p(4), p(5), p(6), p(7), p(8), p(9), p(10), &
            p(11), p(12), p(13), p(14), p(15), p(16), p(17), rdx, rdy, dts, epssm, p(18), p(19), p(20), p(21), p(22), p(23), &
            p(24), p(25), px, sp, ne, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)
    else if (wb == 8) then
       rc = amt_advance_mu_t_ensemble_device_f64(stream, variant, mm, p(0), p(1), p(2), p(3), p(4), p(5), p(6), p(7), p(8),  &
            p(9), p(10), p(11), p(12), p(13), p(14), p(15), p(16), p(17), rdx, rdy, dts, epssm, p(18), p(19), p(20), p(21),   &
            p(22), p(23), p(24), p(25), px, sp, ne, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,                    &
            its, ite, jts, jte, kts, kte)
    else if (mm == 0) then
       rc = amt_advance_mu_t_device_f32(stream, variant, p(0), p(1), p(2), p(3), p(4), p(5), p(6), p(7), p(8), p(9), p(10), &
            p(11), p(12), p(13), p(14), p(15), p(16), p(17), real(rdx, c_float), real(rdy, c_float), real(dts, c_float),     &
            real(epssm, c_float), p(18), p(19), p(20), p(21), p(22), p(23), p(24), p(25), px, sp, ne,                        &
            ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)
    else
       rc = amt_advance_mu_t_ensemble_device_f32(stream, variant, mm, p(0), p(1), p(2), p(3), p(4), p(5), p(6), p(7), p(8),  &
            p(9), p(10), p(11), p(12), p(13), p(14), p(15), p(16), p(17), real(rdx, c_float), real(rdy, c_float),             &
            real(dts, c_float), real(epssm, c_float), p(18), p(19), p(20), p(21), p(22), p(23), p(24), p(25), px, sp, ne,     &
            ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)
    end if
    call amt_check(rc, 'amt_advance_mu_t[_ensemble]_device')
  end subroutine
  subroutine cyclic_device(stream, axes, mm, p)
    type(c_ptr), intent(in) :: stream, p(0:NF-1)
    integer(c_int), intent(in) :: axes, mm
    integer(c_int) :: rc
    if (wb == 8) then
       rc = amt_cyclic_fill_device_f64(stream, axes, mm, p(AMT_F_U), p(AMT_F_U_1), p(AMT_F_V), p(AMT_F_V_1), p(AMT_F_T_1),   &
            p(AMT_F_MUU), p(AMT_F_MUV), p(AMT_F_MSFUY), p(AMT_F_MSFVX_INV), px, sp, ne,                                     &
            ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)
    else
       rc = amt_cyclic_fill_device_f32(stream, axes, mm, p(AMT_F_U), p(AMT_F_U_1), p(AMT_F_V), p(AMT_F_V_1), p(AMT_F_T_1),   &
            p(AMT_F_MUU), p(AMT_F_MUV), p(AMT_F_MSFUY), p(AMT_F_MSFVX_INV), px, sp, ne,                                     &
            ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)
    end if
    call amt_check(rc, 'amt_cyclic_fill_device')
  end subroutine
  subroutine spec_bdy_device(stream, mm, p)
    type(c_ptr), intent(in) :: stream, p(0:NF-1)
    integer(c_int), intent(in) :: mm
    integer(c_int) :: rc
    if (wb == 8) then
       rc = amt_spec_bdy_update_device_f64(stream, mm, p(AMT_F_T), p(AMT_F_FT), p(AMT_F_MU), p(AMT_F_MUTS), p(AMT_F_MU_TEND), &
            dts, px, sp, ne, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)
    else
       rc = amt_spec_bdy_update_device_f32(stream, mm, p(AMT_F_T), p(AMT_F_FT), p(AMT_F_MU), p(AMT_F_MUTS), p(AMT_F_MU_TEND), &
            real(dts, c_float), px, sp, ne, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,                           &
            its, ite, jts, jte, kts, kte)
    end if
    call amt_check(rc, 'amt_spec_bdy_update_device')
  end subroutine

  ! ------------------------------------------------------------------------------------------------------------------
  ! records
  ! ------------------------------------------------------------------------------------------------------------------
  subroutine rec_stats(what, name, region, m, s)
    character(len=*), intent(in) :: what, name
    integer, intent(in) :: region, m
    type(amt_field_stats), intent(in) :: s
    write (ru, '(a,1x,a,1x,i0,1x,i0,8(1x,i0))') what, trim(name), region, m, s%count, s%n_nan, s%n_inf, s%first_nonfinite,   &
         bits(s%min), bits(s%max), bits(s%max_abs), bits(s%sum)
  end subroutine
  subroutine rec_diff(what, name, region, m, d)
    character(len=*), intent(in) :: what, name
    integer, intent(in) :: region, m
    type(amt_field_diff), intent(in) :: d
    write (ru, '(a,1x,a,1x,i0,1x,i0,4(1x,i0))') what, trim(name), region, m, d%count, d%n_diff, d%first_diff,                &
         bits(d%max_abs_diff)
  end subroutine
  subroutine rec_guard(what, rc, g)
    character(len=*), intent(in) :: what
    integer(c_int), intent(in) :: rc
    type(amt_guard_report), intent(in) :: g
    write (ru, '(a,7(1x,i0))') what, rc, g%sweeps_checked, g%sweep, g%field, g%member, g%offset, g%n_nonfinite
  end subroutine
  subroutine rec_int(what, v)
    character(len=*), intent(in) :: what
    integer, intent(in) :: v
    write (ru, '(a,1x,i0)') what, v
  end subroutine
  subroutine rec_last_error(what)
    character(len=*), intent(in) :: what
    call rec_cstr(what, amt_last_error())
  end subroutine
  subroutine rec_cstr(what, cptr)                ! a NUL-terminated C string the library owns
    character(len=*), intent(in) :: what
    type(c_ptr), intent(in) :: cptr
    character(kind=c_char), pointer :: cmsg(:)
    character(len=400) :: msg
    integer :: n
    call c_f_pointer(cptr, cmsg, [400])
    msg = ' '
    do n = 1, 400
       if (cmsg(n) == c_null_char) exit
       msg(n:n) = cmsg(n)
    end do
    write (ru, '(a,1x,a)') what, trim(msg)
  end subroutine

  ! ------------------------------------------------------------------------------------------------------------------
  ! ensemble: handle stepping, the device drop-ins for an ensemble and for a single patch, wrap, compare of two handles
  ! ------------------------------------------------------------------------------------------------------------------
  subroutine run_ensemble()
    type(c_ptr) :: e1, e2, ew, d, dw, p(0:NF-1), stream
    type(amt_field_diff) :: df(16)
    real(c_float) :: ms, tries(8)
    integer(c_int) :: w(6)
    integer :: fid, m
    call alloc_fields(int(members))
    call fill_fields_host(int(members), seed)
    call ens_create(e1)
    call rec_int('members', int(amt_ensemble_members(e1)))
    call ens_upload_all(e1)
    ! a second handle filled on the device: bit-equal to the uploaded one, field by field, member by member
    call ens_create(e2)
    call amt_check(amt_ensemble_fill_synthetic(e2, seed, int(ims, c_long), int(kms-1, c_long), int(jms, c_long),            &
                   int(gni+2, c_long), int(gnk+1, c_long), int(gnj+2, c_long)), 'amt_ensemble_fill_synthetic')
    call amt_check(amt_ensemble_sync(e2), 'amt_ensemble_sync')
    do fid = 0, NF - 1
       if (frank(fid) == 1) cycle
       call amt_check(amt_ensemble_compare(e1, e2, int(fid, c_int), AMT_REGION_MEMORY, df), 'amt_ensemble_compare')
       do m = 1, members
          call rec_diff('ecompare', fname(fid), int(AMT_REGION_MEMORY), m - 1, df(m))
       end do
    end do
    call amt_check(amt_ensemble_destroy(e2), 'amt_ensemble_destroy')
    ! two sweeps on the handle
    call amt_check(amt_ensemble_step(e1, 2_c_int), 'amt_ensemble_step')
    call amt_check(amt_ensemble_sync(e1), 'amt_ensemble_sync')
    call ens_dump_all(e1, 'step2')
    ! a third through the ensemble's device drop-in, on the handle's pointers and stream
    call ens_ptrs(e1, p)
    stream = amt_ensemble_stream(e1)
    call advance_device(stream, members, p)
    call amt_check(amt_ensemble_sync(e1), 'amt_ensemble_sync')
    call ens_dump_all(e1, 'dev3')
    ! a fourth through a handle wrapped over the same pointers
    call amt_check(amt_ensemble_wrap(ew, members, wb, px, sp, ne, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,    &
                                     its, ite, jts, jte, kts, kte, p, stream), 'amt_ensemble_wrap')
    call amt_check(amt_ensemble_set_scalars(ew, rdx, rdy, dts, epssm), 'amt_ensemble_set_scalars')
    call amt_check(amt_ensemble_set_variant(ew, variant), 'amt_ensemble_set_variant')
    call amt_check(amt_ensemble_step_timed(ew, 1_c_int, ms), 'amt_ensemble_step_timed')
    call amt_check(amt_ensemble_destroy(ew), 'amt_ensemble_destroy')
    call ens_dump_all(e1, 'wrap4')
    call amt_check(amt_ensemble_destroy(e1), 'amt_ensemble_destroy')

    ! the single patch the same way: member 0, one sweep through amt_advance_mu_t_device_*, one through amt_domain_wrap
    call dom_create(d)
    call dom_upload_all(d, 0, by_rows=.true.)
    call dom_ptrs(d, p)
    stream = amt_domain_stream(d)
    ! t_1 zeroed on the device, then filled there by the generator: the bits the host fill gave
    tmp = 0.0_wp
    call amt_check(amt_domain_upload(d, AMT_F_T_1, c_loc(tmp)), 'amt_domain_upload')
    call amt_check(amt_synth_fill_device(stream, AMT_F_T_1, wb, p(AMT_F_T_1), seed,                                          &
                   int(ime-ims+1, c_long), int(kme-kms+1, c_long), int(jme-jms+1, c_long),                                  &
                   int(ims, c_long), int(kms-1, c_long), int(jms, c_long),                                                  &
                   int(gni+2, c_long), int(gnk+1, c_long), int(gnj+2, c_long)), 'amt_synth_fill_device')
    call advance_device(stream, 0_c_int, p)
    call amt_check(amt_domain_sync(d), 'amt_domain_sync')
    call dom_dump_all(d, 'one1', by_rows=.true.)
    call amt_check(amt_domain_wrap(dw, wb, px, sp, ne, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme,               &
                                   its, ite, jts, jte, kts, kte, p, stream), 'amt_domain_wrap')
    call amt_check(amt_domain_set_scalars(dw, rdx, rdy, dts, epssm), 'amt_domain_set_scalars')
    call amt_check(amt_domain_set_variant(dw, variant), 'amt_domain_set_variant')
    call amt_check(amt_domain_step(dw, 1_c_int), 'amt_domain_step')
    call amt_check(amt_domain_sync(dw), 'amt_domain_sync')
    call amt_check(amt_domain_destroy(dw), 'amt_domain_destroy')
    call dom_dump_all(d, 'one2')
    call rec_int('placement', int(amt_domain_placement(d, tries, 8_c_int)))
    call amt_check(amt_domain_destroy(d), 'amt_domain_destroy')
    ! host arithmetic
    call amt_check(amt_compute_window(px, sp, ne, ids, ide, jds, jde, its, ite, jts, jte, kts, kte,                          &
                                      w(1), w(2), w(3), w(4), w(5), w(6)), 'amt_compute_window')
    write (ru, '(a,6(1x,i0))') 'window', w
    call rec_int('rows_for_members', int(amt_march_rows_for_members(int((ite - its) / 16 + 1, c_long), members,              &
                                        int(jte - jts + 1, c_int), 256_c_int, 1000000_c_long, wb, 1_c_int)))
    call rec_int('rows_for', int(amt_march_rows_for(int((ite - its) / 16 + 1, c_long), int(jte - jts + 1, c_int),           &
                                                    256_c_int, 1000000_c_long, wb, 1_c_int)))
  end subroutine

  ! ------------------------------------------------------------------------------------------------------------------
  ! cyclic: NaN payloads in every destination cell; the refresh alone, pointer level, armed stepping; the ensemble twins
  ! ------------------------------------------------------------------------------------------------------------------
  subroutine plant_cyclic_destinations()
    real(wp) :: x
    x = nan_payload()
    call plant_col(AMT_F_U, int(ide), x); call plant_col(AMT_F_U_1, int(ide), x); call plant_col(AMT_F_T_1, int(ide), x)
    call plant_col(AMT_F_MUU, int(ide), x); call plant_col(AMT_F_MSFUY, int(ide), x)
    call plant_col(AMT_F_T_1, int(ids - 1), x)
    call plant_row(AMT_F_V, int(jde), x); call plant_row(AMT_F_V_1, int(jde), x); call plant_row(AMT_F_T_1, int(jde), x)
    call plant_row(AMT_F_MUV, int(jde), x); call plant_row(AMT_F_MSFVX_INV, int(jde), x)
    call plant_row(AMT_F_T_1, int(jds - 1), x)
  end subroutine
  subroutine run_cyclic()
    type(c_ptr) :: d, e, p(0:NF-1)
    integer(c_int) :: axes
    axes = AMT_CYCLIC_X + AMT_CYCLIC_Y
    call alloc_fields(int(members))
    call fill_fields_host(int(members), seed)
    call plant_cyclic_destinations()
    call dom_create(d)
    call dom_upload_all(d, 0)
    call amt_check(amt_domain_cyclic_fill(d, axes), 'amt_domain_cyclic_fill')
    call amt_check(amt_domain_sync(d), 'amt_domain_sync')
    call rec_int('cyclic_after_fill', int(amt_domain_cyclic(d)))
    call dom_dump_all(d, 'fill')
    call dom_upload_all(d, 0)
    call dom_ptrs(d, p)
    call cyclic_device(amt_domain_stream(d), axes, 1_c_int, p)
    call amt_check(amt_domain_sync(d), 'amt_domain_sync')
    call dom_dump_all(d, 'ptr')
    call dom_upload_all(d, 0)
    call amt_check(amt_domain_set_cyclic(d, axes), 'amt_domain_set_cyclic')
    call rec_int('cyclic_set', int(amt_domain_cyclic(d)))
    call amt_check(amt_domain_step(d, 2_c_int), 'amt_domain_step')
    call amt_check(amt_domain_sync(d), 'amt_domain_sync')
    call dom_dump_all(d, 'step')
    call amt_check(amt_domain_destroy(d), 'amt_domain_destroy')

    call ens_create(e)
    call ens_upload_all(e)
    call amt_check(amt_ensemble_cyclic_fill(e, axes), 'amt_ensemble_cyclic_fill')
    call amt_check(amt_ensemble_sync(e), 'amt_ensemble_sync')
    call rec_int('ecyclic_after_fill', int(amt_ensemble_cyclic(e)))
    call ens_dump_all(e, 'efill')
    call ens_upload_all(e)
    call ens_ptrs(e, p)
    call cyclic_device(amt_ensemble_stream(e), axes, members, p)
    call amt_check(amt_ensemble_sync(e), 'amt_ensemble_sync')
    call ens_dump_all(e, 'eptr')
    call ens_upload_all(e)
    call amt_check(amt_ensemble_set_cyclic(e, axes), 'amt_ensemble_set_cyclic')
    call rec_int('ecyclic_set', int(amt_ensemble_cyclic(e)))
    call amt_check(amt_ensemble_step(e, 2_c_int), 'amt_ensemble_step')
    call amt_check(amt_ensemble_sync(e), 'amt_ensemble_sync')
    call ens_dump_all(e, 'estep')
    call amt_check(amt_ensemble_destroy(e), 'amt_ensemble_destroy')
  end subroutine

  ! ------------------------------------------------------------------------------------------------------------------
  ! boundary zone of a specified / nested domain: the update alone, pointer level, behind every sweep; the ensemble twins
  ! ------------------------------------------------------------------------------------------------------------------
  subroutine run_specbdy()
    type(c_ptr) :: d, e, p(0:NF-1)
    call alloc_fields(int(members))
    call fill_fields_host(int(members), seed)
    call dom_create(d)
    call dom_upload_all(d, 0)
    call amt_check(amt_domain_spec_bdy_update(d), 'amt_domain_spec_bdy_update')
    call amt_check(amt_domain_sync(d), 'amt_domain_sync')
    call rec_int('spec_bdy_after_update', int(amt_domain_spec_bdy(d)))
    call dom_dump_all(d, 'upd')
    call dom_upload_all(d, 0)
    call dom_ptrs(d, p)
    call spec_bdy_device(amt_domain_stream(d), 1_c_int, p)
    call amt_check(amt_domain_sync(d), 'amt_domain_sync')
    call dom_dump_all(d, 'ptr')
    call dom_upload_all(d, 0)
    call amt_check(amt_domain_set_spec_bdy(d, 1_c_int), 'amt_domain_set_spec_bdy')
    call rec_int('spec_bdy_set', int(amt_domain_spec_bdy(d)))
    call amt_check(amt_domain_step(d, 2_c_int), 'amt_domain_step')
    call amt_check(amt_domain_sync(d), 'amt_domain_sync')
    call dom_dump_all(d, 'step')
    call amt_check(amt_domain_destroy(d), 'amt_domain_destroy')

    call ens_create(e)
    call ens_upload_all(e)
    call amt_check(amt_ensemble_spec_bdy_update(e), 'amt_ensemble_spec_bdy_update')
    call amt_check(amt_ensemble_sync(e), 'amt_ensemble_sync')
    call rec_int('espec_bdy_after_update', int(amt_ensemble_spec_bdy(e)))
    call ens_dump_all(e, 'eupd')
    call ens_upload_all(e)
    call ens_ptrs(e, p)
    call spec_bdy_device(amt_ensemble_stream(e), members, p)
    call amt_check(amt_ensemble_sync(e), 'amt_ensemble_sync')
    call ens_dump_all(e, 'eptr')
    call ens_upload_all(e)
    call amt_check(amt_ensemble_set_spec_bdy(e, 1_c_int), 'amt_ensemble_set_spec_bdy')
    call rec_int('espec_bdy_set', int(amt_ensemble_spec_bdy(e)))
    call amt_check(amt_ensemble_step(e, 2_c_int), 'amt_ensemble_step')
    call amt_check(amt_ensemble_sync(e), 'amt_ensemble_sync')
    call ens_dump_all(e, 'estep')
    call amt_check(amt_ensemble_destroy(e), 'amt_ensemble_destroy')
  end subroutine

  ! ------------------------------------------------------------------------------------------------------------------
  ! statistics, compare, guard.  Planted cells are fixed offsets from (its, kts, jts): the checker plants the same.
  ! ------------------------------------------------------------------------------------------------------------------
  subroutine plant_specials()
    real(wp) :: x
    x = 1.0_wp
    call set3(AMT_F_T, its + 2, kts + 2, jts + 1, ieee_value(x, ieee_quiet_nan))
    call set3(AMT_F_T, its + 4, kts + 1, jts + 2, ieee_value(x, ieee_positive_inf))
    call set3(AMT_F_T, its + 1, kts + 3, jts + 3, ieee_value(x, ieee_negative_inf))
    call set3(AMT_F_T, its + 3, kts + 2, jts + 2, -0.0_wp)
    call set2(AMT_F_MU, its + 2, jts + 2, ieee_value(x, ieee_quiet_nan))
    call set2(AMT_F_MU, its + 5, jts + 1, ieee_value(x, ieee_negative_inf))
    call set2(AMT_F_MU, its + 3, jts + 3, ieee_value(x, ieee_positive_inf))
    call set2(AMT_F_MU, its + 1, jts + 3, -0.0_wp)
  end subroutine
  ! three cells of t and three of mu that differ from the planted state: a sign of zero, a finite step, a NaN made finite
  subroutine plant_differences()
    integer :: m
    call set3(AMT_F_T, its + 3, kts + 2, jts + 2, 0.0_wp)
    call set3(AMT_F_T, its + 2, kts + 2, jts + 1, 1.0_wp)
    call set2(AMT_F_MU, its + 1, jts + 3, 0.0_wp)
    do m = 0, members - 1                         ! each member's own value, stepped
       call set3(AMT_F_T, its + 6, kts + 1, jts + 1, get3(AMT_F_T, its + 6, kts + 1, jts + 1, m) + 0.5_wp, only_member=m)
       call set2(AMT_F_MU, its + 4, jts + 2, get2(AMT_F_MU, its + 4, jts + 2, m) - 1.25_wp, only_member=m)
       call set2(AMT_F_MU, its + 6, jts + 1, -get2(AMT_F_MU, its + 6, jts + 1, m), only_member=m)
    end do
  end subroutine
  subroutine run_diag()
    type(c_ptr) :: d, d2, e, e2, pa(0:NF-1), pb(0:NF-1), stream
    type(amt_field_stats) :: st(16)
    type(amt_field_diff) :: df(16)
    type(amt_guard_report) :: g
    integer(c_int) :: rc, region, box(6)
    integer :: k, m, fid
    real(wp) :: x
    x = 1.0_wp
    call alloc_fields(int(members))
    call fill_fields_host(int(members), seed)
    call plant_specials()
    call dom_create(d)
    call dom_upload_all(d, 0)
    call ens_create(e)
    call ens_upload_all(e)
    do k = 1, 2
       fid = merge(AMT_F_T, AMT_F_MU, k == 1)
       do region = AMT_REGION_WINDOW, AMT_REGION_MEMORY
          call amt_check(amt_domain_field_stats(d, int(fid, c_int), region, st), 'amt_domain_field_stats')
          call rec_stats('dstats', fname(fid), int(region), 0, st(1))
          call amt_check(amt_ensemble_field_stats(e, int(fid, c_int), region, st), 'amt_ensemble_field_stats')
          do m = 1, members
             call rec_stats('estats', fname(fid), int(region), m - 1, st(m))
          end do
       end do
    end do
    ! pointer level: a box strictly inside the extents, the first two members of the stacked arrays
    box = [ims + 1, ime - 1, kms + 1, kme - 1, jms + 1, jme - 1]
    call ens_ptrs(e, pa)
    stream = amt_ensemble_stream(e)
    do k = 1, 2
       fid = merge(AMT_F_T, AMT_F_MU, k == 1)
       if (wb == 8) then
          rc = amt_stats_device_f64(stream, pa(fid), int(frank(fid), c_int), 2_c_int, ims, ime, jms, jme, kms, kme,         &
                                    box(1), box(2), box(3), box(4), box(5), box(6), st)
       else
          rc = amt_stats_device_f32(stream, pa(fid), int(frank(fid), c_int), 2_c_int, ims, ime, jms, jme, kms, kme,         &
                                    box(1), box(2), box(3), box(4), box(5), box(6), st)
       end if
       call amt_check(rc, 'amt_stats_device')
       do m = 1, 2
          call rec_stats('pstats', fname(fid), 9, m - 1, st(m))
       end do
    end do
    ! a second state that differs in three cells of t and three of mu
    call plant_differences()
    call dom_create(d2)
    call dom_upload_all(d2, 0)
    call ens_create(e2)
    call ens_upload_all(e2)
    call ens_ptrs(e2, pb)
    do k = 1, 2
       fid = merge(AMT_F_T, AMT_F_MU, k == 1)
       do region = AMT_REGION_WINDOW, AMT_REGION_MEMORY
          call amt_check(amt_domain_compare(d, d2, int(fid, c_int), region, df), 'amt_domain_compare')
          call rec_diff('dcompare', fname(fid), int(region), 0, df(1))
       end do
       if (wb == 8) then
          rc = amt_compare_device_f64(stream, pa(fid), pb(fid), int(frank(fid), c_int), 2_c_int, ims, ime, jms, jme,        &
                                      kms, kme, box(1), box(2), box(3), box(4), box(5), box(6), df)
       else
          rc = amt_compare_device_f32(stream, pa(fid), pb(fid), int(frank(fid), c_int), 2_c_int, ims, ime, jms, jme,        &
                                      kms, kme, box(1), box(2), box(3), box(4), box(5), box(6), df)
       end if
       call amt_check(rc, 'amt_compare_device')
       do m = 1, 2
          call rec_diff('pcompare', fname(fid), 9, m - 1, df(m))
       end do
    end do
    call amt_check(amt_domain_destroy(d2), 'amt_domain_destroy')
    call amt_check(amt_ensemble_destroy(e2), 'amt_ensemble_destroy')
    call amt_check(amt_domain_destroy(d), 'amt_domain_destroy')
    call amt_check(amt_ensemble_destroy(e), 'amt_ensemble_destroy')

    ! the guard: clean inputs but for ONE NaN in ft (a domain), in ft of member 1 only (an ensemble)
    call fill_fields_host(int(members), seed)
    call set3(AMT_F_FT, its + 3, kts + 2, jts + 2, ieee_value(x, ieee_quiet_nan), only_member=0)
    call dom_create(d)
    call dom_upload_all(d, 0)
    call amt_check(amt_domain_guard_report(d, g), 'amt_domain_guard_report')
    call rec_guard('dguard_off', 0_c_int, g)
    call amt_check(amt_domain_set_guard(d, 2_c_int), 'amt_domain_set_guard')
    call amt_check(amt_domain_step(d, 4_c_int), 'amt_domain_step')
    rc = amt_domain_sync(d)
    if (rc /= AMT_OK .and. rc /= AMT_ERR_NONFINITE) call amt_check(rc, 'amt_domain_sync')
    call rec_last_error('dguard_message')
    call amt_check(amt_domain_guard_report(d, g), 'amt_domain_guard_report')
    call rec_guard('dguard', rc, g)
    call amt_check(amt_domain_set_guard(d, 0_c_int), 'amt_domain_set_guard')
    call amt_check(amt_domain_destroy(d), 'amt_domain_destroy')

    call fill_fields_host(int(members), seed)
    call set3(AMT_F_FT, its + 3, kts + 2, jts + 2, ieee_value(x, ieee_quiet_nan), only_member=1)
    call ens_create(e)
    call ens_upload_all(e)
    call amt_check(amt_ensemble_set_guard(e, 1_c_int), 'amt_ensemble_set_guard')
    call amt_check(amt_ensemble_step(e, 2_c_int), 'amt_ensemble_step')
    rc = amt_ensemble_sync(e)
    if (rc /= AMT_OK .and. rc /= AMT_ERR_NONFINITE) call amt_check(rc, 'amt_ensemble_sync')
    call amt_check(amt_ensemble_guard_report(e, g), 'amt_ensemble_guard_report')
    call rec_guard('eguard', rc, g)
    call amt_check(amt_ensemble_set_guard(e, 0_c_int), 'amt_ensemble_set_guard')
    call amt_check(amt_ensemble_destroy(e), 'amt_ensemble_destroy')
  end subroutine

  ! ------------------------------------------------------------------------------------------------------------------
  ! host-owned halos: BOTH ranks of a 2 x 1 grid (PI = 2) or of a 1 x 2 slab pair (PJ = 2) in this one process; the two MPI
  ! calls of INTEGRATION.md section 8 are an array copy from one rank's send buffer to the other's receive buffer
  ! ------------------------------------------------------------------------------------------------------------------
  subroutine patch_bounds(ri, rj)
    integer, intent(in) :: ri, rj
    integer :: ncol, nrow
    ncol = gide - gids; nrow = gjde - gjds
    its = gids + (ncol * ri) / pi; ite = gids + (ncol * (ri + 1)) / pi - 1
    jts = gjds + (nrow * rj) / pj; jte = gjds + (nrow * (rj + 1)) / pj - 1
    ims = its - 1; ime = ite + 1; jms = jts - 1; jme = jte + 1
  end subroutine
  integer function opposite(side)
    integer(c_int), intent(in) :: side
    select case (side)
    case (AMT_SIDE_BELOW); opposite = AMT_SIDE_ABOVE
    case (AMT_SIDE_ABOVE); opposite = AMT_SIDE_BELOW
    case (AMT_SIDE_LEFT);  opposite = AMT_SIDE_RIGHT
    case default;          opposite = AMT_SIDE_LEFT
    end select
  end function
  subroutine carry(msg, nmsg)
    type(amt_halo_message), intent(in) :: msg(4, 0:1)
    integer(c_int), intent(in) :: nmsg(0:1)
    integer(c_int8_t), pointer :: sbuf(:), rbuf(:)
    integer :: r, m, o, found
    do r = 0, 1
       do m = 1, nmsg(r)
          found = 0
          do o = 1, nmsg(msg(m, r)%peer)
             if (msg(o, msg(m, r)%peer)%peer == r .and. msg(o, msg(m, r)%peer)%side == opposite(msg(m, r)%side)) found = o
          end do
          if (found == 0) error stop 4
          if (msg(found, msg(m, r)%peer)%recv_bytes /= msg(m, r)%send_bytes) error stop 5
          call c_f_pointer(msg(m, r)%send, sbuf, [msg(m, r)%send_bytes])
          call c_f_pointer(msg(found, msg(m, r)%peer)%recv, rbuf, [msg(m, r)%send_bytes])
          rbuf = sbuf
       end do
    end do
  end subroutine
  subroutine run_halo()
    type(c_ptr) :: dom(0:1), h(0:1), g1
    type(amt_halo_message) :: msg(4, 0:1)
    integer(c_int) :: nmsg(0:1), sides(0:1), flags, rc
    integer :: r, s, m
    logical :: slab
    character(kind=c_char) :: uid(128)
    if (pi * pj /= 2) error stop 6
    slab = (pi == 1)
    gids = ids; gide = ide; gjds = jds; gjde = jde
    flags = ior(AMT_SLAB_TRANSPORT_EXTERNAL, AMT_SLAB_EXTERNAL_HOST_BUFFERS)
    do r = 0, 1
       call patch_bounds(mod(r, pi), r / pi)
       rb(:, r) = [ims, ime, jms, jme, its, ite, jts, jte]
       call dom_create(dom(r))
       call amt_check(amt_domain_fill_synthetic(dom(r), seed, int(ims, c_long), int(kms-1, c_long), int(jms, c_long),        &
                      int(gni+2, c_long), int(gnk+1, c_long), int(gnj+2, c_long)), 'amt_domain_fill_synthetic')
       if (slab) then
          call amt_check(amt_slab_create(h(r), dom(r), int(r, c_int), 2_c_int, c_null_ptr, flags), 'amt_slab_create')
          call amt_check(amt_slab_halo_messages(h(r), msg(:, r), 4_c_int, nmsg(r)), 'amt_slab_halo_messages')
       else
          call amt_check(amt_grid_create(h(r), dom(r), int(mod(r, pi), c_int), int(r / pi, c_int), int(pi, c_int),          &
                                         int(pj, c_int), c_null_ptr, flags), 'amt_grid_create')
          call amt_check(amt_grid_halo_messages(h(r), msg(:, r), 4_c_int, nmsg(r)), 'amt_grid_halo_messages')
       end if
       if (slab) then
          call rec_cstr('transport', amt_slab_transport(h(r)))
       else
          call rec_cstr('transport', amt_grid_transport(h(r)))
       end if
       sides(r) = 0
       do m = 1, nmsg(r)
          sides(r) = sides(r) + msg(m, r)%side
          write (ru, '(a,7(1x,i0))') 'message', r, msg(m, r)%side, msg(m, r)%peer, msg(m, r)%send_bytes, msg(m, r)%recv_bytes, &
               msg(m, r)%on_host, merge(1, 0, c_associated(msg(m, r)%send) .and. c_associated(msg(m, r)%recv))
       end do
    end do
    do s = 0, 1
       do r = 0, 1
          call next_inputs(dom(r), r, s, sides(r))
       end do
       do r = 0, 1
          if (slab) then
             call amt_check(amt_slab_step_begin(h(r)), 'amt_slab_step_begin')
          else
             call amt_check(amt_grid_step_begin(h(r)), 'amt_grid_step_begin')
          end if
       end do
       do r = 0, 1
          if (slab) then
             call amt_check(amt_slab_halo_wait(h(r)), 'amt_slab_halo_wait')
          else
             call amt_check(amt_grid_halo_wait(h(r)), 'amt_grid_halo_wait')
          end if
       end do
       call carry(msg, nmsg)
       do r = 0, 1
          if (slab) then
             call amt_check(amt_slab_step_end(h(r)), 'amt_slab_step_end')
          else
             call amt_check(amt_grid_step_end(h(r)), 'amt_grid_step_end')
          end if
       end do
    end do
    do r = 0, 1
       call sync_rank(h(r), slab)
       call dump_rank(dom(r), r, 'step')
    end do
    ! the two halves of an exchange without any compute: new inputs, pack, move, unpack
    do r = 0, 1
       call next_inputs(dom(r), r, 2, sides(r))
       if (slab) then
          call amt_check(amt_slab_halo_pack(h(r)), 'amt_slab_halo_pack')
       else
          call amt_check(amt_grid_halo_pack(h(r)), 'amt_grid_halo_pack')
       end if
    end do
    do r = 0, 1
       call sync_rank(h(r), slab)
    end do
    call carry(msg, nmsg)
    do r = 0, 1
       if (slab) then
          call amt_check(amt_slab_halo_unpack(h(r)), 'amt_slab_halo_unpack')
       else
          call amt_check(amt_grid_halo_unpack(h(r)), 'amt_grid_halo_unpack')
       end if
       call sync_rank(h(r), slab)
       call dump_rank(dom(r), r, 'pack')
    end do
    do r = 0, 1
       if (slab) then
          call amt_check(amt_slab_destroy(h(r)), 'amt_slab_destroy')
       else
          call amt_check(amt_grid_destroy(h(r)), 'amt_grid_destroy')
       end if
    end do
    ! a grid of one patch has nobody to exchange with: amt_grid_exchange is then a call that moves nothing
    call amt_check(amt_grid_create(g1, dom(0), 0_c_int, 0_c_int, 1_c_int, 1_c_int, c_null_ptr, 0_c_int), 'amt_grid_create 1x1')
    rc = amt_grid_exchange(g1)
    call rec_int('grid_exchange_1x1', int(rc))
    call amt_check(amt_grid_step(g1, 1_c_int), 'amt_grid_step')       ! rank 0's patch as it stands, halos and all: one plain sweep
    call amt_check(amt_grid_sync(g1), 'amt_grid_sync')
    call dump_rank(dom(0), 0, 'grid')
    call rec_cstr('transport_1x1', amt_grid_transport(g1))
    call amt_check(amt_grid_destroy(g1), 'amt_grid_destroy')
    call amt_check(amt_slab_create(g1, dom(1), 0_c_int, 1_c_int, c_null_ptr, 0_c_int), 'amt_slab_create 1')
    rc = amt_slab_exchange(g1)
    call rec_int('slab_exchange_1', int(rc))
    call amt_check(amt_slab_sync(g1), 'amt_slab_sync')
    call rec_cstr('transport_slab_1', amt_slab_transport(g1))
    call amt_check(amt_slab_destroy(g1), 'amt_slab_destroy')
    do r = 0, 1
       call amt_check(amt_domain_destroy(dom(r)), 'amt_domain_destroy')
    end do
    ! what a host without the rendezvous file broadcasts itself, and the launch's nonce (host calls, recorded only)
    call amt_check(amt_comm_unique_id(uid), 'amt_comm_unique_id')
    write (ru, '(a,1x,i0)') 'launch_nonce', amt_comm_launch_nonce()
  end subroutine
  subroutine use_rank(r)
    integer, intent(in) :: r
    ims = rb(1, r); ime = rb(2, r); jms = rb(3, r); jme = rb(4, r); its = rb(5, r); ite = rb(6, r); jts = rb(7, r); jte = rb(8, r)
  end subroutine
  ! sub-step s of rank r: the exchanged fields from the generator with seed + s, NaN in the halos the neighbours deliver
  subroutine next_inputs(d, r, s, sd)
    type(c_ptr), intent(in) :: d
    integer, intent(in) :: r, s
    integer(c_int), intent(in) :: sd
    call use_rank(r)
    if (s > 0) call amt_check(amt_domain_fill_fields(d, AMT_EXCHANGED_FIELDS, seed + s, int(ims, c_long), int(kms-1, c_long), &
                   int(jms, c_long), int(gni+2, c_long), int(gnk+1, c_long), int(gnj+2, c_long)), 'amt_domain_fill_fields')
    call amt_check(amt_domain_poison_halos(d, sd), 'amt_domain_poison_halos')
  end subroutine
  subroutine sync_rank(hh, slab)
    type(c_ptr), intent(in) :: hh
    logical, intent(in) :: slab
    if (slab) then
       call amt_check(amt_slab_sync(hh), 'amt_slab_sync')
    else
       call amt_check(amt_grid_sync(hh), 'amt_grid_sync')
    end if
  end subroutine
  subroutine dump_rank(d, r, stage)
    type(c_ptr), intent(in) :: d
    integer, intent(in) :: r
    character(len=*), intent(in) :: stage
    character(len=2) :: tag
    call use_rank(r)
    call alloc_fields(1)
    write (tag, '(a,i1)') 'r', r
    call dom_dump_all(d, tag//stage, by_rows=.true.)
  end subroutine

  ! ------------------------------------------------------------------------------------------------------------------
  ! the one-shot host call with the residency cache in its checking mode and one device slot named explicitly
  ! ------------------------------------------------------------------------------------------------------------------
  subroutine run_oneshot()
    integer(c_int) :: slot(4), n, rc
    type(c_ptr) :: p(0:NF-1)
    integer :: fid, s
    call alloc_fields(1)
    call fill_fields_host(1, seed)
    do fid = 0, NF - 1
       p(fid) = c_loc(f(fid)%a)
    end do
    slot = 0
    call amt_check(amt_host_set_devices(1_c_int, slot), 'amt_host_set_devices')
    n = amt_host_devices(slot, 4_c_int)
    write (ru, '(a,2(1x,i0))') 'host_devices', n, slot(1)
    call amt_check(amt_host_cache_enable(1_c_int), 'amt_host_cache_enable')
    call amt_check(amt_host_cache_check(1_c_int), 'amt_host_cache_check')
    do s = 1, 2
       if (wb == 8) then
          rc = amt_advance_mu_t_f64(p(0), p(1), p(2), p(3), p(4), p(5), p(6), p(7), p(8), p(9), p(10), p(11), p(12), p(13),  &
               p(14), p(15), p(16), p(17), rdx, rdy, dts, epssm, p(18), p(19), p(20), p(21), p(22), p(23), p(24), p(25),     &
               px, sp, ne, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)
       else
          rc = amt_advance_mu_t_f32(p(0), p(1), p(2), p(3), p(4), p(5), p(6), p(7), p(8), p(9), p(10), p(11), p(12), p(13),  &
               p(14), p(15), p(16), p(17), real(rdx, c_float), real(rdy, c_float), real(dts, c_float), real(epssm, c_float), &
               p(18), p(19), p(20), p(21), p(22), p(23), p(24), p(25),                                                       &
               px, sp, ne, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte)
       end if
       call amt_check(rc, 'amt_advance_mu_t')
       ! "a new stage has rewritten the cached inputs": the next call uploads them again
       call amt_check(amt_host_invalidate(c_null_ptr), 'amt_host_invalidate')
    end do
    call amt_check(amt_host_cache_check(0_c_int), 'amt_host_cache_check')
    call amt_check(amt_host_cache_enable(0_c_int), 'amt_host_cache_enable')
    call amt_check(amt_host_set_devices(0_c_int, slot), 'amt_host_set_devices')
    call amt_check(amt_host_release(), 'amt_host_release')
    do fid = 0, NF - 1
       call write_bin('host2', fid, fsize(fid), f(fid)%a)
    end do
  end subroutine

  ! ------------------------------------------------------------------------------------------------------------------
  ! amt_halo_plan for every rank of PI x PJ (host arithmetic, no device): the count and each message's side, peer and bytes
  ! ------------------------------------------------------------------------------------------------------------------
  subroutine run_plan()
    type(amt_halo_message) :: out(4)
    integer(c_int) :: n, rc
    integer :: r, m
    gids = ids; gide = ide; gjds = jds; gjde = jde
    call rec_cstr('version', amt_version())
    call rec_cstr('status_string_2', amt_status_string(2_c_int))
    do r = 0, pi * pj - 1
       call patch_bounds(mod(r, pi), r / pi)
       n = -1
       rc = amt_halo_plan(wb, px, sp, ne, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte, &
                          int(mod(r, pi), c_int), int(r / pi, c_int), int(pi, c_int), int(pj, c_int), int(pflags, c_int),     &
                          out, 4_c_int, n)
       write (ru, '(a,3(1x,i0))') 'plan', r, rc, n
       if (rc /= AMT_OK) cycle
       do m = 1, n
          write (ru, '(a,7(1x,i0))') 'planned', r, out(m)%side, out(m)%peer, out(m)%send_bytes, out(m)%recv_bytes,           &
               out(m)%on_host, merge(1, 0, c_associated(out(m)%send) .or. c_associated(out(m)%recv))
       end do
    end do
  end subroutine

end program amt_binding_host
