// amt_uv.hip -- the momentum update that opens every acoustic sub-step, on the device (include/amt_advance_mu_t.h section 17,
// DESIGN.md section 7.12).  In WRF's solve_em advance_uv precedes every advance_mu_t: from the pressure p, the inverse density
// al and the geopotential ph that calc_p_rho has left, and from mu and mudf of the last sweep, it advances u and v by the
// horizontal pressure gradient and the divergence damping.  With clip = specified || nested:
//   columns, clip && !periodic_x:  i_start = max(its, ids+1), i_end = min(ite, ide-2), i_endu = min(ite, ide-1)
//   columns, otherwise:            i_start = its, i_endu = ite, i_end = min(ite, ide-1)
//   rows, clip:                    j_start = max(jts, jds+1), j_end = min(jte, jde-2), j_endv = min(jte, jde-1)
//   rows, otherwise:               j_start = jts, j_endv = jte, j_end = min(jte, jde-1)
// u part, j = j_start..j_end, i = i_start..i_endu, k = kts..kte-1, with x' the value at (i-1, j):
//   mr   = msfux / msfuy;   c = ((mr * T(0.5)) * rdx) * muu
//   g    = (((ph(k+1) - ph'(k+1)) + (ph(k) - ph'(k))) + ((alt + alt') * (p - p'))) + ((al + al') * (pb - pb'))
//   dpxy = c * g
//   non-hydrostatic:  s(k) = p + p';  dpn(kts) = T(0.5) * (((cf1*s(1)) + (cf2*s(2))) + (cf3*s(3)));
//                     dpn(k) = T(0.5) * ((fnm(k)*s(k)) + (fnp(k)*s(k-1))),  k = kts+1..kte-1;  dpn(kte) = T(0)
//                     dpxy = dpxy + (((mr * rdx) * (php - php')) * ((rdnw(k) * (dpn(k+1) - dpn(k))) - (T(0.5) * (mu' + mu))))
//   mdx  = (((-emdiv) * dx) * (mudf - mudf')) / msfuy
//   u    = ((u + (dts * ru_tend)) - ((dts * cqu) * dpxy)) + mdx
// v part, j = j_start..j_endv, i = i_start..i_end: the same text with x' the value at (i, j-1), mr = msfvy / msfvx, rdy, muv,
// cqv, rv_tend and mdy = (((-emdiv) * dy) * (mudf - mudf')) * msfvx_inv.
// Every operation rounded once in the arrays' type (the library is built with -ffp-contract=off), IEEE divides.
// One streaming pass in the family of amt_p_rho.hip: a work item owns one 16-byte chunk of a row and walks the levels of its
// group.  u and v are ONE launch of TWO parts selected by blockIdx.y, not one fused body: the two ranges differ in both
// directions (i_endu against i_end, j_end against j_endv), so a fused body would predicate every access of either part, and
// one text with the neighbour's distance as a parameter states the arithmetic once.  The u part takes its neighbour from the
// chunk itself, shifted by one element, and one more element in front of it; the v part loads the chunk of row j-1.
#include "amt_halo.h"
// the device text: the job, the accesses, the walk over k and the kernel.  A header of its own so that
// tests/uv_host_check.cpp can run the same text on the host.
#include "amt_uv_kernel.h"

namespace {
struct UvArrays {
    void *u, *v;
    const void *ru_tend, *rv_tend, *p, *pb, *ph, *php, *alt, *al, *mu, *muu, *muv, *mudf, *cqu, *cqv, *msfux, *msfuy, *msfvx, *msfvx_inv,
        *msfvy, *fnm, *fnp, *rdnw;
};
struct UvScalars { double rdx, rdy, dts, cf1, cf2, cf3, emdiv; int non_hydrostatic; };

// the cells are on the levels kts..kte-1: a tile needs two levels to hold one.  Whether a part holds a cell is this pass's own
// question (the u part reaches column ide, the v part row jde).
const AmtPassRules kUvRules = {2, false, "an output array overlaps another array of the call", "an output array overlaps another array of the call"};

// the ranges of the two parts, Fortran-inclusive and global: part 0 = u, part 1 = v
struct UvRanges { int i_lo[2], i_hi[2], j_lo[2], j_hi[2]; };
UvRanges uv_ranges(const amt_domain &s)
{
    const bool clip = s.specified || s.nested;
    const auto lo = [](int a, int b) { return a < b ? a : b; };
    const auto hi = [](int a, int b) { return a > b ? a : b; };
    int i_start, i_end, i_endu, j_start, j_end, j_endv;
    if (clip && !s.periodic_x) { i_start = hi(s.its, s.ids + 1); i_end = lo(s.ite, s.ide - 2); i_endu = lo(s.ite, s.ide - 1); }
    else { i_start = s.its; i_endu = s.ite; i_end = lo(s.ite, s.ide - 1); }
    if (clip) { j_start = hi(s.jts, s.jds + 1); j_end = lo(s.jte, s.jde - 2); j_endv = lo(s.jte, s.jde - 1); }
    else { j_start = s.jts; j_endv = s.jte; j_end = lo(s.jte, s.jde - 1); }
    return UvRanges{{i_start, i_start}, {i_endu, i_end}, {j_start, j_start}, {j_end, j_endv}};
}

// Argument and precondition checks (amt_pass.h): host arithmetic only.  *empty: neither part holds a cell (nothing to do).
int uv_check(const char *who, const amt_domain &s, int members, int non_hydrostatic, const UvArrays &a, bool *empty)
{
    const AmtPassArray arr[24] = {
        {a.u, 3, true, false}, {a.v, 3, true, false}, {a.ru_tend, 3, false, false}, {a.rv_tend, 3, false, false}, {a.p, 3, false, false},
        {a.pb, 3, false, false}, {a.ph, 3, false, false}, {a.php, 3, false, false}, {a.alt, 3, false, false}, {a.al, 3, false, false},
        {a.mu, 2, false, false}, {a.muu, 2, false, false}, {a.muv, 2, false, false}, {a.mudf, 2, false, false}, {a.cqu, 3, false, false},
        {a.cqv, 3, false, false}, {a.msfux, 2, false, false}, {a.msfuy, 2, false, false}, {a.msfvx, 2, false, false},
        {a.msfvx_inv, 2, false, false}, {a.msfvy, 2, false, false}, {a.fnm, 1, false, false}, {a.fnp, 1, false, false}, {a.rdnw, 1, false, false}};
    int rc = amt_pass_check_arrays(who, members, arr, 24);
    if (rc) return rc;
    rc = amt_pass_check_box(who, s, members, arr, 24, kUvRules, empty);
    if (rc || *empty) return rc;
    const UvRanges r = uv_ranges(s);
    const bool has_u = r.i_lo[0] <= r.i_hi[0] && r.j_lo[0] <= r.j_hi[0], has_v = r.i_lo[1] <= r.i_hi[1] && r.j_lo[1] <= r.j_hi[1];
    if (!has_u && !has_v) { *empty = true; return AMT_OK; }
    if (non_hydrostatic && s.kde < 4)
        return amt_fail(AMT_ERR_PRECONDITION, "%s: kde = %d: the non-hydrostatic form needs three levels of p (kde >= 4)", who, s.kde);
    // the cells read beside the tile: column i_start-1 (u part), row j_start-1 (v part); i_endu and j_endv lie in the tile
    const int i_first = has_u ? r.i_lo[0] - 1 : r.i_lo[1], j_first = has_v ? r.j_lo[1] - 1 : r.j_lo[0];
    // (named in the text; amt_pass_check_box has already held the tile, and with it i_endu and j_endv, inside memory)
    const int i_last = has_u ? r.i_hi[0] : r.i_hi[1], j_last = has_v ? r.j_hi[1] : r.j_hi[0];
    if (i_first < s.ims || j_first < s.jms)
        return amt_fail(AMT_ERR_PRECONDITION, "%s: the cells read, %d:%d, %d:%d, are not inside memory %d:%d, %d:%d", who, i_first, i_last,
                        j_first, j_last, s.ims, s.ime, s.jms, s.jme);
    return AMT_OK;
}

template <typename T>
int uv_launch(const amt_domain &d, int members, const UvArrays &a, const UvScalars &s)
{
    const auto in = [](const void *q) { return static_cast<const T *>(q); };
    AmtUvJob<T> job{};
    amt_pass_set_layout(d, job);
    const UvRanges r = uv_ranges(d);
    const T rdx = (T)s.rdx, rdy = (T)s.rdy, emdiv = (T)s.emdiv;
    const T dx = T(1) / rdx, dy = T(1) / rdy;
    AmtUvPart<T> &pu = job.part[0], &pv = job.part[1];
    pu.out = static_cast<T *>(a.u); pu.tend = in(a.ru_tend); pu.cq = in(a.cqu); pu.mass = in(a.muu);
    pu.msf_num = in(a.msfux); pu.msf_den = in(a.msfuy); pu.msf_md = in(a.msfuy);
    pu.rd = rdx; pu.md_scale = (-emdiv) * dx;
    pv.out = static_cast<T *>(a.v); pv.tend = in(a.rv_tend); pv.cq = in(a.cqv); pv.mass = in(a.muv);
    pv.msf_num = in(a.msfvy); pv.msf_den = in(a.msfvx); pv.msf_md = in(a.msfvx_inv);
    pv.rd = rdy; pv.md_scale = (-emdiv) * dy;
    long units = 0;
    constexpr long seg = 64 * 16 / (long)sizeof(T);                 // the elements of a wave's segment
    for (int k = 0; k < 2; ++k) {
        AmtUvPart<T> &pt = job.part[k];
        pt.i0 = r.i_lo[k] - d.its; pt.j0 = r.j_lo[k] - d.jts;
        pt.ni = r.i_hi[k] - r.i_lo[k] + 1; pt.nj = r.j_hi[k] - r.j_lo[k] + 1;
        if (pt.ni < 1 || pt.nj < 1) { pt.ni = 0; pt.nj = 0; continue; }
        const long n = (long)pt.nj * ((pt.ni + seg - 1) / seg);
        if (n > units) units = n;
    }
    job.p = in(a.p); job.pb = in(a.pb); job.ph = in(a.ph); job.php = in(a.php); job.alt = in(a.alt); job.al = in(a.al);
    job.mu = in(a.mu); job.mudf = in(a.mudf);
    job.fnm = in(a.fnm) + (d.kts - d.kms); job.fnp = in(a.fnp) + (d.kts - d.kms); job.rdnw = in(a.rdnw) + (d.kts - d.kms);
    job.nk = d.kte - d.kts;
    job.dts = (T)s.dts; job.cf1 = (T)s.cf1; job.cf2 = (T)s.cf2; job.cf3 = (T)s.cf3;
    long blocks = (units + 3) / 4;                                 // four waves to a block
    if (blocks > 1024) blocks = 1024;
    const unsigned groups = (unsigned)((job.nk + AMT_UV_GROUP - 1) / AMT_UV_GROUP);
    const dim3 grid((unsigned)blocks, 2 * groups, (unsigned)members);
    if (s.non_hydrostatic) hipLaunchKernelGGL((amt_uv_kernel<T, true>), grid, dim3(256), 0, d.stream, job);
    else hipLaunchKernelGGL((amt_uv_kernel<T, false>), grid, dim3(256), 0, d.stream, job);
    AMT_HIP(hipGetLastError());
    return AMT_OK;
}

// the checks, then the launch (amt_pass_run)
int uv_run(const char *who, const amt_domain &d, int members, const UvArrays &a, const UvScalars &s, bool pointer_level)
{
    bool empty = false;
    const int rc = uv_check(who, d, members, s.non_hydrostatic, a, &empty);
    return amt_pass_run(rc, empty, d, pointer_level, [&](auto t) { return uv_launch<decltype(t)>(d, members, a, s); });
}

// what a handle's call works on: ru_tend, rv_tend, pb, php, cqu, cqv, msfux, msfvx, msfvy are the setting's, p, al, ph, alt the
// pressure diagnosis's, the rest fields of the handle
UvArrays uv_of_domain(const amt_domain *d)
{
    void *const *x = d->uv_arr, *const *q = d->p_rho_arr, *const *f = d->field;
    return UvArrays{f[AMT_F_U], f[AMT_F_V], x[0], x[1], q[1], x[2], q[2], x[3], q[4], q[0], f[AMT_F_MU], f[AMT_F_MUU], f[AMT_F_MUV],
                    f[AMT_F_MUDF], x[4], x[5], x[6], f[AMT_F_MSFUY], x[7], f[AMT_F_MSFVX_INV], x[8], f[AMT_F_FNM], f[AMT_F_FNP], f[AMT_F_RDNW]};
}
UvScalars uv_scalars_of_domain(const amt_domain *d)
{
    return UvScalars{d->rdx, d->rdy, d->dts, d->uv_cf1, d->uv_cf2, d->uv_cf3, d->uv_emdiv, d->p_rho_mode == 1};
}

AmtPassSetting uv_setting(amt_domain *d, int members)
{
    const size_t b3 = d->count(AMT_F_T) * (size_t)members * (size_t)d->dtype_bytes, b2 = d->count(AMT_F_MU) * (size_t)members * (size_t)d->dtype_bytes;
    return AmtPassSetting{d->uv_arr, &d->uv_owned, 9, {b3, b3, b3, b3, b3, b3, b2, b2, b2}, "nine arrays", "an array",
                          "the momentum update", "an array"};
}

// The wrap refresh in front of an update on a cyclic handle, with the mover of amt_halo.h: of p, al, ph, alt, pb, php, mu, mudf
// column ide <- ids and ids-1 <- ide-1 over the rows of the u part, row jde <- jds and jds-1 <- jde-1 over the columns of the v
// part, every memory level, elements moved as bits.  The pass reads no corner cell, so no copy reads what another writes.
int uv_wrap_refresh(const amt_domain &d, int members, const UvArrays &a)
{
    const UvRanges r = uv_ranges(d);
    const long idim = d.ime - d.ims + 1, kdim = d.kme - d.kms + 1, jdim = d.jme - d.jms + 1;
    const size_t es = (size_t)d.dtype_bytes;
    const struct { const void *p; int rank; } wrapped[8] = {{a.p, 3}, {a.al, 3}, {a.ph, 3}, {a.alt, 3}, {a.pb, 3}, {a.php, 3}, {a.mu, 2}, {a.mudf, 2}};
    AmtHaloJob jobs[AMT_HALO_MAX_JOBS];
    int n = 0;
    const auto flush = [&]() { const int rc = n ? amt_halo_launch(d.stream, d.dtype_bytes, members, jobs, n) : AMT_OK; n = 0; return rc; };
    for (int side : {AMT_HALO_RIGHT, AMT_HALO_LEFT, AMT_HALO_ABOVE, AMT_HALO_BELOW}) {
        const bool column = amt_halo_is_column(side);
        if (!(d.cyclic & (column ? AMT_CYCLIC_X : AMT_CYCLIC_Y))) continue;
        const bool high = side == AMT_HALO_RIGHT || side == AMT_HALO_ABOVE;
        const int j0 = r.j_lo[0], nrows = r.j_hi[0] - r.j_lo[0] + 1, i0 = r.i_lo[1], ncols = r.i_hi[1] - r.i_lo[1] + 1;
        if ((column ? nrows : ncols) < 1) continue;
        const int si = column ? (high ? d.ids : d.ide - 1) : i0, di = column ? (high ? d.ide : d.ids - 1) : i0;
        const int sj = column ? j0 : (high ? d.jds : d.jde - 1), dj = column ? j0 : (high ? d.jde : d.jds - 1);
        for (const auto &w : wrapped) {
            const long levels = w.rank == 3 ? kdim : 1;
            const auto at = [&](int i, int j) { return (size_t)((long)(j - d.jms) * levels * idim + (i - d.ims)) * es; };
            char *base = static_cast<char *>(const_cast<void *>(w.p));
            jobs[n++] = AmtHaloJob{base + at(si, sj), base + at(di, dj), column ? (long)nrows * levels : levels, column ? 1 : ncols, idim, idim,
                                   idim * levels * jdim};
            if (n == AMT_HALO_MAX_JOBS) { const int rc = flush(); if (rc) return rc; }
        }
    }
    return flush();
}
}  // namespace

// ---- what the handles call (amt_handle_*uv of amt_domain.hip) ---------------------------------------------------------------
int amt_uv_domain(const char *who, amt_domain *d, int members)
{
    if (!d->uv_on) return amt_fail(AMT_ERR_PRECONDITION, "%s: the momentum update is off (amt_*_set_uv)", who);
    if (!d->p_rho_mode)
        return amt_fail(AMT_ERR_PRECONDITION, "%s: the pressure diagnosis, whose al, p, ph, alt the update reads, is off (amt_*_set_p_rho)", who);
    const UvArrays a = uv_of_domain(d);
    const UvScalars s = uv_scalars_of_domain(d);
    bool empty = false;
    int rc = uv_check(who, *d, members, s.non_hydrostatic, a, &empty);
    if (rc != AMT_OK || empty) return rc;
    if (d->cyclic) {
        DeviceScope scope(d->device);
        if ((rc = uv_wrap_refresh(*d, members, a)) != AMT_OK) return rc;
    }
    return uv_run(who, *d, members, a, s, false);
}

void amt_uv_release(amt_domain *d)
{
    amt_pass_setting_release(uv_setting(d, 1));
    d->uv_on = 0;
    d->uv_per_sweep = 0;
}

// amt_*_set_uv.  A refusal changes nothing.
int amt_uv_set_domain(const char *who, amt_domain *d, int members, int on, int per_sweep, double emdiv, double cf1, double cf2, double cf3,
                      void *const arr[9])
{
    if (!on) {
        DeviceScope scope(d->device);
        amt_uv_release(d);
        return AMT_OK;
    }
    const AmtPassSetting s = uv_setting(d, members);
    int given;
    bool same;                                                     // the library's own arrays handed back (amt_*_uv_ptr): they stay
    int rc = amt_pass_setting_offer(who, s, arr, &given, &same);
    if (rc) return rc;
    if (!d->p_rho_mode)
        return amt_fail(AMT_ERR_PRECONDITION, "%s: the pressure diagnosis, whose al, p, ph, alt the update reads, is off (amt_*_set_p_rho)", who);
    rc = amt_pass_setting_take(who, d, members, s, arr, given, same, [&](void *const *theirs) {
        amt_domain probe = *d;
        memcpy(probe.uv_arr, theirs, sizeof probe.uv_arr);
        bool empty = false;
        return uv_check(who, probe, members, d->p_rho_mode == 1, uv_of_domain(&probe), &empty);
    });
    if (rc) return rc;
    d->uv_on = 1;                                                  // also for the library's own arrays: the scalars are set anew
    d->uv_per_sweep = per_sweep != 0;
    d->uv_emdiv = emdiv; d->uv_cf1 = cf1; d->uv_cf2 = cf2; d->uv_cf3 = cf3;
    return AMT_OK;
}

// ---- pointer level -------------------------------------------------------------------------------------------------------
#define AMT_UV_SIG(T)                                                                                            \
    void *hip_stream, int members, int non_hydrostatic, T *u, T *v, const T *ru_tend, const T *rv_tend, const T *p, \
    const T *pb, const T *ph, const T *php, const T *alt, const T *al, const T *mu, const T *muu, const T *muv,  \
    const T *mudf, const T *cqu, const T *cqv, const T *msfux, const T *msfuy, const T *msfvx,                   \
    const T *msfvx_inv, const T *msfvy, const T *fnm, const T *fnp, const T *rdnw, T rdx, T rdy, T dts, T cf1,   \
    T cf2, T cf3, T emdiv, int periodic_x, int specified, int nested, AMT_BOUNDS_SIG
#define AMT_UV_BODY(T, name)                                                                                     \
    amt_domain d = amt_pass_domain((int)sizeof(T), hip_stream, AMT_BOUNDS_ARGS);                                 \
    d.periodic_x = periodic_x != 0; d.specified = specified != 0; d.nested = nested != 0;                        \
    return uv_run(name, d, members,                                                                              \
                  UvArrays{u, v, ru_tend, rv_tend, p, pb, ph, php, alt, al, mu, muu, muv, mudf, cqu, cqv, msfux, msfuy, msfvx, \
                           msfvx_inv, msfvy, fnm, fnp, rdnw},                                                    \
                  UvScalars{(double)rdx, (double)rdy, (double)dts, (double)cf1, (double)cf2, (double)cf3, (double)emdiv, \
                            non_hydrostatic != 0}, true);

extern "C" int amt_advance_uv_device_f32(AMT_UV_SIG(float)) { AMT_UV_BODY(float, "amt_advance_uv_device_f32") }
extern "C" int amt_advance_uv_device_f64(AMT_UV_SIG(double)) { AMT_UV_BODY(double, "amt_advance_uv_device_f64") }
