// amt_p_rho.hip -- the pressure diagnosis that closes every acoustic sub-step, on the device (include/amt_advance_mu_t.h
// section 16).  In WRF's solve_em calc_p_rho follows every advance_mu_t (and small_step_prep, with
// step = 0): from t = t_2, t_old = t_1, mu = mu_2 and muts it diagnoses the inverse density al and the pressure p, and in its
// hydrostatic branch integrates the geopotential ph up the column.  For every cell of the columns its..min(ite, ide-1),
// jts..min(jte, jde-1), k = kts..kte-1:
//   q = (alt * (t - (mu * t_old))) / (muts * (t0 + t_old))
//   mode 1:  al = (T(-1) / muts) * ((alt * mu) + (rdnw(k) * (ph(k+1) - ph(k))));   p = c2a * (q - al)
//   mode 2:  p = mu * znu(k);   al = q - (p / c2a);   ph(k+1) = ph(k) - (dnw(k) * ((muts * al) + (mu * alt)))     k ascending
//   both:    x = p;  step == 0:  p = x, pm1 = x;   step != 0:  p = x + (smdiv * (x - pm1)), pm1 = x
// every operation rounded once in the arrays' type (the library is built with -ffp-contract=off), IEEE divides.
// One streaming pass in the family of amt_stage.hip and amt_sumflux.hip; unlike them a work item WALKS k: it owns one 16-byte
// chunk of a row (element by element where the addresses do not allow that) and carries it through the levels of its group.  In mode 2 the group is the whole column: the running ph stays
// in registers and the serial chain costs one subtraction per level, every load and every other operation of a level is
// independent of it.  In mode 1 the column is cut into groups of AMT_P_RHO_GROUP levels, one per blockIdx.y, and ph(k+1)
// becomes the next level's ph(k) in registers: ph is read once per group plus one level.  The level index is uniform in a
// workgroup, so rdnw, znu and dnw come through scalar loads.
#include "amt_internal.h"
// the device text: the job, the 16-byte accesses, the walk over k and the kernel.  A header of its own so that
// tests/p_rho_host_check.cpp can run the same text on the host.
#include "amt_p_rho_kernel.h"

namespace {
struct PRhoArrays {
    void *al, *p, *ph, *pm1;
    const void *alt, *c2a, *t, *t_old, *mu, *muts, *rdnw, *znu, *dnw;
};

// Argument and precondition checks: host arithmetic only.  *empty: the range holds no cell (nothing to do).
int p_rho_check(const char *who, const amt_domain &s, int members, int mode, int step, const PRhoArrays &a, bool *empty)
{
    *empty = false;
    // rank 3, 2 or 1; an output may overlap nothing, inputs may alias one another.  ph is written in mode 2 only.
    const struct { const void *p; int rank; bool output; } arr[13] = {
        {a.al, 3, true}, {a.p, 3, true}, {a.ph, 3, mode == 2}, {a.pm1, 3, true}, {a.alt, 3, false}, {a.c2a, 3, false},
        {a.t, 3, false}, {a.t_old, 3, false}, {a.mu, 2, false}, {a.muts, 2, false}, {a.rdnw, 1, false}, {a.znu, 1, false},
        {a.dnw, 1, false}};
    for (const auto &x : arr)
        if (!x.p) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null array pointer", who);
    if (members < 1) return amt_fail(AMT_ERR_INVALID_ARG, "%s: members = %d: an ensemble has at least one member", who, members);
    if (mode != 1 && mode != 2) return amt_fail(AMT_ERR_INVALID_ARG, "%s: mode = %d: 1 (non-hydrostatic) or 2 (hydrostatic)", who, mode);
    if (step < 0) return amt_fail(AMT_ERR_INVALID_ARG, "%s: step = %d: at least 0", who, step);
    if (s.ime < s.ims || s.jme < s.jms || s.kme < s.kms) return amt_fail(AMT_ERR_PRECONDITION, "%s: empty memory extents", who);
    const size_t idim = s.ime - s.ims + 1, kdim = s.kme - s.kms + 1, jdim = s.jme - s.jms + 1, wb = (size_t)s.dtype_bytes;
    const size_t bytes[4] = {0, kdim * wb, idim * jdim * (size_t)members * wb, idim * kdim * jdim * (size_t)members * wb};
    for (int k = 0; k < 13; ++k) {
        const uintptr_t p0 = reinterpret_cast<uintptr_t>(arr[k].p), pb = bytes[arr[k].rank];
        for (int m = k + 1; m < 13; ++m) {
            if (!(arr[k].output || arr[m].output)) continue;
            const uintptr_t r0 = reinterpret_cast<uintptr_t>(arr[m].p), rb = bytes[arr[m].rank];
            if (p0 < r0 + rb && r0 < p0 + pb) return amt_fail(AMT_ERR_INVALID_ARG, "%s: an output array overlaps another array of the call", who);
        }
    }
    if (s.kts != 1) return amt_fail(AMT_ERR_PRECONDITION, "%s: kts = %d, the library needs kts == 1", who, s.kts);
    if (s.kte != s.kde) return amt_fail(AMT_ERR_PRECONDITION, "%s: kte = %d is not kde = %d", who, s.kte, s.kde);
    if (s.kme < s.kte || s.kms > s.kts) return amt_fail(AMT_ERR_PRECONDITION, "%s: levels kts:kte = %d:%d are not inside memory kms:kme = %d:%d", who, s.kts, s.kte, s.kms, s.kme);
    if (s.ite < s.its || s.jte < s.jts || s.kte <= s.kts) { *empty = true; return AMT_OK; }
    if (s.its < s.ims || s.ite > s.ime || s.jts < s.jms || s.jte > s.jme)
        return amt_fail(AMT_ERR_PRECONDITION, "%s: the tile %d:%d, %d:%d is not inside memory %d:%d, %d:%d", who,
                        s.its, s.ite, s.jts, s.jte, s.ims, s.ime, s.jms, s.jme);
    if (members > 65535) return amt_fail(AMT_ERR_PRECONDITION, "%s: %d members: one launch covers at most 65535", who, members);
    const int ihi = s.ite < s.ide - 1 ? s.ite : s.ide - 1, jhi = s.jte < s.jde - 1 ? s.jte : s.jde - 1;
    if (ihi < s.its || jhi < s.jts) *empty = true;
    return AMT_OK;
}

template <typename T>
int p_rho_launch(const amt_domain &d, int members, int mode, int step, const PRhoArrays &a, double t0, double smdiv)
{
    const long idim = d.ime - d.ims + 1, kdim = d.kme - d.kms + 1, jdim = d.jme - d.jms + 1;
    AmtPRhoJob<T> job{};
    job.al = static_cast<T *>(a.al); job.p = static_cast<T *>(a.p); job.ph = static_cast<T *>(a.ph); job.pm1 = static_cast<T *>(a.pm1);
    job.alt = static_cast<const T *>(a.alt); job.c2a = static_cast<const T *>(a.c2a);
    job.t = static_cast<const T *>(a.t); job.t_old = static_cast<const T *>(a.t_old);
    job.mu = static_cast<const T *>(a.mu); job.muts = static_cast<const T *>(a.muts);
    job.rdnw = static_cast<const T *>(a.rdnw) + (d.kts - d.kms);
    job.znu = static_cast<const T *>(a.znu) + (d.kts - d.kms);
    job.dnw = static_cast<const T *>(a.dnw) + (d.kts - d.kms);
    job.ni = (d.ite < d.ide - 1 ? d.ite : d.ide - 1) - d.its + 1;
    job.nk = d.kte - d.kts;
    job.nj = (d.jte < d.jde - 1 ? d.jte : d.jde - 1) - d.jts + 1;
    job.idim = idim; job.jstride3 = kdim * idim; job.mstride3 = idim * kdim * jdim; job.mstride2 = idim * jdim;
    job.first3 = ((long)(d.jts - d.jms) * kdim + (d.kts - d.kms)) * idim + (d.its - d.ims);
    job.first2 = (long)(d.jts - d.jms) * idim + (d.its - d.ims);
    job.t0 = (T)t0; job.smdiv = (T)smdiv;
    job.step0 = step == 0;
    constexpr long seg = 64 * 16 / (long)sizeof(T);                 // the elements of a wave's segment
    const long units = (long)job.nj * ((job.ni + seg - 1) / seg);
    long blocks = (units + 3) / 4;                                 // four waves to a block
    if (blocks > 1024) blocks = 1024;
    if (mode == 1) {
        const unsigned groups = (unsigned)((job.nk + AMT_P_RHO_GROUP - 1) / AMT_P_RHO_GROUP);
        hipLaunchKernelGGL((amt_p_rho_kernel<T, 1>), dim3((unsigned)blocks, groups, (unsigned)members), dim3(256), 0, d.stream, job);
    } else {
        hipLaunchKernelGGL((amt_p_rho_kernel<T, 2>), dim3((unsigned)blocks, 1, (unsigned)members), dim3(256), 0, d.stream, job);
    }
    AMT_HIP(hipGetLastError());
    return AMT_OK;
}

// with_device_check: the pointer-level calls, which may be the first HIP call of a process, report a missing device
// themselves -- behind the argument errors, which need none -- and run on the caller's current device
int p_rho_run(const char *who, const amt_domain &d, int members, int mode, int step, const PRhoArrays &a, double t0, double smdiv,
              bool with_device_check)
{
    bool empty = false;
    const int rc = p_rho_check(who, d, members, mode, step, a, &empty);
    if (rc != AMT_OK || empty) return rc;
    int dev = d.device;
    if (with_device_check) {
        int ndev = 0;
        AMT_HIP(hipGetDeviceCount(&ndev));
        if (ndev < 1) return amt_fail(AMT_ERR_NO_DEVICE, "no HIP device visible");
        (void)hipGetDevice(&dev);
    }
    DeviceScope scope(dev);
    return d.dtype_bytes == 8 ? p_rho_launch<double>(d, members, mode, step, a, t0, smdiv)
                              : p_rho_launch<float>(d, members, mode, step, a, t0, smdiv);
}

// what a handle's call works on: al, p, ph, pm1, alt, c2a, znu, dnw are the setting's, t_old the stage bracket's
PRhoArrays p_rho_of_domain(const amt_domain *d)
{
    void *const *x = d->p_rho_arr;
    return PRhoArrays{x[0], x[1], x[2], x[3], x[4], x[5], d->field[AMT_F_T], d->stage_arr[0], d->field[AMT_F_MU], d->field[AMT_F_MUTS],
                      d->field[AMT_F_RDNW], x[6], x[7]};
}
}  // namespace

// ---- what the handles call (amt_handle_*p_rho of amt_domain.hip) ----------------------------------------------------------
int amt_p_rho_domain(const char *who, amt_domain *d, int members, int step)
{
    if (!d->p_rho_mode) return amt_fail(AMT_ERR_PRECONDITION, "%s: the pressure diagnosis is off (amt_*_set_p_rho)", who);
    if (!d->stage_on) return amt_fail(AMT_ERR_PRECONDITION, "%s: the stage bracket, whose t_old the diagnosis reads, is off (amt_*_set_stage)", who);
    return p_rho_run(who, *d, members, d->p_rho_mode, step, p_rho_of_domain(d), d->p_rho_t0, d->p_rho_smdiv, false);
}

void amt_p_rho_release(amt_domain *d)
{
    for (void *&q : d->p_rho_arr) {
        if (q && d->p_rho_owned) (void)hipFree(q);
        q = nullptr;
    }
    d->p_rho_mode = 0;
    d->p_rho_per_sweep = 0;
    d->p_rho_owned = false;
}

// amt_*_set_p_rho.  A refusal changes nothing.
int amt_p_rho_set_domain(const char *who, amt_domain *d, int members, int mode, int per_sweep, double t0, double smdiv, void *const given_arr[8])
{
    if (mode == 0) {
        DeviceScope scope(d->device);
        amt_p_rho_release(d);
        return AMT_OK;
    }
    if (mode != 1 && mode != 2) return amt_fail(AMT_ERR_INVALID_ARG, "%s: mode = %d: 0 (off), 1 (non-hydrostatic) or 2 (hydrostatic)", who, mode);
    void *arr[8];
    int given = 0;
    for (int k = 0; k < 8; ++k) given += (arr[k] = given_arr[k]) != nullptr;
    if (given != 0 && given != 8)
        return amt_fail(AMT_ERR_INVALID_ARG, "%s: give all eight arrays or none (the library then allocates them)", who);
    if (!d->stage_on) return amt_fail(AMT_ERR_PRECONDITION, "%s: the stage bracket, whose t_old the diagnosis reads, is off (amt_*_set_stage)", who);
    // the library's own arrays handed back (amt_*_p_rho_ptr): they stay the library's, the mode and the scalars are set anew;
    // some of them among the caller's would be freed under the caller
    const bool same = given == 8 && d->p_rho_owned && memcmp(arr, d->p_rho_arr, sizeof arr) == 0;
    if (given == 8 && d->p_rho_owned && !same)
        for (void *mine : d->p_rho_arr)
            for (void *theirs : arr)
                if (mine == theirs) return amt_fail(AMT_ERR_INVALID_ARG, "%s: an array the library allocated, mixed with others", who);
    if (given == 8) {
        amt_domain probe = *d;                                     // the checks against the caller's arrays, nothing enqueued
        memcpy(probe.p_rho_arr, arr, sizeof arr);
        bool empty = false;
        const int rc = p_rho_check(who, probe, members, mode, 0, p_rho_of_domain(&probe), &empty);
        if (rc) return rc;
    } else {
        if (members > 65535) return amt_fail(AMT_ERR_PRECONDITION, "%s: %d members: one launch covers at most 65535", who, members);
        if (d->kts != 1 || d->kte != d->kde || d->kme < d->kte || d->kms > d->kts || d->its < d->ims || d->ite > d->ime || d->jts < d->jms || d->jte > d->jme)
            return amt_fail(AMT_ERR_PRECONDITION, "%s: the handle's tile does not admit the pressure diagnosis (kts == 1, kte == kde, tile inside memory)", who);
    }
    DeviceScope scope(d->device);                                  // behind every refusal but a failed allocation
    if (given == 0) {
        for (int k = 0; k < 8; ++k) {
            const size_t bytes = (k < 6 ? d->count(AMT_F_T) * (size_t)members : d->count(AMT_F_DNW)) * (size_t)d->dtype_bytes;
            arr[k] = nullptr;
            if (hipMalloc(&arr[k], bytes) != hipSuccess) {
                (void)hipGetLastError();
                for (int m = 0; m < k; ++m) (void)hipFree(arr[m]);
                return amt_fail(AMT_ERR_ALLOC, "%s: no room for an array of %zu bytes", who, bytes);
            }
        }
    }
    if (!same) {
        amt_p_rho_release(d);
        memcpy(d->p_rho_arr, arr, sizeof arr);
        d->p_rho_owned = given == 0;
    }
    d->p_rho_mode = mode;
    d->p_rho_per_sweep = per_sweep != 0;
    d->p_rho_t0 = t0;
    d->p_rho_smdiv = smdiv;
    return AMT_OK;
}

// ---- pointer level -------------------------------------------------------------------------------------------------------
#define AMT_P_RHO_SIG(T)                                                                                        \
    void *hip_stream, int members, int mode, int step, T *al, T *p, T *ph, T *pm1, const T *alt, const T *c2a,  \
    const T *t, const T *t_old, const T *mu, const T *muts, const T *rdnw, const T *znu, const T *dnw,          \
    T t0, T smdiv,                                                                                              \
    int ids, int ide, int jds, int jde, int kde, int ims, int ime, int jms, int jme, int kms, int kme,          \
    int its, int ite, int jts, int jte, int kts, int kte
#define AMT_P_RHO_BODY(T, name)                                                                                 \
    amt_domain d{(int)sizeof(T), 0, 0, 0, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte}; \
    d.stream = static_cast<hipStream_t>(hip_stream);                                                            \
    return p_rho_run(name, d, members, mode, step, PRhoArrays{al, p, ph, pm1, alt, c2a, t, t_old, mu, muts, rdnw, znu, dnw}, \
                     (double)t0, (double)smdiv, true);

extern "C" int amt_p_rho_device_f32(AMT_P_RHO_SIG(float)) { AMT_P_RHO_BODY(float, "amt_p_rho_device_f32") }
extern "C" int amt_p_rho_device_f64(AMT_P_RHO_SIG(double)) { AMT_P_RHO_BODY(double, "amt_p_rho_device_f64") }
