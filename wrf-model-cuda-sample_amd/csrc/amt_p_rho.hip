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

// the cells are on the levels kts..kte-1: a tile needs two levels to hold one, and a mass column
const AmtPassRules kPRhoRules = {2, true, "an output array overlaps another array of the call", "an output array overlaps another array of the call"};

// Argument and precondition checks (amt_pass.h): host arithmetic only.  *empty: the range holds no cell (nothing to do).
int p_rho_check(const char *who, const amt_domain &s, int members, int mode, int step, const PRhoArrays &a, bool *empty)
{
    // ph is written in mode 2 only; rdnw, znu and dnw are shared by the members
    const AmtPassArray arr[13] = {{a.al, 3, true, false}, {a.p, 3, true, false}, {a.ph, 3, mode == 2, false}, {a.pm1, 3, true, false},
                                  {a.alt, 3, false, false}, {a.c2a, 3, false, false}, {a.t, 3, false, false}, {a.t_old, 3, false, false},
                                  {a.mu, 2, false, false}, {a.muts, 2, false, false}, {a.rdnw, 1, false, false}, {a.znu, 1, false, false},
                                  {a.dnw, 1, false, false}};
    const int rc = amt_pass_check_arrays(who, members, arr, 13);
    if (rc) return rc;
    if (mode != 1 && mode != 2) return amt_fail(AMT_ERR_INVALID_ARG, "%s: mode = %d: 1 (non-hydrostatic) or 2 (hydrostatic)", who, mode);
    if (step < 0) return amt_fail(AMT_ERR_INVALID_ARG, "%s: step = %d: at least 0", who, step);
    return amt_pass_check_box(who, s, members, arr, 13, kPRhoRules, empty);
}

template <typename T>
int p_rho_launch(const amt_domain &d, int members, int mode, int step, const PRhoArrays &a, double t0, double smdiv)
{
    AmtPRhoJob<T> job{};
    job.al = static_cast<T *>(a.al); job.p = static_cast<T *>(a.p); job.ph = static_cast<T *>(a.ph); job.pm1 = static_cast<T *>(a.pm1);
    job.alt = static_cast<const T *>(a.alt); job.c2a = static_cast<const T *>(a.c2a);
    job.t = static_cast<const T *>(a.t); job.t_old = static_cast<const T *>(a.t_old);
    job.mu = static_cast<const T *>(a.mu); job.muts = static_cast<const T *>(a.muts);
    job.rdnw = static_cast<const T *>(a.rdnw) + (d.kts - d.kms);
    job.znu = static_cast<const T *>(a.znu) + (d.kts - d.kms);
    job.dnw = static_cast<const T *>(a.dnw) + (d.kts - d.kms);
    amt_pass_mass_lengths(d, &job.ni, &job.nj);
    job.nk = d.kte - d.kts;
    amt_pass_set_layout(d, job);
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

// the checks, then the launch (amt_pass_run)
int p_rho_run(const char *who, const amt_domain &d, int members, int mode, int step, const PRhoArrays &a, double t0, double smdiv,
              bool pointer_level)
{
    bool empty = false;
    const int rc = p_rho_check(who, d, members, mode, step, a, &empty);
    return amt_pass_run(rc, empty, d, pointer_level, [&](auto t) { return p_rho_launch<decltype(t)>(d, members, mode, step, a, t0, smdiv); });
}

// what a handle's call works on: al, p, ph, pm1, alt, c2a, znu, dnw are the setting's, t_old the stage bracket's
PRhoArrays p_rho_of_domain(const amt_domain *d)
{
    void *const *x = d->p_rho_arr;
    return PRhoArrays{x[0], x[1], x[2], x[3], x[4], x[5], d->field[AMT_F_T], d->stage_arr[0], d->field[AMT_F_MU], d->field[AMT_F_MUTS],
                      d->field[AMT_F_RDNW], x[6], x[7]};
}

// the eight arrays in the handle: al, p, ph, pm1, alt, c2a one 3-D field's extents times the members, znu and dnw one column
AmtPassSetting p_rho_setting(amt_domain *d, int members)
{
    const size_t b3 = d->count(AMT_F_T) * (size_t)members * (size_t)d->dtype_bytes, b1 = d->count(AMT_F_DNW) * (size_t)d->dtype_bytes;
    return AmtPassSetting{d->p_rho_arr, &d->p_rho_owned, 8, {b3, b3, b3, b3, b3, b3, b1, b1}, "eight arrays", "an array",
                          "the pressure diagnosis", "an array"};
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
    amt_pass_setting_release(p_rho_setting(d, 1));
    d->p_rho_mode = 0;
    d->p_rho_per_sweep = 0;
}

// amt_*_set_p_rho.  A refusal changes nothing.
int amt_p_rho_set_domain(const char *who, amt_domain *d, int members, int mode, int per_sweep, double t0, double smdiv, void *const arr[8])
{
    if (mode == 0) {
        DeviceScope scope(d->device);
        amt_p_rho_release(d);
        return AMT_OK;
    }
    if (mode != 1 && mode != 2) return amt_fail(AMT_ERR_INVALID_ARG, "%s: mode = %d: 0 (off), 1 (non-hydrostatic) or 2 (hydrostatic)", who, mode);
    const AmtPassSetting s = p_rho_setting(d, members);
    int given;
    bool same;                                                     // the library's own arrays handed back (amt_*_p_rho_ptr): they stay
    int rc = amt_pass_setting_offer(who, s, arr, &given, &same);
    if (rc) return rc;
    if (!d->stage_on) return amt_fail(AMT_ERR_PRECONDITION, "%s: the stage bracket, whose t_old the diagnosis reads, is off (amt_*_set_stage)", who);
    rc = amt_pass_setting_take(who, d, members, s, arr, given, same, [&](void *const *theirs) {
        amt_domain probe = *d;
        memcpy(probe.p_rho_arr, theirs, sizeof probe.p_rho_arr);
        bool empty = false;
        return p_rho_check(who, probe, members, mode, 0, p_rho_of_domain(&probe), &empty);
    });
    if (rc) return rc;
    d->p_rho_mode = mode;                                          // also for the library's own arrays: the mode and the scalars are set anew
    d->p_rho_per_sweep = per_sweep != 0;
    d->p_rho_t0 = t0;
    d->p_rho_smdiv = smdiv;
    return AMT_OK;
}

// ---- pointer level -------------------------------------------------------------------------------------------------------
#define AMT_P_RHO_SIG(T)                                                                                        \
    void *hip_stream, int members, int mode, int step, T *al, T *p, T *ph, T *pm1, const T *alt, const T *c2a,  \
    const T *t, const T *t_old, const T *mu, const T *muts, const T *rdnw, const T *znu, const T *dnw,          \
    T t0, T smdiv, AMT_BOUNDS_SIG
#define AMT_P_RHO_BODY(T, name)                                                                                 \
    return p_rho_run(name, amt_pass_domain((int)sizeof(T), hip_stream, AMT_BOUNDS_ARGS), members, mode, step,   \
                     PRhoArrays{al, p, ph, pm1, alt, c2a, t, t_old, mu, muts, rdnw, znu, dnw}, (double)t0, (double)smdiv, true);

extern "C" int amt_p_rho_device_f32(AMT_P_RHO_SIG(float)) { AMT_P_RHO_BODY(float, "amt_p_rho_device_f32") }
extern "C" int amt_p_rho_device_f64(AMT_P_RHO_SIG(double)) { AMT_P_RHO_BODY(double, "amt_p_rho_device_f64") }
