// amt_internal.h -- what the translation units of the host-side runtime share (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <new>

#include "../../include/amt_advance_mu_t.h"
#include "../../include/amt_synth.h"
#include "amt_params.h"

// ---------------------------------------------------------------------------
// errors: the text goes to the calling thread's amt_last_error(), the status is returned
// ---------------------------------------------------------------------------
int amt_fail(int status, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define AMT_HIP(call)                                                                   \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess)                                                           \
            return amt_fail(e_ == hipErrorNoDevice ? AMT_ERR_NO_DEVICE : AMT_ERR_HIP,   \
                            "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),      \
                            __FILE__, __LINE__);                                        \
    } while (0)

// ---------------------------------------------------------------------------
// Fault injection for the halo-freshness tests (tests/test_gpu_34_halo_freshness.py): AMT_TEST_FAULT="<step>@<n>" turns the
// n-th occurrence (1-based, per exchange / per stepper) of one step of the halo exchange into a no-op, everything around it
// -- sequence numbers, posts, waits -- running as usual, so that the sweep completes with STALE halo data instead of
// hanging.  Steps: skip_stage (IPC: the staging copies of the send segments are not refreshed), skip_pull (IPC: the rows
// are not pulled), skip_group (RCCL: the ncclSend/ncclRecv group is not issued -- every rank must carry the same setting),
// skip_pack / skip_unpack (grid stepper: the halo columns are not gathered / scattered).  A test that cannot tell such a
// run from a healthy one does not test the exchange beyond its first sweep.  Unset (always, outside those tests): no effect.
// ---------------------------------------------------------------------------
inline bool amt_test_fault(const char *step, unsigned long long occurrence)
{
    const char *spec = getenv("AMT_TEST_FAULT");          // read per call (a few times per sweep): a test sets and clears it in-process
    if (!spec || !*spec) return false;
    const char *at = strchr(spec, '@');
    if (!at || (size_t)(at - spec) != strlen(step) || strncmp(spec, step, at - spec) != 0) return false;
    return strtoull(at + 1, nullptr, 10) == occurrence;
}

// ---------------------------------------------------------------------------
// argument bundle shared by the entry points
// ---------------------------------------------------------------------------
template <typename T>
struct AmtArgs {
    T *ww; const T *ww_1, *u, *u_1, *v, *v_1;
    T *mu; const T *mut; T *muave, *muts; const T *muu, *muv;
    T *mudf, *t; const T *t_1; T *t_ave; const T *ft, *mu_tend;
    T rdx, rdy, dts, epssm;
    const T *dnw, *fnm, *fnp, *rdnw, *msfuy, *msfvx_inv, *msftx, *msfty;
    int periodic_x, specified, nested;
    int ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte;
};


// ---------------------------------------------------------------------------
// The field table: one row per AMT_F_* in the order of the enum (include/amt_synth.h) -- id, the AmtArgs member that carries
// it (its name is the field's name), whether advance_mu_t reads it (`in`) and whether it assigns it (`out`).  t_ave
// (module_small_step_em.f90:210) and muave, muts, mudf (:152-156) are assigned before any use; of ww only level 1 is read
// (:161).  A field's rank is amt_field_rank(); the fields that need a halo row or column are the lists of amt_halo.h.
// ---------------------------------------------------------------------------
#define AMT_FIELDS(X)                                                                                              \
    X(WW, ww, 1, 1) X(WW_1, ww_1, 1, 0) X(U, u, 1, 0) X(U_1, u_1, 1, 0) X(V, v, 1, 0) X(V_1, v_1, 1, 0)            \
    X(MU, mu, 1, 1) X(MUT, mut, 1, 0) X(MUAVE, muave, 0, 1) X(MUTS, muts, 0, 1) X(MUU, muu, 1, 0) X(MUV, muv, 1, 0) \
    X(MUDF, mudf, 0, 1) X(T, t, 1, 1) X(T_1, t_1, 1, 0) X(T_AVE, t_ave, 0, 1) X(FT, ft, 1, 0)                      \
    X(MU_TEND, mu_tend, 1, 0) X(DNW, dnw, 1, 0) X(FNM, fnm, 1, 0) X(FNP, fnp, 1, 0) X(RDNW, rdnw, 1, 0)            \
    X(MSFUY, msfuy, 1, 0) X(MSFVX_INV, msfvx_inv, 1, 0) X(MSFTX, msftx, 1, 0) X(MSFTY, msfty, 1, 0)

struct AmtFieldRole {
    int id;
    const char *name;
    bool in, out;
};
#define AMT_FIELD_ROW(ID, member, in, out) {AMT_F_##ID, #member, in != 0, out != 0},
constexpr AmtFieldRole kAmtField[] = {AMT_FIELDS(AMT_FIELD_ROW)};
#undef AMT_FIELD_ROW
constexpr bool amt_field_table_in_order()
{
    int nwrong = 0;
    for (int f = 0; f < AMT_F_COUNT; ++f) nwrong += kAmtField[f].id != f;
    return nwrong == 0;
}
static_assert(sizeof kAmtField / sizeof *kAmtField == AMT_F_COUNT && amt_field_table_in_order(), "AMT_FIELDS must follow enum amt_field");
inline const char *amt_field_name(int f) { return kAmtField[f].name; }

// AmtArgs <-> an array of the AMT_F_COUNT array pointers, indexed by AMT_F_*
template <typename T>
inline void amt_args_get_fields(const AmtArgs<T> &a, const T *q[AMT_F_COUNT])
{
#define AMT_FIELD_GET(ID, member, in, out) q[AMT_F_##ID] = a.member;
    AMT_FIELDS(AMT_FIELD_GET)
#undef AMT_FIELD_GET
}
template <typename T>
inline void amt_args_set_fields(AmtArgs<T> &a, T *const q[AMT_F_COUNT])
{
#define AMT_FIELD_SET(ID, member, in, out) a.member = q[AMT_F_##ID];
    AMT_FIELDS(AMT_FIELD_SET)
#undef AMT_FIELD_SET
}

// Checks the preconditions and rebases the Fortran bounds to memory-relative zero-based ones;
// *empty is set when the compute window holds no column (amt_api.hip).
template <typename T> int amt_build_params(const AmtArgs<T> &a, AmtParams<T> &p, AmtWindow &w, bool *empty);
// bounds check + kernel launch on a stream: the device-resident entry point (amt_api.hip)
template <typename T> int amt_device_call(void *hip_stream, int variant, const AmtArgs<T> &a);
// the same for the first and the last row of the window only (one launch where the march kernel runs)
template <typename T> int amt_device_call_edges(void *hip_stream, int variant, const AmtArgs<T> &a);
extern template int amt_build_params<float>(const AmtArgs<float> &, AmtParams<float> &, AmtWindow &, bool *);
extern template int amt_build_params<double>(const AmtArgs<double> &, AmtParams<double> &, AmtWindow &, bool *);
extern template int amt_device_call<float>(void *, int, const AmtArgs<float> &);
extern template int amt_device_call<double>(void *, int, const AmtArgs<double> &);
// the whole window, launched beside another stream's kernels (planned in at least two rounds of workgroups)
template <typename T> int amt_device_call_shared(void *hip_stream, int variant, const AmtArgs<T> &a);
extern template int amt_device_call_shared<float>(void *, int, const AmtArgs<float> &);
extern template int amt_device_call_shared<double>(void *, int, const AmtArgs<double> &);
// `members` patches of these bounds, member-stacked arrays, one launch (amt_ensemble.hip)
template <typename T> int amt_device_call_ensemble(void *hip_stream, int variant, int members, const AmtArgs<T> &a);
extern template int amt_device_call_ensemble<float>(void *, int, int, const AmtArgs<float> &);
extern template int amt_device_call_ensemble<double>(void *, int, int, const AmtArgs<double> &);
extern template int amt_device_call_edges<float>(void *, int, const AmtArgs<float> &);
extern template int amt_device_call_edges<double>(void *, int, const AmtArgs<double> &);

#define AMT_PACK_ARGS(T)                                                                        \
    AmtArgs<T> a;                                                                               \
    a.ww = ww; a.ww_1 = ww_1; a.u = u; a.u_1 = u_1; a.v = v; a.v_1 = v_1; a.mu = mu;            \
    a.mut = mut; a.muave = muave; a.muts = muts; a.muu = muu; a.muv = muv; a.mudf = mudf;       \
    a.t = t; a.t_1 = t_1; a.t_ave = t_ave; a.ft = ft; a.mu_tend = mu_tend;                      \
    a.rdx = rdx; a.rdy = rdy; a.dts = dts; a.epssm = epssm;                                     \
    a.dnw = dnw; a.fnm = fnm; a.fnp = fnp; a.rdnw = rdnw; a.msfuy = msfuy;                      \
    a.msfvx_inv = msfvx_inv; a.msftx = msftx; a.msfty = msfty;                                  \
    a.periodic_x = periodic_x; a.specified = specified; a.nested = nested;                      \
    a.ids = ids; a.ide = ide; a.jds = jds; a.jde = jde; a.kde = kde;                            \
    a.ims = ims; a.ime = ime; a.jms = jms; a.jme = jme; a.kms = kms; a.kme = kme;               \
    a.its = its; a.ite = ite; a.jts = jts; a.jte = jte; a.kts = kts; a.kte = kte;

#define AMT_SIG(T)                                                                              \
    T *ww, const T *ww_1, const T *u, const T *u_1, const T *v, const T *v_1,                   \
    T *mu, const T *mut, T *muave, T *muts, const T *muu, const T *muv,                         \
    T *mudf, T *t, const T *t_1, T *t_ave, const T *ft, const T *mu_tend,                       \
    T rdx, T rdy, T dts, T epssm,                                                               \
    const T *dnw, const T *fnm, const T *fnp, const T *rdnw,                                    \
    const T *msfuy, const T *msfvx_inv, const T *msftx, const T *msfty,                         \
    int periodic_x, int specified, int nested,                                                  \
    int ids, int ide, int jds, int jde, int kde,                                                \
    int ims, int ime, int jms, int jme, int kms, int kme,                                       \
    int its, int ite, int jts, int jte, int kts, int kte


// ---------------------------------------------------------------------------
// resident domain handle (amt_domain.hip), also stepped by the grid and slab steppers (amt_grid.hip)
// ---------------------------------------------------------------------------
namespace {
// makes the domain's device current for the duration of a call and restores the caller's
struct DeviceScope {
    int prev = -1;
    bool switched = false;
    explicit DeviceScope(int want)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != want) switched = (hipSetDevice(want) == hipSuccess);
    }
    ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
};
}  // namespace

struct AmtDiagState;              // workspace, result records and guard state of section (10) (amt_diag.hip)

struct amt_domain {
    int dtype_bytes = 8;
    int periodic_x = 0, specified = 0, nested = 0;
    int ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte;
    double rdx = AMT_SYNTH_RDX, rdy = AMT_SYNTH_RDY, dts = AMT_SYNTH_DTS, epssm = AMT_SYNTH_EPSSM;
    int variant = AMT_VARIANT_AUTO;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    void *field[AMT_F_COUNT] = {};
    bool owns_fields = true;      // false: the arrays belong to the caller (amt_domain_wrap)
    bool owns_stream = true;      // false: the stream belongs to the caller
    int cyclic = 0;               // amt_cyclic_axes refreshed in front of every sweep (amt_domain_set_cyclic); 0 = off
    int spec_bdy = 0;             // 1: the boundary-zone update follows every sweep (amt_domain_set_spec_bdy); 0 = off
    int placement_tries = 0;      // allocations of the state that were timed (amt_domain_create / amt_domain_tune_placement)
    float placement_ms[16] = {};  // sweep time on each (0: not tried)
    int guard_every = 0;          // non-finite guard: check after every n-th sweep (amt_domain_set_guard); 0 = off
    AmtDiagState *diag = nullptr; // made by the first call of section (10) on this handle, freed with it
    int sumflux_n = 0;            // n_small_steps: one flux accumulation follows every sweep (amt_domain_set_sumflux); 0 = off
    int sumflux_next = 1;         // the iteration the next accumulation is, 1..sumflux_n
    void *sumflux_acc[3] = {};    // ru_m, rv_m, ww_m: one 3-D field's extents each (times the members of an ensemble)
    bool sumflux_owned = false;   // true: allocated by the library, freed with the setting or the handle
    bool stage_on = false;        // the Runge-Kutta stage bracket is set up (amt_domain_set_stage)
    void *stage_arr[4] = {};      // t_old (3-D), mu_old, mu_save, mub (2-D), times the members of an ensemble
    bool stage_owned = false;     // true: allocated by the library, freed with the setting or the handle
    int p_rho_mode = 0;           // the pressure diagnosis (amt_domain_set_p_rho): 1 non-hydrostatic, 2 hydrostatic; 0 = off
    int p_rho_per_sweep = 0;      // 1: one diagnosis with step != 0 follows every sweep
    double p_rho_t0 = 0., p_rho_smdiv = 0.;
    void *p_rho_arr[8] = {};      // al, p, ph, pm1, alt, c2a (3-D, times the members of an ensemble), znu, dnw (1-D, shared)
    bool p_rho_owned = false;     // true: allocated by the library, freed with the setting or the handle
    int uv_on = 0;                // the momentum update (amt_domain_set_uv); it reads the pressure diagnosis's al, p, ph, alt
    int uv_per_sweep = 0;         // 1: one update precedes every sweep
    double uv_emdiv = 0., uv_cf1 = 0., uv_cf2 = 0., uv_cf3 = 0.;
    void *uv_arr[9] = {};         // ru_tend, rv_tend, pb, php, cqu, cqv (3-D, times the members), msfux, msfvx, msfvy (2-D)
    bool uv_owned = false;        // true: allocated by the library, freed with the setting or the handle
    size_t count(int f) const
    {
        const size_t idim = ime - ims + 1, kdim = kme - kms + 1, jdim = jme - jms + 1;
        const int r = amt_field_rank(f);
        return r == 3 ? idim * kdim * jdim : r == 2 ? idim * jdim : kdim;
    }
};

// resident ensemble handle (amt_ensemble.hip).  The bounds, flags, scalars, variant, stream and the 26 BASE pointers live in an
// amt_domain (so that amt_domain_args packs the call); what that struct calls a field's count is ONE member's: a rank-3 or
// rank-2 array holds `members` of them, a rank-1 array is shared.
struct amt_ensemble {
    amt_domain d;
    int members = 1;
};

template <typename T>
inline void amt_domain_args(amt_domain *d, AmtArgs<T> &a)
{
    amt_args_set_fields(a, reinterpret_cast<T *const *>(d->field));
    a.rdx = (T)d->rdx; a.rdy = (T)d->rdy; a.dts = (T)d->dts; a.epssm = (T)d->epssm;
    a.periodic_x = d->periodic_x; a.specified = d->specified; a.nested = d->nested;
    a.ids = d->ids; a.ide = d->ide; a.jds = d->jds; a.jde = d->jde; a.kde = d->kde;
    a.ims = d->ims; a.ime = d->ime; a.jms = d->jms; a.jme = d->jme; a.kms = d->kms; a.kme = d->kme;
    a.its = d->its; a.ite = d->ite; a.jts = d->jts; a.jte = d->jte; a.kts = d->kts; a.kte = d->kte;
}

// the shape arguments of the create / wrap calls and of amt_halo_plan, in the header's order
#define AMT_SHAPE_SIG                                                                           \
    int dtype_bytes, int periodic_x, int specified, int nested,                                 \
    int ids, int ide, int jds, int jde, int kde,                                                \
    int ims, int ime, int jms, int jme, int kms, int kme,                                       \
    int its, int ite, int jts, int jte, int kts, int kte
#define AMT_SHAPE_ARGS                                                                          \
    dtype_bytes, periodic_x, specified, nested, ids, ide, jds, jde, kde,                        \
    ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte
// Hidden visibility down to the pop: these functions are new, and the library's dynamic symbol table stays what it was.
// (The older cross-file helpers below -- amt_cyclic_refresh_domain and the rest -- are exported C++ symbols by accident of the
// default visibility; nothing outside the library may call either kind.)
#pragma GCC visibility push(hidden)
void amt_domain_set_shape(amt_domain *d, AMT_SHAPE_SIG);

// ---------------------------------------------------------------------------
// The bodies under the exports amt_domain_* and amt_ensemble_* (amt_domain.hip).  An ensemble handle is an amt_domain plus a
// member count, so each is one function of (who, d, members): `who` the export's name for the error texts, `members` 1 for a
// domain.  The exports keep the null check and the argument checks whose texts differ, and are one call of these otherwise.
//   amt_handle_open:         behind the argument checks of create / wrap: d (shape set) gets the current device, a stream and
//                            two events, and adopts `fields` / `hip_stream` or allocates (fields == nullptr); on an error d
//                            holds nothing
//   amt_handle_close:        releases everything d holds (the caller deletes the handle)
//   amt_handle_step:         THE SWEEP SEQUENCE of a resident handle, n_sweeps times: guard status, then per sweep
//                                [cyclic refresh] -> sweep -> [zone update] -> [accumulation] -> [pressure diagnosis] -> [guard check]
//                            stacked = false: the single-patch launch amt_device_call (a domain); true: the launch
//                            amt_device_call_ensemble (an ensemble, also one of a single member).  A per-sweep setting is a
//                            member at the END of amt_domain, a line of this sequence, and -- when the placement sampling must
//                            not see it -- a line of StepExtrasPause next to it.
//   amt_handle_behind_sweep: the part behind the sweep that the grid and slab steppers share with it (amt_grid.hip): zone update,
//                            then accumulation, then the pressure diagnosis; NOT the guard check
//   amt_handle_copy:         device scope, one asynchronous copy between `dev` (inside an array of d) and `host`, stream sync
//   amt_handle_fill:         the fields of `field_mask` from the generator, member m with seed + m at its offset
// ---------------------------------------------------------------------------
int amt_handle_open(const char *who, amt_domain *d, int members, void *const *fields, void *hip_stream);
void amt_handle_close(amt_domain *d);
int amt_handle_set_scalars(amt_domain *d, double rdx, double rdy, double dts, double epssm);
int amt_handle_set_variant(amt_domain *d, int variant);
int amt_handle_step(const char *who, amt_domain *d, int members, bool stacked, int n_sweeps);
int amt_handle_step_timed(const char *who_step, const char *who, amt_domain *d, int members, bool stacked, int n_sweeps,
                          float *ms_total);
int amt_handle_behind_sweep(const char *who, amt_domain *d, int members);
int amt_handle_sync(const char *who, amt_domain *d);
int amt_handle_cyclic_fill(const char *who, amt_domain *d, int members, int axes);
int amt_handle_set_cyclic(const char *who, amt_domain *d, int members, int axes);
int amt_handle_spec_bdy_update(const char *who, amt_domain *d, int members);
int amt_handle_set_spec_bdy(const char *who, amt_domain *d, int members, int on);
void *amt_handle_field_ptr(amt_domain *d, int field);
// the Runge-Kutta stage bracket (header section 15): NOT part of the sweep sequence, a host calls them around its acoustic loop
int amt_handle_set_stage(const char *who, amt_domain *d, int members, int on, void *t_old, void *mu_old, void *mu_save, void *mub);
void *amt_handle_stage_ptr(amt_domain *d, int which);
int amt_handle_stage_prep(const char *who, amt_domain *d, int members, int rk_step);
int amt_handle_stage_finish(const char *who, amt_domain *d, int members, int n_small_steps, const void *h_diabatic);
// the pressure diagnosis that closes an acoustic sub-step (header section 16): a per-sweep setting when per_sweep != 0
int amt_handle_set_p_rho(const char *who, amt_domain *d, int members, int mode, int per_sweep, double t0, double smdiv,
                         void *al, void *p, void *ph, void *pm1, void *alt, void *c2a, void *znu, void *dnw);
void *amt_handle_p_rho_ptr(amt_domain *d, int which);
int amt_handle_p_rho(const char *who, amt_domain *d, int members, int step);
// the momentum update that opens an acoustic sub-step (header section 17): in front of every sweep when per_sweep != 0
int amt_handle_set_uv(const char *who, amt_domain *d, int members, int on, int per_sweep, double emdiv, double cf1, double cf2, double cf3,
                      void *const arr[9]);
void *amt_handle_uv_ptr(amt_domain *d, int which);
int amt_handle_uv(const char *who, amt_domain *d, int members);
int amt_handle_copy(amt_domain *d, void *dev, void *host, size_t bytes, bool up);
int amt_handle_fill(amt_domain *d, int members, uint64_t field_mask, uint64_t seed,
                    long gi0, long gk0, long gj0, long gidim, long gkdim, long gjdim);
#pragma GCC visibility pop

// ---------------------------------------------------------------------------
// cyclic lateral boundaries (amt_cyclic.hip): one refresh of `members` member-stacked patches of the domain's shape on the
// domain's stream, and the argument / precondition checks alone (host arithmetic)
// ---------------------------------------------------------------------------
int amt_cyclic_refresh_domain(const char *who, amt_domain *d, int axes, int members);
int amt_cyclic_check_domain(const char *who, const amt_domain *d, int axes, int members);

// ---------------------------------------------------------------------------
// specified / nested lateral boundaries (amt_bdy.hip, header section 12): one boundary-zone update of `members`
// member-stacked patches of the domain's shape on the domain's stream, with the domain's dts, and the argument /
// precondition checks alone (host arithmetic).  An empty zone enqueues nothing.
// ---------------------------------------------------------------------------
int amt_bdy_update_domain(const char *who, amt_domain *d, int members);
int amt_bdy_check_domain(const char *who, const amt_domain *d, int members);

// ---------------------------------------------------------------------------
// The three streaming passes around the acoustic loop -- the flux averages, the stage bracket, the pressure diagnosis -- have
// their kernels, their scalar arguments and what their setting means in a file each; the check of a call, the layout of the
// tile box, the way from the check to the launch, the setting of a handle's arrays (all or none, the library's own handed
// back, the probe check, allocation, release) and the bounds of the pointer-level exports are amt_pass.h / amt_pass.hip.
// Each *_set_domain is amt_*_set_<pass>: a refusal changes nothing; each *_release turns the setting off and frees what the
// library allocated (the handles' destroy).
// ---------------------------------------------------------------------------
#include "amt_pass.h"

// ---------------------------------------------------------------------------
// the acoustic loop's flux averages (amt_sumflux.hip, header section 14).  The steppers call amt_sumflux_accumulate_domain
// only while the setting is on (d->sumflux_n != 0): with it off they enqueue what they always did.
//   amt_sumflux_accumulate_domain: one accumulation of `members` member-stacked patches of the domain's shape on the domain's
//                                  stream, as iteration d->sumflux_next, which then advances 1..n and wraps;
//                                  AMT_ERR_INVALID_ARG while the setting is off
//   amt_sumflux_set_domain:        n = 0: off; the library's own arrays handed back: n and the counter are set anew
// ---------------------------------------------------------------------------
int amt_sumflux_accumulate_domain(const char *who, amt_domain *d, int members);
int amt_sumflux_set_domain(const char *who, amt_domain *d, int members, int n, void *ru_m, void *rv_m, void *ww_m);
void amt_sumflux_release(amt_domain *d);

// ---------------------------------------------------------------------------
// the bracket of a Runge-Kutta stage (amt_stage.hip, header section 15): small_step_prep and small_step_finish of `members`
// member-stacked patches of the domain's shape on the domain's stream.  Nothing of the sweep sequence calls these.
//   amt_stage_prep_domain / amt_stage_finish_domain: AMT_ERR_PRECONDITION while the setting is off; finish uses the domain's dts
//   amt_stage_set_domain:                            on = 0: off; the library's own arrays handed back: nothing changes
// ---------------------------------------------------------------------------
#pragma GCC visibility push(hidden)
int amt_stage_prep_domain(const char *who, amt_domain *d, int members, int rk_step);
int amt_stage_finish_domain(const char *who, amt_domain *d, int members, int n_small_steps, const void *h_diabatic);
int amt_stage_set_domain(const char *who, amt_domain *d, int members, int on, void *t_old, void *mu_old, void *mu_save, void *mub);
void amt_stage_release(amt_domain *d);
#pragma GCC visibility pop

// ---------------------------------------------------------------------------
// the pressure diagnosis calc_p_rho (amt_p_rho.hip, header section 16) of `members` member-stacked patches of the domain's shape
// on the domain's stream.  The steppers call amt_p_rho_domain only while d->p_rho_per_sweep is set.
//   amt_p_rho_domain:     one diagnosis; AMT_ERR_PRECONDITION while the setting or the stage bracket (t_old) is off
//   amt_p_rho_set_domain: mode = 0: off; arr = al, p, ph, pm1, alt, c2a, znu, dnw; AMT_ERR_PRECONDITION while the stage bracket
//                         is off; the library's own arrays handed back: the mode and the scalars are set anew
// ---------------------------------------------------------------------------
#pragma GCC visibility push(hidden)
// advance_uv (amt_uv.hip, header section 17) of `members` member-stacked patches on the domain's stream, behind the wrap refresh
// of its eight read arrays on a cyclic handle; AMT_ERR_PRECONDITION while its setting or the pressure diagnosis's is off
int amt_uv_domain(const char *who, amt_domain *d, int members);
int amt_uv_set_domain(const char *who, amt_domain *d, int members, int on, int per_sweep, double emdiv, double cf1, double cf2, double cf3,
                      void *const arr[9]);
void amt_uv_release(amt_domain *d);
int amt_p_rho_domain(const char *who, amt_domain *d, int members, int step);
int amt_p_rho_set_domain(const char *who, amt_domain *d, int members, int mode, int per_sweep, double t0, double smdiv, void *const arr[8]);
void amt_p_rho_release(amt_domain *d);
#pragma GCC visibility pop

// ---------------------------------------------------------------------------
// field statistics, comparison and the non-finite guard (amt_diag.hip, header section 10).  The steppers call these only
// while a guard is armed (d->guard_every != 0): with it off they enqueue what they always did.
//   amt_diag_guard_status: AMT_ERR_NONFINITE (with the text of amt_last_error) when the guard's host record shows a finding
//                          NOW, else AMT_OK; reads page-locked host memory, never waits
//   amt_diag_after_sweep:  one more sweep of `members` member-stacked patches was enqueued on d->stream; on every n-th the
//                          three checks follow it on the same stream
//   amt_diag_release:      frees d->diag (the handles' destroy)
// ---------------------------------------------------------------------------
int amt_diag_guard_status(const char *who, const amt_domain *d);
int amt_diag_after_sweep(const char *who, amt_domain *d, int members);
void amt_diag_release(amt_domain *d);

// ---------------------------------------------------------------------------
// The BOX of header section 10, for the other passes over resident state (amt_moments.hip): the checks of amt_diag.hip and
// what they work out, in elements -- host arithmetic only, an error is AMT_ERR_INVALID_ARG with its text.
//   amt_box_plan:   a box i0..i1, k0..k1, j0..j1 inside the extents of a rank-2 / rank-3 field (rank 2 ignores k)
//   amt_box_region: AMT_REGION_WINDOW / AMT_REGION_MEMORY of a field of a handle; *empty (with AMT_OK) when the compute
//                   window holds no cell
// ---------------------------------------------------------------------------
struct AmtBox {
    long idim;        // elements of a memory row of i
    long jstride;     // elements from row j to row j + 1
    long mstride;     // elements from member m to member m + 1
    long first;       // offset of the box's first element from the member's base
    int ni, nk, nj;   // the box; nk = 1 for rank 2
};
int amt_box_plan(const char *who, int rank, int members, int ims, int ime, int jms, int jme, int kms, int kme,
                 int i0, int i1, int k0, int k1, int j0, int j1, AmtBox *box);
int amt_box_region(const char *who, const amt_domain *d, int field, int region, int members, AmtBox *box, bool *empty);
