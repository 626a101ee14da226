// amt_ensemble.hip -- ensembles: `members` patches of one shape advanced by ONE launch per sweep (header section 8,
// DESIGN.md section 4.4).  Every 3-D and 2-D array has one more, slowest, dimension -- member m's row j is row m * jdim + j of a
// taller array -- and bounds, flags, scalars and the four 1-D metric arrays are shared.  The device-resident drop-in
// amt_advance_mu_t_ensemble_device_* and a resident handle amt_ensemble_* that mirrors amt_domain_*.
#include "amt_internal.h"

extern "C" int amt_advance_mu_t_ensemble_device_f32(void *hip_stream, int variant, int members, AMT_SIG(float))
{
    AMT_PACK_ARGS(float)
    return amt_device_call_ensemble<float>(hip_stream, variant, members, a);
}
extern "C" int amt_advance_mu_t_ensemble_device_f64(void *hip_stream, int variant, int members, AMT_SIG(double))
{
    AMT_PACK_ARGS(double)
    return amt_device_call_ensemble<double>(hip_stream, variant, members, a);
}

extern "C" int amt_ensemble_destroy(amt_ensemble *e)
{
    if (!e) return AMT_OK;
    amt_domain &d = e->d;
    DeviceScope scope(d.device);
    amt_diag_release(&d);
    amt_sumflux_release(&d);
    if (d.owns_fields)
        for (void *&q : d.field)
            if (q) { (void)hipFree(q); q = nullptr; }
    if (d.ev0) (void)hipEventDestroy(d.ev0);
    if (d.ev1) (void)hipEventDestroy(d.ev1);
    if (d.stream && d.owns_stream) (void)hipStreamDestroy(d.stream);
    delete e;
    return AMT_OK;
}

// fields == nullptr: allocate the stacked arrays (amt_ensemble_create); otherwise adopt the caller's (amt_ensemble_wrap)
static int amt_ensemble_make(amt_ensemble **out, int members, int dtype_bytes,
                             int periodic_x, int specified, int nested,
                             int ids, int ide, int jds, int jde, int kde,
                             int ims, int ime, int jms, int jme, int kms, int kme,
                             int its, int ite, int jts, int jte, int kts, int kte,
                             void *const *fields, void *hip_stream)
{
    if (!out) return amt_fail(AMT_ERR_INVALID_ARG, "null out pointer");
    *out = nullptr;
    if (members < 1) return amt_fail(AMT_ERR_INVALID_ARG, "members = %d: an ensemble has at least one member", members);
    if (dtype_bytes != 4 && dtype_bytes != 8) return amt_fail(AMT_ERR_INVALID_ARG, "dtype_bytes must be 4 or 8");
    if (ime < ims || jme < jms || kme < kms) return amt_fail(AMT_ERR_PRECONDITION, "empty memory extents");
    if ((long)members * (jme - jms + 1) > 0x7fffffffL)
        return amt_fail(AMT_ERR_PRECONDITION, "%d members of %d rows: the stacked arrays have more than 2^31 - 1 rows", members, jme - jms + 1);
    if (fields)
        for (int f = 0; f < AMT_F_COUNT; ++f)
            if (!fields[f]) return amt_fail(AMT_ERR_INVALID_ARG, "amt_ensemble_wrap: field %d is a null pointer", f);
    int ndev = 0;
    AMT_HIP(hipGetDeviceCount(&ndev));
    if (ndev < 1) return amt_fail(AMT_ERR_NO_DEVICE, "no HIP device visible");
    amt_ensemble *e = new (std::nothrow) amt_ensemble;
    if (!e) return amt_fail(AMT_ERR_ALLOC, "host allocation failed");
    e->members = members;
    amt_domain &d = e->d;
    d.dtype_bytes = dtype_bytes;
    d.periodic_x = periodic_x; d.specified = specified; d.nested = nested;
    d.ids = ids; d.ide = ide; d.jds = jds; d.jde = jde; d.kde = kde;
    d.ims = ims; d.ime = ime; d.jms = jms; d.jme = jme; d.kms = kms; d.kme = kme;
    d.its = its; d.ite = ite; d.jts = jts; d.jte = jte; d.kts = kts; d.kte = kte;
    d.owns_fields = (fields == nullptr);
    d.owns_stream = (hip_stream == nullptr);
    hipError_t err = hipGetDevice(&d.device);
    if (hip_stream) d.stream = static_cast<hipStream_t>(hip_stream);
    else if (err == hipSuccess) err = hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking);
    if (err == hipSuccess) err = hipEventCreate(&d.ev0);
    if (err == hipSuccess) err = hipEventCreate(&d.ev1);
    for (int f = 0; f < AMT_F_COUNT && err == hipSuccess; ++f) {
        if (fields) d.field[f] = fields[f];
        else err = hipMalloc(&d.field[f], e->count(f) * (size_t)dtype_bytes);
    }
    if (err != hipSuccess) {
        amt_ensemble_destroy(e);
        return amt_fail(err == hipErrorOutOfMemory ? AMT_ERR_ALLOC : AMT_ERR_HIP, "amt_ensemble_create: %s", hipGetErrorString(err));
    }
    *out = e;
    return AMT_OK;
}

extern "C" int amt_ensemble_create(amt_ensemble **out, int members, int dtype_bytes,
                                   int periodic_x, int specified, int nested,
                                   int ids, int ide, int jds, int jde, int kde,
                                   int ims, int ime, int jms, int jme, int kms, int kme,
                                   int its, int ite, int jts, int jte, int kts, int kte)
{
    return amt_ensemble_make(out, members, dtype_bytes, periodic_x, specified, nested, ids, ide, jds, jde, kde,
                             ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte, nullptr, nullptr);
}

extern "C" int amt_ensemble_wrap(amt_ensemble **out, int members, int dtype_bytes,
                                 int periodic_x, int specified, int nested,
                                 int ids, int ide, int jds, int jde, int kde,
                                 int ims, int ime, int jms, int jme, int kms, int kme,
                                 int its, int ite, int jts, int jte, int kts, int kte,
                                 void *const *fields, void *hip_stream)
{
    if (!fields) return amt_fail(AMT_ERR_INVALID_ARG, "amt_ensemble_wrap needs the %d device pointers", (int)AMT_F_COUNT);
    return amt_ensemble_make(out, members, dtype_bytes, periodic_x, specified, nested, ids, ide, jds, jde, kde,
                             ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte, fields, hip_stream);
}

extern "C" int amt_ensemble_set_scalars(amt_ensemble *e, double rdx, double rdy, double dts, double epssm)
{
    if (!e) return amt_fail(AMT_ERR_INVALID_ARG, "null ensemble");
    e->d.rdx = rdx; e->d.rdy = rdy; e->d.dts = dts; e->d.epssm = epssm;
    return AMT_OK;
}

extern "C" int amt_ensemble_set_variant(amt_ensemble *e, int variant)
{
    if (!e) return amt_fail(AMT_ERR_INVALID_ARG, "null ensemble");
    if (variant < AMT_VARIANT_AUTO || variant > AMT_VARIANT_MARCH)
        return amt_fail(AMT_ERR_INVALID_ARG, "unknown variant %d", variant);
    e->d.variant = variant;
    return AMT_OK;
}

extern "C" int amt_ensemble_members(const amt_ensemble *e) { return e ? e->members : 0; }

// one member of a field: contiguous in the stacked layout (a rank-1 field is shared: `member` only has to name a member)
static int amt_ensemble_copy_member(amt_ensemble *e, int field, int member, void *host, bool up)
{
    if (!e || !host || field < 0 || field >= AMT_F_COUNT) return amt_fail(AMT_ERR_INVALID_ARG, "bad member-copy argument");
    if (member < 0 || member >= e->members) return amt_fail(AMT_ERR_INVALID_ARG, "member %d not in 0..%d", member, e->members - 1);
    amt_domain &d = e->d;
    const size_t bytes = d.count(field) * (size_t)d.dtype_bytes;
    char *dev = static_cast<char *>(d.field[field]) + (amt_field_rank(field) == 1 ? (size_t)0 : (size_t)member * bytes);
    DeviceScope scope(d.device);
    if (up) AMT_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, d.stream));
    else AMT_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, d.stream));
    AMT_HIP(hipStreamSynchronize(d.stream));
    return AMT_OK;
}

extern "C" int amt_ensemble_upload_member(amt_ensemble *e, int field, int member, const void *host)
{
    return amt_ensemble_copy_member(e, field, member, const_cast<void *>(host), true);
}

extern "C" int amt_ensemble_download_member(amt_ensemble *e, int field, int member, void *host)
{
    return amt_ensemble_copy_member(e, field, member, host, false);
}

extern "C" int amt_ensemble_fill_synthetic(amt_ensemble *e, uint64_t seed,
                                           long gi0, long gk0, long gj0,
                                           long gidim, long gkdim, long gjdim)
{
    if (!e) return amt_fail(AMT_ERR_INVALID_ARG, "null ensemble");
    amt_domain &d = e->d;
    DeviceScope scope(d.device);
    const long idim = d.ime - d.ims + 1, kdim = d.kme - d.kms + 1, jdim = d.jme - d.jms + 1;
    for (int f = 0; f < AMT_F_COUNT; ++f) {
        const int rank = amt_field_rank(f);
        const size_t bytes = d.count(f) * (size_t)d.dtype_bytes;
        for (int m = 0; m < (rank == 1 ? 1 : e->members); ++m) {       // the vertical metrics do not depend on the seed
            int rc = amt_synth_fill_device(d.stream, f, d.dtype_bytes, static_cast<char *>(d.field[f]) + (size_t)m * bytes,
                                           seed + (uint64_t)m, idim, kdim, jdim, gi0, gk0, gj0, gidim, gkdim, gjdim);
            if (rc) return rc;
        }
    }
    return AMT_OK;
}

template <typename T>
static int amt_ensemble_step_t(amt_ensemble *e, int n_sweeps)
{
    AmtArgs<T> a;
    amt_domain_args<T>(&e->d, a);
    // an armed guard that already shows a finding: nothing is enqueued (no wait: the record is in host memory)
    if (e->d.guard_every) { const int rc = amt_diag_guard_status("amt_ensemble_step", &e->d); if (rc) return rc; }
    for (int s = 0; s < n_sweeps; ++s) {
        // cyclic boundaries: every member's wrap cells in one launch in front of the sweep, on the same stream
        int rc = e->d.cyclic ? amt_cyclic_refresh_domain("amt_ensemble_step", &e->d, e->d.cyclic, e->members) : AMT_OK;
        if (rc == AMT_OK) rc = amt_device_call_ensemble<T>(e->d.stream, e->d.variant, e->members, a);
        // specified / nested boundaries: every member's boundary zone in one launch behind the sweep
        if (rc == AMT_OK && e->d.spec_bdy) rc = amt_bdy_update_domain("amt_ensemble_step", &e->d, e->members);
        // the flux averages: every member's accumulation in one launch behind the boundary-zone update
        if (rc == AMT_OK && e->d.sumflux_n) rc = amt_sumflux_accumulate_domain("amt_ensemble_step", &e->d, e->members);
        if (rc == AMT_OK && e->d.guard_every) rc = amt_diag_after_sweep("amt_ensemble_step", &e->d, e->members);
        if (rc) return rc;
    }
    return AMT_OK;
}

extern "C" int amt_ensemble_cyclic_fill(amt_ensemble *e, int axes)
{
    if (!e) return amt_fail(AMT_ERR_INVALID_ARG, "null ensemble");
    DeviceScope scope(e->d.device);
    return amt_cyclic_refresh_domain("amt_ensemble_cyclic_fill", &e->d, axes, e->members);
}

extern "C" int amt_ensemble_set_cyclic(amt_ensemble *e, int axes)
{
    if (!e) return amt_fail(AMT_ERR_INVALID_ARG, "null ensemble");
    const int rc = amt_cyclic_check_domain("amt_ensemble_set_cyclic", &e->d, axes, e->members);
    if (rc == AMT_OK) e->d.cyclic = axes;
    return rc;
}

extern "C" int amt_ensemble_cyclic(const amt_ensemble *e) { return e ? e->d.cyclic : 0; }

extern "C" int amt_ensemble_spec_bdy_update(amt_ensemble *e)
{
    if (!e) return amt_fail(AMT_ERR_INVALID_ARG, "null ensemble");
    DeviceScope scope(e->d.device);
    return amt_bdy_update_domain("amt_ensemble_spec_bdy_update", &e->d, e->members);
}

extern "C" int amt_ensemble_set_spec_bdy(amt_ensemble *e, int on)
{
    if (!e) return amt_fail(AMT_ERR_INVALID_ARG, "null ensemble");
    if (!on) { e->d.spec_bdy = 0; return AMT_OK; }
    const int rc = amt_bdy_check_domain("amt_ensemble_set_spec_bdy", &e->d, e->members);
    if (rc == AMT_OK) e->d.spec_bdy = 1;
    return rc;
}

extern "C" int amt_ensemble_spec_bdy(const amt_ensemble *e) { return e ? e->d.spec_bdy : 0; }

extern "C" int amt_ensemble_step(amt_ensemble *e, int n_sweeps)
{
    if (!e || n_sweeps < 0) return amt_fail(AMT_ERR_INVALID_ARG, "bad step argument");
    DeviceScope scope(e->d.device);
    return e->d.dtype_bytes == 8 ? amt_ensemble_step_t<double>(e, n_sweeps) : amt_ensemble_step_t<float>(e, n_sweeps);
}

extern "C" int amt_ensemble_step_timed(amt_ensemble *e, int n_sweeps, float *ms_total)
{
    if (!e || n_sweeps < 0) return amt_fail(AMT_ERR_INVALID_ARG, "bad step argument");
    amt_domain &d = e->d;
    DeviceScope scope(d.device);
    AMT_HIP(hipEventRecord(d.ev0, d.stream));
    int rc = amt_ensemble_step(e, n_sweeps);
    if (rc) return rc;
    AMT_HIP(hipEventRecord(d.ev1, d.stream));
    AMT_HIP(hipEventSynchronize(d.ev1));
    float ms = 0.f;
    AMT_HIP(hipEventElapsedTime(&ms, d.ev0, d.ev1));
    if (ms_total) *ms_total = ms;
    return d.guard_every ? amt_diag_guard_status("amt_ensemble_step_timed", &d) : AMT_OK;
}

extern "C" int amt_ensemble_sync(amt_ensemble *e)
{
    if (!e) return amt_fail(AMT_ERR_INVALID_ARG, "null ensemble");
    DeviceScope scope(e->d.device);
    AMT_HIP(hipStreamSynchronize(e->d.stream));
    return e->d.guard_every ? amt_diag_guard_status("amt_ensemble_sync", &e->d) : AMT_OK;
}

extern "C" void *amt_ensemble_field_ptr(amt_ensemble *e, int field)
{
    if (!e || field < 0 || field >= AMT_F_COUNT) return nullptr;
    return e->d.field[field];
}

extern "C" void *amt_ensemble_stream(amt_ensemble *e) { return e ? (void *)e->d.stream : nullptr; }
