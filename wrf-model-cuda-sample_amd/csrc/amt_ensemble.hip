// amt_ensemble.hip -- ensembles: `members` patches of one shape advanced by ONE launch per sweep (header section 8,
// DESIGN.md section 4.4).  Every 3-D and 2-D array has one more, slowest, dimension -- member m's row j is row m * jdim + j of a
// taller array -- and bounds, flags, scalars and the four 1-D metric arrays are shared.  The device-resident drop-in
// amt_advance_mu_t_ensemble_device_* and a resident handle amt_ensemble_* that mirrors amt_domain_*: its own argument checks and
// error texts over the bodies amt_handle_* of amt_domain.hip, called with the handle's member count.
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
    if (e) amt_handle_close(&e->d);
    delete e;
    return AMT_OK;
}

// fields == nullptr: allocate the stacked arrays (amt_ensemble_create); otherwise adopt the caller's (amt_ensemble_wrap)
static int amt_ensemble_make(amt_ensemble **out, int members, AMT_SHAPE_SIG, void *const *fields, void *hip_stream)
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
    amt_ensemble *e = new (std::nothrow) amt_ensemble;
    if (!e) return amt_fail(AMT_ERR_ALLOC, "host allocation failed");
    e->members = members;
    amt_domain_set_shape(&e->d, AMT_SHAPE_ARGS);
    const int rc = amt_handle_open("amt_ensemble_create", &e->d, members, fields, hip_stream);
    if (rc) delete e;
    else *out = e;
    return rc;
}

extern "C" int amt_ensemble_create(amt_ensemble **out, int members, AMT_SHAPE_SIG)
{
    return amt_ensemble_make(out, members, AMT_SHAPE_ARGS, nullptr, nullptr);
}

extern "C" int amt_ensemble_wrap(amt_ensemble **out, int members, AMT_SHAPE_SIG, void *const *fields, void *hip_stream)
{
    if (!fields) return amt_fail(AMT_ERR_INVALID_ARG, "amt_ensemble_wrap needs the %d device pointers", (int)AMT_F_COUNT);
    return amt_ensemble_make(out, members, AMT_SHAPE_ARGS, fields, hip_stream);
}

static int amt_null_ensemble() { return amt_fail(AMT_ERR_INVALID_ARG, "null ensemble"); }

extern "C" int amt_ensemble_set_scalars(amt_ensemble *e, double rdx, double rdy, double dts, double epssm)
{
    return e ? amt_handle_set_scalars(&e->d, rdx, rdy, dts, epssm) : amt_null_ensemble();
}

extern "C" int amt_ensemble_set_variant(amt_ensemble *e, int variant)
{
    return e ? amt_handle_set_variant(&e->d, variant) : amt_null_ensemble();
}

extern "C" int amt_ensemble_members(const amt_ensemble *e) { return e ? e->members : 0; }

// one member of a field: contiguous in the stacked layout (a rank-1 field is shared: `member` only has to name a member)
static int amt_ensemble_copy_member(amt_ensemble *e, int field, int member, void *host, bool up)
{
    if (!e || !host || field < 0 || field >= AMT_F_COUNT) return amt_fail(AMT_ERR_INVALID_ARG, "bad member-copy argument");
    if (member < 0 || member >= e->members) return amt_fail(AMT_ERR_INVALID_ARG, "member %d not in 0..%d", member, e->members - 1);
    const size_t bytes = e->d.count(field) * (size_t)e->d.dtype_bytes;
    char *dev = static_cast<char *>(e->d.field[field]) + (amt_field_rank(field) == 1 ? (size_t)0 : (size_t)member * bytes);
    return amt_handle_copy(&e->d, dev, host, bytes, up);
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
                                           long gi0, long gk0, long gj0, long gidim, long gkdim, long gjdim)
{
    return e ? amt_handle_fill(&e->d, e->members, ~0ull, seed, gi0, gk0, gj0, gidim, gkdim, gjdim) : amt_null_ensemble();
}

extern "C" int amt_ensemble_cyclic_fill(amt_ensemble *e, int axes)
{
    return e ? amt_handle_cyclic_fill("amt_ensemble_cyclic_fill", &e->d, e->members, axes) : amt_null_ensemble();
}
extern "C" int amt_ensemble_set_cyclic(amt_ensemble *e, int axes)
{
    return e ? amt_handle_set_cyclic("amt_ensemble_set_cyclic", &e->d, e->members, axes) : amt_null_ensemble();
}
extern "C" int amt_ensemble_cyclic(const amt_ensemble *e) { return e ? e->d.cyclic : 0; }
extern "C" int amt_ensemble_spec_bdy_update(amt_ensemble *e)
{
    return e ? amt_handle_spec_bdy_update("amt_ensemble_spec_bdy_update", &e->d, e->members) : amt_null_ensemble();
}
extern "C" int amt_ensemble_set_spec_bdy(amt_ensemble *e, int on)
{
    return e ? amt_handle_set_spec_bdy("amt_ensemble_set_spec_bdy", &e->d, e->members, on) : amt_null_ensemble();
}
extern "C" int amt_ensemble_spec_bdy(const amt_ensemble *e) { return e ? e->d.spec_bdy : 0; }

extern "C" int amt_ensemble_set_stage(amt_ensemble *e, int on, void *t_old, void *mu_old, void *mu_save, void *mub)
{
    return e ? amt_handle_set_stage("amt_ensemble_set_stage", &e->d, e->members, on, t_old, mu_old, mu_save, mub) : amt_null_ensemble();
}
extern "C" void *amt_ensemble_stage_ptr(amt_ensemble *e, int which) { return e ? amt_handle_stage_ptr(&e->d, which) : nullptr; }
extern "C" int amt_ensemble_stage_prep(amt_ensemble *e, int rk_step)
{
    return e ? amt_handle_stage_prep("amt_ensemble_stage_prep", &e->d, e->members, rk_step) : amt_null_ensemble();
}
extern "C" int amt_ensemble_stage_finish(amt_ensemble *e, int n_small_steps, const void *h_diabatic)
{
    return e ? amt_handle_stage_finish("amt_ensemble_stage_finish", &e->d, e->members, n_small_steps, h_diabatic) : amt_null_ensemble();
}

extern "C" int amt_ensemble_set_p_rho(amt_ensemble *e, int mode, int per_sweep, double t0, double smdiv, void *al, void *p, void *ph,
                                     void *pm1, void *alt, void *c2a, void *znu, void *dnw)
{
    return e ? amt_handle_set_p_rho("amt_ensemble_set_p_rho", &e->d, e->members, mode, per_sweep, t0, smdiv, al, p, ph, pm1, alt, c2a, znu, dnw)
             : amt_null_ensemble();
}
extern "C" int amt_ensemble_set_uv(amt_ensemble *e, int on, int per_sweep, double emdiv, double cf1, double cf2, double cf3, void *ru_tend,
                                  void *rv_tend, void *pb, void *php, void *cqu, void *cqv, void *msfux, void *msfvx, void *msfvy)
{
    void *const arr[9] = {ru_tend, rv_tend, pb, php, cqu, cqv, msfux, msfvx, msfvy};
    return e ? amt_handle_set_uv("amt_ensemble_set_uv", &e->d, e->members, on, per_sweep, emdiv, cf1, cf2, cf3, arr) : amt_null_ensemble();
}
extern "C" void *amt_ensemble_uv_ptr(amt_ensemble *e, int which) { return e ? amt_handle_uv_ptr(&e->d, which) : nullptr; }
extern "C" int amt_ensemble_uv(amt_ensemble *e) { return e ? amt_handle_uv("amt_ensemble_uv", &e->d, e->members) : amt_null_ensemble(); }
extern "C" void *amt_ensemble_p_rho_ptr(amt_ensemble *e, int which) { return e ? amt_handle_p_rho_ptr(&e->d, which) : nullptr; }
extern "C" int amt_ensemble_p_rho(amt_ensemble *e, int step)
{
    return e ? amt_handle_p_rho("amt_ensemble_p_rho", &e->d, e->members, step) : amt_null_ensemble();
}

extern "C" int amt_ensemble_step(amt_ensemble *e, int n_sweeps)
{
    if (!e || n_sweeps < 0) return amt_fail(AMT_ERR_INVALID_ARG, "bad step argument");
    return amt_handle_step("amt_ensemble_step", &e->d, e->members, true, n_sweeps);
}

extern "C" int amt_ensemble_step_timed(amt_ensemble *e, int n_sweeps, float *ms_total)
{
    if (!e || n_sweeps < 0) return amt_fail(AMT_ERR_INVALID_ARG, "bad step argument");
    return amt_handle_step_timed("amt_ensemble_step", "amt_ensemble_step_timed", &e->d, e->members, true, n_sweeps, ms_total);
}

extern "C" int amt_ensemble_sync(amt_ensemble *e) { return e ? amt_handle_sync("amt_ensemble_sync", &e->d) : amt_null_ensemble(); }
extern "C" void *amt_ensemble_field_ptr(amt_ensemble *e, int field) { return e ? amt_handle_field_ptr(&e->d, field) : nullptr; }
extern "C" void *amt_ensemble_stream(amt_ensemble *e) { return e ? (void *)e->d.stream : nullptr; }
