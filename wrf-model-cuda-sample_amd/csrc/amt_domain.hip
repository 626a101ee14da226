// amt_domain.hip -- the resident domain handle amt_domain_*: native owner of the 26 device arrays,
// a stream and the scalars, for C / Fortran hosts that keep the state on the GPU across sub-steps.
#include "amt_halo.h"
#include <fcntl.h>
#include <sys/file.h>
#include <time.h>
#include <unistd.h>

void amt_domain_set_shape(amt_domain *d, AMT_SHAPE_SIG)
{
    d->dtype_bytes = dtype_bytes;
    d->periodic_x = periodic_x; d->specified = specified; d->nested = nested;
    d->ids = ids; d->ide = ide; d->jds = jds; d->jde = jde; d->kde = kde;
    d->ims = ims; d->ime = ime; d->jms = jms; d->jme = jme; d->kms = kms; d->kme = kme;
    d->its = its; d->ite = ite; d->jts = jts; d->jte = jte; d->kts = kts; d->kte = kte;
}

void amt_handle_close(amt_domain *d)
{
    DeviceScope scope(d->device);
    amt_diag_release(d);
    amt_sumflux_release(d);
    amt_uv_release(d);
    amt_p_rho_release(d);
    amt_stage_release(d);
    if (d->owns_fields)
        for (void *&q : d->field)
            if (q) { (void)hipFree(q); q = nullptr; }
    if (d->ev0) (void)hipEventDestroy(d->ev0);
    if (d->ev1) (void)hipEventDestroy(d->ev1);
    if (d->stream && d->owns_stream) (void)hipStreamDestroy(d->stream);
}

// fields == nullptr: allocate the 26 arrays, `members` of every rank-3 and rank-2 one (create).  Otherwise adopt the caller's
// device arrays and, when given, the caller's stream (wrap): nothing is copied and nothing of the caller's is freed by close.
int amt_handle_open(const char *who, amt_domain *d, int members, void *const *fields, void *hip_stream)
{
    int ndev = 0;
    AMT_HIP(hipGetDeviceCount(&ndev));
    if (ndev < 1) return amt_fail(AMT_ERR_NO_DEVICE, "no HIP device visible");
    d->owns_fields = (fields == nullptr);
    d->owns_stream = (hip_stream == nullptr);
    hipError_t e = hipGetDevice(&d->device);
    if (hip_stream) d->stream = static_cast<hipStream_t>(hip_stream);
    else if (e == hipSuccess) e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&d->ev0);
    if (e == hipSuccess) e = hipEventCreate(&d->ev1);
    for (int f = 0; f < AMT_F_COUNT && e == hipSuccess; ++f) {
        if (fields) d->field[f] = fields[f];
        else e = hipMalloc(&d->field[f], d->count(f) * (amt_field_rank(f) == 1 ? 1 : (size_t)members) * (size_t)d->dtype_bytes);
    }
    if (e == hipSuccess) return AMT_OK;
    amt_handle_close(d);
    return amt_fail(e == hipErrorOutOfMemory ? AMT_ERR_ALLOC : AMT_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
}

extern "C" int amt_domain_destroy(amt_domain *d)
{
    if (d) amt_handle_close(d);
    delete d;
    return AMT_OK;
}

static int amt_domain_make(amt_domain **out, AMT_SHAPE_SIG, void *const *fields, void *hip_stream)
{
    if (!out) return amt_fail(AMT_ERR_INVALID_ARG, "null out pointer");
    *out = nullptr;
    if (dtype_bytes != 4 && dtype_bytes != 8) return amt_fail(AMT_ERR_INVALID_ARG, "dtype_bytes must be 4 or 8");
    if (ime < ims || jme < jms || kme < kms) return amt_fail(AMT_ERR_PRECONDITION, "empty memory extents");
    if (fields)
        for (int f = 0; f < AMT_F_COUNT; ++f)
            if (!fields[f]) return amt_fail(AMT_ERR_INVALID_ARG, "amt_domain_wrap: field %d is a null pointer", f);
    amt_domain *d = new (std::nothrow) amt_domain;
    if (!d) return amt_fail(AMT_ERR_ALLOC, "host allocation failed");
    amt_domain_set_shape(d, AMT_SHAPE_ARGS);
    const int rc = amt_handle_open("amt_domain_create", d, 1, fields, hip_stream);
    if (rc) delete d;
    else *out = d;
    return rc;
}

static int amt_domain_tune(amt_domain *d, int tries, float *ms_per_try, bool preserve);

// Do the ranks of this launch outnumber the devices this process sees (two test ranks on a one-GPU box, AMT_SLAB_TRANSPORT=ipc
// with --share-gpu)?  Then several of them would sample at the same time on one device: each holds twice its state plus the
// spacer for a moment -- a peer's allocation may fail -- and times its sweeps beside the others': noise.  
static bool amt_ranks_outnumber_devices(int ndev)
{
    const char *lw = getenv("LOCAL_WORLD_SIZE"), *w = getenv("WORLD_SIZE");
    const long n = lw && *lw ? atol(lw) : w && *w ? atol(w) : 1;
    return n > ndev;
}

// One sampler per device at a time, across processes: an advisory lock on a file named after the device's PCI address,
// held for the duration of the sampling (processes that share a device without saying so in their environment).  Gives up
// after 60 s and returns -1: the caller then takes its first allocation as it comes.
static int amt_placement_lock(int device)
{
    char bus[32] = "unknown";
    (void)hipDeviceGetPCIBusId(bus, (int)sizeof bus, device);
    for (char *q = bus; *q; ++q)
        if (*q == ':' || *q == '.' || *q == '/') *q = '_';
    char path[96];
    snprintf(path, sizeof path, "/tmp/amt_placement_%s.lock", bus);
    const int fd = open(path, O_CREAT | O_RDWR, 0666);
    if (fd < 0) return -1;
    for (int waited_ms = 0; flock(fd, LOCK_EX | LOCK_NB) != 0; waited_ms += 20) {
        if (waited_ms >= 60000) { close(fd); return -1; }
        struct timespec ts = {0, 20 * 1000 * 1000};
        nanosleep(&ts, nullptr);
    }
    return fd;
}

extern "C" int amt_domain_create(amt_domain **out, AMT_SHAPE_SIG)
{
    int rc = amt_domain_make(out, AMT_SHAPE_ARGS, nullptr, nullptr);
    if (rc != AMT_OK) return rc;
    // Placement sampling, on by default (a host that creates its handle ONCE must get the sweep time the
    // bench prints).  Which physical pages the driver hands out moves a sweep of a large domain by +-3 % and cannot be steered
    // (profiles/r03_placement.md, r05_placement.md: not the TLB, not the L2 channels -- below the L2), only sampled: the state
    // is allocated AMT_DOMAIN_PLACEMENT_TRIES times (default 4; 0 or 1 = take the first as it comes), one set after the other,
    // three sweeps of the handle's own kernel on each, the fastest kept.  Skipped for states under 256 MiB (nothing to gain), for
    // windows the routine cannot run, and where a second copy does not fit.  The arrays hold nothing yet: no contents move.
    amt_domain *d = *out;
    int tries = 4;
    if (const char *e = getenv("AMT_DOMAIN_PLACEMENT_TRIES")) tries = atoi(e);
    if (tries > 16) tries = 16;
    size_t state = 0;
    for (int f = 0; f < AMT_F_COUNT; ++f) state += d->count(f) * (size_t)dtype_bytes;
    size_t free_b = 0, total_b = 0;
    int ndev = 1;
    (void)hipGetDeviceCount(&ndev);
    if (tries > 1 && state >= ((size_t)256 << 20) && kts == 1 && kte == kde && !amt_ranks_outnumber_devices(ndev)) {
        // not when the ranks of this launch share devices; one sampler per device at a time otherwise (the memory check is made
        // with the lock held: the only other large allocations of a well-behaved node are other samplers')
        const int lock_fd = amt_placement_lock(d->device);
        if (lock_fd >= 0) {
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > state + state / 16 + ((size_t)6 << 30)) {
                float ms[16] = {};
                if (amt_domain_tune(d, tries, ms, false) == AMT_OK) {
                    d->placement_tries = tries;
                    memcpy(d->placement_ms, ms, sizeof ms);
                }
                (void)hipGetLastError();                          // a sampling that could not run costs nothing but itself
            }
            (void)flock(lock_fd, LOCK_UN);
            close(lock_fd);
        }
    }
    return AMT_OK;
}

extern "C" int amt_domain_wrap(amt_domain **out, AMT_SHAPE_SIG, void *const *fields, void *hip_stream)
{
    if (!fields) return amt_fail(AMT_ERR_INVALID_ARG, "amt_domain_wrap needs the %d device pointers", (int)AMT_F_COUNT);
    return amt_domain_make(out, AMT_SHAPE_ARGS, fields, hip_stream);
}

int amt_handle_set_scalars(amt_domain *d, double rdx, double rdy, double dts, double epssm)
{
    d->rdx = rdx; d->rdy = rdy; d->dts = dts; d->epssm = epssm;
    return AMT_OK;
}

int amt_handle_set_variant(amt_domain *d, int variant)
{
    if (variant < AMT_VARIANT_AUTO || variant > AMT_VARIANT_MARCH)
        return amt_fail(AMT_ERR_INVALID_ARG, "unknown variant %d", variant);
    d->variant = variant;
    return AMT_OK;
}

int amt_handle_copy(amt_domain *d, void *dev, void *host, size_t bytes, bool up)
{
    DeviceScope scope(d->device);
    if (up) AMT_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, d->stream));
    else AMT_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, d->stream));
    AMT_HIP(hipStreamSynchronize(d->stream));
    return AMT_OK;
}

int amt_handle_fill(amt_domain *d, int members, uint64_t field_mask, uint64_t seed,
                    long gi0, long gk0, long gj0, long gidim, long gkdim, long gjdim)
{
    DeviceScope scope(d->device);
    const long idim = d->ime - d->ims + 1, kdim = d->kme - d->kms + 1, jdim = d->jme - d->jms + 1;
    for (int f = 0; f < AMT_F_COUNT; ++f) {
        if (!(field_mask & AMT_FIELD_BIT(f))) continue;
        const size_t bytes = d->count(f) * (size_t)d->dtype_bytes;
        for (int m = 0; m < (amt_field_rank(f) == 1 ? 1 : members); ++m) {       // the vertical metrics do not depend on the seed
            int rc = amt_synth_fill_device(d->stream, f, d->dtype_bytes, static_cast<char *>(d->field[f]) + (size_t)m * bytes,
                                           seed + (uint64_t)m, idim, kdim, jdim, gi0, gk0, gj0, gidim, gkdim, gjdim);
            if (rc) return rc;
        }
    }
    return AMT_OK;
}

static int amt_null_domain() { return amt_fail(AMT_ERR_INVALID_ARG, "null domain"); }

extern "C" int amt_domain_set_scalars(amt_domain *d, double rdx, double rdy, double dts, double epssm)
{
    return d ? amt_handle_set_scalars(d, rdx, rdy, dts, epssm) : amt_null_domain();
}

extern "C" int amt_domain_set_variant(amt_domain *d, int variant)
{
    return d ? amt_handle_set_variant(d, variant) : amt_null_domain();
}

extern "C" int amt_domain_upload(amt_domain *d, int field, const void *host)
{
    if (!d || !host || field < 0 || field >= AMT_F_COUNT) return amt_fail(AMT_ERR_INVALID_ARG, "bad upload argument");
    return amt_handle_copy(d, d->field[field], const_cast<void *>(host), d->count(field) * d->dtype_bytes, true);
}

extern "C" int amt_domain_download(amt_domain *d, int field, void *host)
{
    if (!d || !host || field < 0 || field >= AMT_F_COUNT) return amt_fail(AMT_ERR_INVALID_ARG, "bad download argument");
    return amt_handle_copy(d, d->field[field], host, d->count(field) * d->dtype_bytes, false);
}

// rows j_lo..j_hi (Fortran indices, inside jms:jme) of a rank-3 or rank-2 field: contiguous in the
// (i,k,j) layout, so one copy each; `host` holds just those rows.  Synchronous.
static int amt_domain_copy_rows(amt_domain *d, int field, int j_lo, int j_hi, void *host, bool up)
{
    if (!d || !host || field < 0 || field >= AMT_F_COUNT) return amt_fail(AMT_ERR_INVALID_ARG, "bad row-copy argument");
    const int rank = amt_field_rank(field);
    if (rank == 1) return amt_fail(AMT_ERR_INVALID_ARG, "field %d has no j rows", field);
    if (j_lo < d->jms || j_hi > d->jme || j_hi < j_lo)
        return amt_fail(AMT_ERR_PRECONDITION, "rows %d:%d not inside memory jms:jme=%d:%d", j_lo, j_hi, d->jms, d->jme);
    const size_t idim = d->ime - d->ims + 1, kdim = d->kme - d->kms + 1;
    const size_t row = (rank == 3 ? idim * kdim : idim) * (size_t)d->dtype_bytes;
    char *dev = static_cast<char *>(d->field[field]) + (size_t)(j_lo - d->jms) * row;
    return amt_handle_copy(d, dev, host, (size_t)(j_hi - j_lo + 1) * row, up);
}

extern "C" int amt_domain_upload_rows(amt_domain *d, int field, int j_lo, int j_hi, const void *host)
{
    return amt_domain_copy_rows(d, field, j_lo, j_hi, const_cast<void *>(host), true);
}

extern "C" int amt_domain_download_rows(amt_domain *d, int field, int j_lo, int j_hi, void *host)
{
    return amt_domain_copy_rows(d, field, j_lo, j_hi, host, false);
}

extern "C" int amt_domain_fill_synthetic(amt_domain *d, uint64_t seed,
                                         long gi0, long gk0, long gj0, long gidim, long gkdim, long gjdim)
{
    return d ? amt_handle_fill(d, 1, ~0ull, seed, gi0, gk0, gj0, gidim, gkdim, gjdim) : amt_null_domain();
}

extern "C" int amt_domain_fill_fields(amt_domain *d, uint64_t field_mask, uint64_t seed,
                                      long gi0, long gk0, long gj0, long gidim, long gkdim, long gjdim)
{
    if (!d) return amt_null_domain();
    if (field_mask >> AMT_F_COUNT) return amt_fail(AMT_ERR_INVALID_ARG, "field mask names a field beyond AMT_F_COUNT");
    return amt_handle_fill(d, 1, field_mask, seed, gi0, gk0, gj0, gidim, gkdim, gjdim);
}

// NaN into up to twelve strided runs in one launch: job q = `count` elements from `base` at stride `stride` (a row of the
// (i,k,j) layout: stride 1; a column: stride idim)
namespace {
template <typename W>
struct AmtPoisonJobs {
    W *base[12];
    long count[12], stride[12];
    W nan;
    int n;
};
template <typename W>
__global__ __launch_bounds__(256) void amt_poison_kernel(AmtPoisonJobs<W> jobs)
{
    const int q = blockIdx.y;
    W *p = jobs.base[q];
    const long n = jobs.count[q], stride = jobs.stride[q];
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) p[e * stride] = jobs.nan;
}

template <typename W>
int amt_domain_poison_t(amt_domain *d, int sides, W nan)
{
    const long idim = d->ime - d->ims + 1, kdim = d->kme - d->kms + 1, jdim = d->jme - d->jms + 1;
    AmtPoisonJobs<W> jobs{};
    jobs.nan = nan;
    if ((sides & (AMT_SIDE_BELOW | AMT_SIDE_ABOVE)) && (d->jts - 1 < d->jms || d->jte + 1 > d->jme))
        return amt_fail(AMT_ERR_PRECONDITION, "amt_domain_poison_halos: the patch holds no halo row below jts / above jte");
    if ((sides & (AMT_SIDE_LEFT | AMT_SIDE_RIGHT)) && (d->its - 1 < d->ims || d->ite + 1 > d->ime))
        return amt_fail(AMT_ERR_PRECONDITION, "amt_domain_poison_halos: the patch holds no halo column left of its / right of ite");
    // the halo cells of amt_halo.h's table: a whole memory row jts-1 / jte+1, a whole memory column its-1 / ite+1
    const int cell[AMT_HALO_SIDES] = {d->jts - 1, d->jte + 1, d->its - 1, d->ite + 1};
    for (int side = 0; side < AMT_HALO_SIDES; ++side) {
        if (!(sides & (1 << side))) continue;
        const bool column = amt_halo_is_column(side);
        for (int k = 0; k < amt_halo_recv(side).n; ++k) {
            const int f = amt_halo_recv(side).field[k], q = jobs.n++;
            const long levels = amt_halo_levels(f, kdim);
            jobs.base[q] = static_cast<W *>(d->field[f]) + (column ? amt_halo_at(*d, f, cell[side], d->jms) : amt_halo_at(*d, f, d->ims, cell[side]));
            jobs.count[q] = levels * (column ? jdim : idim);
            jobs.stride[q] = column ? idim : 1;
        }
    }
    if (jobs.n == 0) return AMT_OK;
    long most = 0;
    for (int q = 0; q < jobs.n; ++q) most = jobs.count[q] > most ? jobs.count[q] : most;
    long blocks = (most + 255) / 256;
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(amt_poison_kernel<W>, dim3((unsigned)blocks, (unsigned)jobs.n), dim3(256), 0, d->stream, jobs);
    AMT_HIP(hipGetLastError());
    return AMT_OK;
}
}  // namespace

extern "C" int amt_domain_poison_halos(amt_domain *d, int sides)
{
    if (!d || (sides & ~15)) return amt_fail(AMT_ERR_INVALID_ARG, "bad poison argument");
    DeviceScope scope(d->device);
    return d->dtype_bytes == 8 ? amt_domain_poison_t<uint64_t>(d, sides, 0x7ff8000000000000ull)
                               : amt_domain_poison_t<uint32_t>(d, sides, 0x7fc00000u);
}

// ---------------------------------------------------------------------------
// The sweep sequence of a resident handle (amt_internal.h): what amt_domain_step and amt_ensemble_step enqueue.
// ---------------------------------------------------------------------------
int amt_handle_behind_sweep(const char *who, amt_domain *d, int members)
{
    // specified / nested boundaries: the boundary zone is advanced behind the sweep, where WRF has its spec_bdyupdate calls
    const int rc = d->spec_bdy ? amt_bdy_update_domain(who, d, members) : AMT_OK;
    // the acoustic loop's flux averages: one accumulation behind the boundary-zone update, where WRF has its sumflux call
    const int rc2 = rc == AMT_OK && d->sumflux_n ? amt_sumflux_accumulate_domain(who, d, members) : rc;
    // the pressure diagnosis closes the sub-step, where WRF has its calc_p_rho call: step != 0, the damping reads pm1
    return rc2 == AMT_OK && d->p_rho_per_sweep ? amt_p_rho_domain(who, d, members, 1) : rc2;
}

namespace {
template <typename T>
int handle_step_t(const char *who, amt_domain *d, int members, bool stacked, int n_sweeps)
{
    AmtArgs<T> a;
    amt_domain_args<T>(d, a);
    // an armed guard that already shows a finding: nothing is enqueued (no wait: the record is in host memory)
    if (d->guard_every) { const int rc = amt_diag_guard_status(who, d); if (rc) return rc; }
    for (int s = 0; s < n_sweeps; ++s) {
        // the momentum update opens the sub-step, where WRF has its advance_uv call: u and v are final behind it
        int rc = d->uv_per_sweep ? amt_uv_domain(who, d, members) : AMT_OK;
        // cyclic boundaries: the wrap cells are refreshed in front of every sweep, on the same stream (the inputs are final there)
        if (rc == AMT_OK && d->cyclic) rc = amt_cyclic_refresh_domain(who, d, d->cyclic, members);
        // every member in one launch; a domain takes the single-patch launch, an ensemble the stacked one also for one member
        if (rc == AMT_OK)
            rc = stacked ? amt_device_call_ensemble<T>(d->stream, d->variant, members, a)
                         : amt_device_call<T>(d->stream, d->variant, a);
        if (rc == AMT_OK) rc = amt_handle_behind_sweep(who, d, members);
        if (rc == AMT_OK && d->guard_every) rc = amt_diag_after_sweep(who, d, members);
        if (rc) return rc;
    }
    return AMT_OK;
}

// Sweeps that are scaffolding (the placement sampling's timed ones): an armed non-finite guard neither checks nor counts them
// (and does not stretch them), nor does the boundary-zone update follow them, nor a flux accumulation (its counter and
// accumulators stay as they are), nor a pressure diagnosis.  The settings of the sequence above that such sweeps must not see are saved and restored here.
struct StepExtrasPause {
    amt_domain *d;
    int every, spec_bdy, sumflux_n, p_rho_per_sweep, uv_per_sweep;
    explicit StepExtrasPause(amt_domain *dom)
        : d(dom), every(dom->guard_every), spec_bdy(dom->spec_bdy), sumflux_n(dom->sumflux_n), p_rho_per_sweep(dom->p_rho_per_sweep),
          uv_per_sweep(dom->uv_per_sweep)
    {
        d->guard_every = 0; d->spec_bdy = 0; d->sumflux_n = 0; d->p_rho_per_sweep = 0; d->uv_per_sweep = 0;
    }
    ~StepExtrasPause()
    {
        d->guard_every = every; d->spec_bdy = spec_bdy; d->sumflux_n = sumflux_n; d->p_rho_per_sweep = p_rho_per_sweep; d->uv_per_sweep = uv_per_sweep;
    }
};
}  // namespace

int amt_handle_step(const char *who, amt_domain *d, int members, bool stacked, int n_sweeps)
{
    DeviceScope scope(d->device);
    return d->dtype_bytes == 8 ? handle_step_t<double>(who, d, members, stacked, n_sweeps)
                               : handle_step_t<float>(who, d, members, stacked, n_sweeps);
}

int amt_handle_step_timed(const char *who_step, const char *who, amt_domain *d, int members, bool stacked, int n_sweeps,
                          float *ms_total)
{
    DeviceScope scope(d->device);
    AMT_HIP(hipEventRecord(d->ev0, d->stream));
    int rc = amt_handle_step(who_step, d, members, stacked, n_sweeps);
    if (rc) return rc;
    AMT_HIP(hipEventRecord(d->ev1, d->stream));
    AMT_HIP(hipEventSynchronize(d->ev1));
    float ms = 0.f;
    AMT_HIP(hipEventElapsedTime(&ms, d->ev0, d->ev1));
    if (ms_total) *ms_total = ms;
    return d->guard_every ? amt_diag_guard_status(who, d) : AMT_OK;
}

int amt_handle_sync(const char *who, amt_domain *d)
{
    DeviceScope scope(d->device);
    AMT_HIP(hipStreamSynchronize(d->stream));
    return d->guard_every ? amt_diag_guard_status(who, d) : AMT_OK;
}

int amt_handle_cyclic_fill(const char *who, amt_domain *d, int members, int axes)
{
    DeviceScope scope(d->device);
    return amt_cyclic_refresh_domain(who, d, axes, members);
}

int amt_handle_set_cyclic(const char *who, amt_domain *d, int members, int axes)
{
    const int rc = amt_cyclic_check_domain(who, d, axes, members);
    if (rc == AMT_OK) d->cyclic = axes;
    return rc;
}

int amt_handle_spec_bdy_update(const char *who, amt_domain *d, int members)
{
    DeviceScope scope(d->device);
    return amt_bdy_update_domain(who, d, members);
}

int amt_handle_set_spec_bdy(const char *who, amt_domain *d, int members, int on)
{
    const int rc = on ? amt_bdy_check_domain(who, d, members) : AMT_OK;
    if (rc == AMT_OK) d->spec_bdy = on ? 1 : 0;
    return rc;
}

void *amt_handle_field_ptr(amt_domain *d, int field) { return field < 0 || field >= AMT_F_COUNT ? nullptr : d->field[field]; }

// The bracket of a Runge-Kutta stage (header section 15): prep in front of a stage's acoustic loop, finish behind it, on the
// handle's stream.  Not a per-sweep setting: the sweep sequence above does not know of it.  The refusals of amt_stage.hip come
// back before the first device call; the device is made current behind them.
int amt_handle_set_stage(const char *who, amt_domain *d, int members, int on, void *t_old, void *mu_old, void *mu_save, void *mub)
{
    return amt_stage_set_domain(who, d, members, on, t_old, mu_old, mu_save, mub);
}

void *amt_handle_stage_ptr(amt_domain *d, int which) { return which < 0 || which > 3 ? nullptr : d->stage_arr[which]; }

int amt_handle_stage_prep(const char *who, amt_domain *d, int members, int rk_step)
{
    return amt_stage_prep_domain(who, d, members, rk_step);
}

int amt_handle_stage_finish(const char *who, amt_domain *d, int members, int n_small_steps, const void *h_diabatic)
{
    return amt_stage_finish_domain(who, d, members, n_small_steps, h_diabatic);
}

// The pressure diagnosis that closes an acoustic sub-step (header section 16).  With per_sweep it is a line of the sweep
// sequence above (amt_handle_behind_sweep); amt_handle_p_rho is the step = 0 call behind small_step_prep, or any other.  The
// refusals of amt_p_rho.hip come back before the first device call.
int amt_handle_set_p_rho(const char *who, amt_domain *d, int members, int mode, int per_sweep, double t0, double smdiv,
                         void *al, void *p, void *ph, void *pm1, void *alt, void *c2a, void *znu, void *dnw)
{
    void *const arr[8] = {al, p, ph, pm1, alt, c2a, znu, dnw};
    return amt_p_rho_set_domain(who, d, members, mode, per_sweep, t0, smdiv, arr);
}

void *amt_handle_p_rho_ptr(amt_domain *d, int which) { return which < 0 || which > 7 ? nullptr : d->p_rho_arr[which]; }

int amt_handle_p_rho(const char *who, amt_domain *d, int members, int step) { return amt_p_rho_domain(who, d, members, step); }

// The momentum update that opens an acoustic sub-step (header section 17): with per_sweep a line of the sweep sequence above.
int amt_handle_set_uv(const char *who, amt_domain *d, int members, int on, int per_sweep, double emdiv, double cf1, double cf2, double cf3,
                      void *const arr[9])
{
    return amt_uv_set_domain(who, d, members, on, per_sweep, emdiv, cf1, cf2, cf3, arr);
}

void *amt_handle_uv_ptr(amt_domain *d, int which) { return which < 0 || which > 8 ? nullptr : d->uv_arr[which]; }

int amt_handle_uv(const char *who, amt_domain *d, int members) { return amt_uv_domain(who, d, members); }

extern "C" int amt_domain_cyclic_fill(amt_domain *d, int axes)
{
    return d ? amt_handle_cyclic_fill("amt_domain_cyclic_fill", d, 1, axes) : amt_null_domain();
}
extern "C" int amt_domain_set_cyclic(amt_domain *d, int axes)
{
    return d ? amt_handle_set_cyclic("amt_domain_set_cyclic", d, 1, axes) : amt_null_domain();
}
extern "C" int amt_domain_cyclic(const amt_domain *d) { return d ? d->cyclic : 0; }
extern "C" int amt_domain_spec_bdy_update(amt_domain *d)
{
    return d ? amt_handle_spec_bdy_update("amt_domain_spec_bdy_update", d, 1) : amt_null_domain();
}
extern "C" int amt_domain_set_spec_bdy(amt_domain *d, int on)
{
    return d ? amt_handle_set_spec_bdy("amt_domain_set_spec_bdy", d, 1, on) : amt_null_domain();
}
extern "C" int amt_domain_spec_bdy(const amt_domain *d) { return d ? d->spec_bdy : 0; }

extern "C" int amt_domain_set_stage(amt_domain *d, int on, void *t_old, void *mu_old, void *mu_save, void *mub)
{
    return d ? amt_handle_set_stage("amt_domain_set_stage", d, 1, on, t_old, mu_old, mu_save, mub) : amt_null_domain();
}
extern "C" void *amt_domain_stage_ptr(amt_domain *d, int which) { return d ? amt_handle_stage_ptr(d, which) : nullptr; }
extern "C" int amt_domain_stage_prep(amt_domain *d, int rk_step)
{
    return d ? amt_handle_stage_prep("amt_domain_stage_prep", d, 1, rk_step) : amt_null_domain();
}
extern "C" int amt_domain_stage_finish(amt_domain *d, int n_small_steps, const void *h_diabatic)
{
    return d ? amt_handle_stage_finish("amt_domain_stage_finish", d, 1, n_small_steps, h_diabatic) : amt_null_domain();
}

extern "C" int amt_domain_set_p_rho(amt_domain *d, int mode, int per_sweep, double t0, double smdiv, void *al, void *p, void *ph,
                                   void *pm1, void *alt, void *c2a, void *znu, void *dnw)
{
    return d ? amt_handle_set_p_rho("amt_domain_set_p_rho", d, 1, mode, per_sweep, t0, smdiv, al, p, ph, pm1, alt, c2a, znu, dnw)
             : amt_null_domain();
}
extern "C" int amt_domain_set_uv(amt_domain *d, int on, int per_sweep, double emdiv, double cf1, double cf2, double cf3, void *ru_tend,
                                void *rv_tend, void *pb, void *php, void *cqu, void *cqv, void *msfux, void *msfvx, void *msfvy)
{
    void *const arr[9] = {ru_tend, rv_tend, pb, php, cqu, cqv, msfux, msfvx, msfvy};
    return d ? amt_handle_set_uv("amt_domain_set_uv", d, 1, on, per_sweep, emdiv, cf1, cf2, cf3, arr) : amt_null_domain();
}
extern "C" void *amt_domain_uv_ptr(amt_domain *d, int which) { return d ? amt_handle_uv_ptr(d, which) : nullptr; }
extern "C" int amt_domain_uv(amt_domain *d) { return d ? amt_handle_uv("amt_domain_uv", d, 1) : amt_null_domain(); }
extern "C" void *amt_domain_p_rho_ptr(amt_domain *d, int which) { return d ? amt_handle_p_rho_ptr(d, which) : nullptr; }
extern "C" int amt_domain_p_rho(amt_domain *d, int step)
{
    return d ? amt_handle_p_rho("amt_domain_p_rho", d, 1, step) : amt_null_domain();
}

extern "C" int amt_domain_step(amt_domain *d, int n_sweeps)
{
    if (!d || n_sweeps < 0) return amt_fail(AMT_ERR_INVALID_ARG, "bad step argument");
    return amt_handle_step("amt_domain_step", d, 1, false, n_sweeps);
}

extern "C" int amt_domain_step_timed(amt_domain *d, int n_sweeps, float *ms_total)
{
    if (!d || n_sweeps < 0) return amt_fail(AMT_ERR_INVALID_ARG, "bad step argument");
    return amt_handle_step_timed("amt_domain_step", "amt_domain_step_timed", d, 1, false, n_sweeps, ms_total);
}

// Placement tuning.  Where the driver puts an array's pages moves the sweep by up to +-3 % (same kernel, same virtual
// layout, fresh physical pages: profiles/r03_placement.md); nothing below the page size matters, so it cannot be steered --
// only sampled.  This samples it for the handle's own arrays: `tries` allocations of the whole state one after the other (at
// most two resident at a time), the current contents copied over, one warm-up and two timed sweeps of the handle's own
// kernel on each, the fastest kept.  The contents of every array are what they were before the call (the in/out and output
// arrays the timed sweeps advanced are restored from a copy).  bench.py does the same with its torch-owned arrays
// (--probe-placements); a C / Fortran host gets the same memory this way.
// preserve = false (amt_domain_create: the arrays hold nothing yet): no copies at all, the candidates are timed as allocated
static int amt_domain_tune(amt_domain *d, int tries, float *ms_per_try, bool preserve)
{
    DeviceScope scope(d->device);
    StepExtrasPause pause(d);                                     // the timed sweeps are scaffolding
    auto bytes = [&](int f) { return d->count(f) * (size_t)d->dtype_bytes; };
    auto time_current = [&](float *ms) -> int {
        int rc = amt_domain_step(d, 1);
        if (rc) return rc;
        AMT_HIP(hipEventRecord(d->ev0, d->stream));
        rc = amt_domain_step(d, 2);
        if (rc) return rc;
        AMT_HIP(hipEventRecord(d->ev1, d->stream));
        AMT_HIP(hipEventSynchronize(d->ev1));
        AMT_HIP(hipEventElapsedTime(ms, d->ev0, d->ev1));
        *ms *= 0.5f;
        return AMT_OK;
    };
    for (int k = 0; k < tries && ms_per_try; ++k) ms_per_try[k] = 0.f;
    // what the timed sweeps overwrite, kept aside
    void *keep[AMT_F_COUNT] = {};
    auto free_set = [](void **set) { for (int f = 0; f < AMT_F_COUNT; ++f) if (set[f]) { (void)hipFree(set[f]); set[f] = nullptr; } };
    hipError_t copy_err = hipSuccess;
    auto note = [&](hipError_t e) { if (e != hipSuccess && copy_err == hipSuccess) copy_err = e; };
    for (int f = 0; f < AMT_F_COUNT && preserve; ++f) {
        if (!kAmtField[f].out) continue;                          // what the timed sweeps overwrite: the fields the routine assigns
        if (hipMalloc(&keep[f], bytes(f)) != hipSuccess) {
            (void)hipGetLastError();
            free_set(keep);
            return amt_fail(AMT_ERR_ALLOC, "amt_domain_tune_placement: no room for a copy of the output arrays (nothing changed)");
        }
        note(hipMemcpyAsync(keep[f], d->field[f], bytes(f), hipMemcpyDeviceToDevice, d->stream));
    }
    note(hipStreamSynchronize(d->stream));
    if (copy_err != hipSuccess) {                                 // nothing was changed yet
        free_set(keep);
        return amt_fail(AMT_ERR_HIP, "amt_domain_tune_placement: saving the output arrays failed: %s", hipGetErrorString(copy_err));
    }
    float best = 0.f;
    int rc = time_current(&best);
    if (ms_per_try) ms_per_try[0] = best;
    for (int k = 1; k < tries && rc == AMT_OK; ++k) {
        void *spacer = nullptr;                                   // shifts what the next allocations get
        if (hipMalloc(&spacer, ((size_t)k * 1237 + 311) << 20) != hipSuccess) { (void)hipGetLastError(); spacer = nullptr; }
        void *cand[AMT_F_COUNT] = {};
        bool ok = true;
        for (int f = 0; f < AMT_F_COUNT && ok; ++f) ok = hipMalloc(&cand[f], bytes(f)) == hipSuccess;
        if (spacer) (void)hipFree(spacer);
        if (!ok) {                                                // a second copy of the state does not fit: keep what we have
            (void)hipGetLastError();
            free_set(cand);
            break;
        }
        hipError_t ce = hipSuccess;
        for (int f = 0; f < AMT_F_COUNT && ce == hipSuccess && preserve; ++f) {
            const bool mut = keep[f] != nullptr;
            ce = hipMemcpyAsync(cand[f], mut ? keep[f] : d->field[f], bytes(f), hipMemcpyDeviceToDevice, d->stream);
        }
        if (ce == hipSuccess) ce = hipStreamSynchronize(d->stream);
        if (ce != hipSuccess) {                                   // a candidate with unknown contents is neither timed nor kept
            (void)hipGetLastError();
            free_set(cand);
            continue;
        }
        void *cur[AMT_F_COUNT];
        memcpy(cur, d->field, sizeof cur);
        memcpy(d->field, cand, sizeof cand);
        float ms = 0.f;
        rc = time_current(&ms);
        if (ms_per_try) ms_per_try[k] = ms;
        if (rc == AMT_OK && ms < best) {
            best = ms;
            free_set(cur);                                        // the candidate stays
        } else {
            memcpy(d->field, cur, sizeof cur);
            free_set(cand);
        }
    }
    for (int f = 0; f < AMT_F_COUNT; ++f)                         // contents as they were before the call
        if (keep[f]) note(hipMemcpyAsync(d->field[f], keep[f], bytes(f), hipMemcpyDeviceToDevice, d->stream));
    note(hipStreamSynchronize(d->stream));
    free_set(keep);
    if (copy_err != hipSuccess)
        return amt_fail(AMT_ERR_HIP, "amt_domain_tune_placement: restoring the output arrays failed: %s (their contents are undefined)", hipGetErrorString(copy_err));
    return rc;
}

extern "C" int amt_domain_tune_placement(amt_domain *d, int tries, float *ms_per_try)
{
    if (!d || tries < 1) return amt_fail(AMT_ERR_INVALID_ARG, "bad tuning argument");
    if (!d->owns_fields) return amt_fail(AMT_ERR_INVALID_ARG, "amt_domain_tune_placement: the arrays belong to the caller (amt_domain_wrap)");
    float ms[16] = {};
    if (tries > 16) tries = 16;
    const int rc = amt_domain_tune(d, tries, ms, true);
    d->placement_tries = tries;
    memcpy(d->placement_ms, ms, sizeof ms);
    for (int k = 0; k < tries && ms_per_try; ++k) ms_per_try[k] = ms[k];
    return rc;
}

extern "C" int amt_domain_placement(const amt_domain *d, float *ms_per_try, int cap)
{
    if (!d) return 0;
    for (int k = 0; k < d->placement_tries && k < cap && ms_per_try; ++k) ms_per_try[k] = d->placement_ms[k];
    return d->placement_tries;
}

extern "C" int amt_domain_sync(amt_domain *d) { return d ? amt_handle_sync("amt_domain_sync", d) : amt_null_domain(); }
extern "C" void *amt_domain_field_ptr(amt_domain *d, int field) { return d ? amt_handle_field_ptr(d, field) : nullptr; }
extern "C" void *amt_domain_stream(amt_domain *d) { return d ? (void *)d->stream : nullptr; }
