// amt_api.hip -- core of the C-ABI of include/amt_advance_mu_t.h: errors, the bounds logic and
// index normalisation (the job of advance_mu_t_no_async.cu:57-85 in the reference), the
// device-resident entry points, the synthetic-input fill and the calibration copy.  The one-shot
// host drop-in is amt_oneshot.hip, the resident handle amt_domain.hip, the grid and slab steppers
// amt_grid.hip.  There is deliberately no CPU compute path anywhere.
#include "amt_internal.h"
#include <atomic>

template <typename T> hipError_t amt_launch_column(hipStream_t, const AmtParams<T> &);
template <typename T> hipError_t amt_launch_march(hipStream_t, const AmtParams<T> &);
template <typename T> bool amt_march_supported(const AmtParams<T> &);
void amt_march_note_kernel(const char *name);

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local std::string g_last_error;

int amt_fail(int status, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return status;
}

extern "C" const char *amt_version(void) { return "amt-advance_mu_t 0.1 (gfx950)"; }

extern "C" const char *amt_status_string(int s)
{
    switch (s) {
    case AMT_OK: return "ok";
    case AMT_ERR_HIP: return "HIP runtime error";
    case AMT_ERR_PRECONDITION: return "bounds violate the preconditions of advance_mu_t";
    case AMT_ERR_INVALID_ARG: return "invalid argument";
    case AMT_ERR_NO_DEVICE: return "no HIP device";
    case AMT_ERR_ALLOC: return "allocation failed";
    case AMT_ERR_COMM: return "RCCL error";
    case AMT_ERR_NONFINITE: return "the non-finite guard found a NaN or Inf in ww, t or mu";
    default: return "unknown status";
    }
}

extern "C" const char *amt_last_error(void) { return g_last_error.c_str(); }

extern "C" int amt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

extern "C" int amt_compute_window(int periodic_x, int specified, int nested,
                                  int ids, int ide, int jds, int jde,
                                  int its, int ite, int jts, int jte, int kts, int kte,
                                  int *i_start, int *i_end, int *j_start, int *j_end,
                                  int *k_start, int *k_end)
{
    const AmtWindow w = amt_window(periodic_x, specified, nested, ids, ide, jds, jde,
                                   its, ite, jts, jte, kts, kte);
    if (i_start) *i_start = w.i_start;
    if (i_end) *i_end = w.i_end;
    if (j_start) *j_start = w.j_start;
    if (j_end) *j_end = w.j_end;
    if (k_start) *k_start = w.k_start;
    if (k_end) *k_end = w.k_end;
    return AMT_OK;
}

// Checks the preconditions and rebases the Fortran bounds to memory-relative
// zero-based ones (cf. advance_mu_t_no_async.cu:57-85).  *empty is set when the
// compute window holds no column (then nothing may be dereferenced).
template <typename T>
int amt_build_params(const AmtArgs<T> &a, AmtParams<T> &p, AmtWindow &w, bool *empty)
{
    w = amt_window(a.periodic_x, a.specified, a.nested, a.ids, a.ide, a.jds, a.jde,
                   a.its, a.ite, a.jts, a.jte, a.kts, a.kte);
    *empty = (w.i_end < w.i_start) || (w.j_end < w.j_start);
    if (a.ime < a.ims || a.jme < a.jms || a.kme < a.kms)
        return amt_fail(AMT_ERR_PRECONDITION, "empty memory extents");
    if (a.kts != 1 || a.kte != a.kde)
        return amt_fail(AMT_ERR_PRECONDITION,
                        "need kts == 1 and kte == kde (got kts=%d kte=%d kde=%d): the Fortran "
                        "uses literal levels 1,2 and wdtn(kde) (module_small_step_em.f90:159,168,221)",
                        a.kts, a.kte, a.kde);
    if (a.kms > 1 || a.kme < a.kte)
        return amt_fail(AMT_ERR_PRECONDITION, "levels 1..kte=%d not inside memory kms:kme=%d:%d",
                        a.kte, a.kms, a.kme);
    if (*empty) return AMT_OK;
    if (w.i_start - 1 < a.ims || w.i_end + 1 > a.ime)
        return amt_fail(AMT_ERR_PRECONDITION,
                        "i window %d:%d plus halo not inside memory ims:ime=%d:%d",
                        w.i_start, w.i_end, a.ims, a.ime);
    if (w.j_start - 1 < a.jms || w.j_end + 1 > a.jme)
        return amt_fail(AMT_ERR_PRECONDITION,
                        "j window %d:%d plus halo not inside memory jms:jme=%d:%d",
                        w.j_start, w.j_end, a.jms, a.jme);
    const T *ptrs[AMT_F_COUNT];
    amt_args_get_fields(a, ptrs);
    for (const T *q : ptrs)
        if (!q) return amt_fail(AMT_ERR_INVALID_ARG, "null array pointer");

#define AMT_FIELD_PARAM(ID, member, in, out) p.member = a.member;
    AMT_FIELDS(AMT_FIELD_PARAM)
#undef AMT_FIELD_PARAM
    p.rdx = a.rdx; p.rdy = a.rdy; p.dts = a.dts; p.epssm = a.epssm;
    p.idim = a.ime - a.ims + 1;
    p.kdim = a.kme - a.kms + 1;
    p.jstride = (long)p.idim * p.kdim;
    p.i0 = w.i_start - a.ims; p.i1 = w.i_end - a.ims;
    p.j0 = w.j_start - a.jms; p.j1 = w.j_end - a.jms;
    p.k1 = 1 - a.kms;
    p.nk = w.k_end;            // levels 1..k_end (k_end may be 0)
    p.edges = 0;
    p.members = 0;             // a single patch; amt_device_call_ensemble sets the member count
    p.jdim = a.jme - a.jms + 1;
    return AMT_OK;
}

template <typename T>
static int amt_launch(hipStream_t stream, int variant, const AmtParams<T> &p)
{
    if (variant == AMT_VARIANT_AUTO) {
        variant = amt_march_supported(p) ? AMT_VARIANT_MARCH : AMT_VARIANT_COLUMN;
        // fp32 beyond 264 levels: the only march shapes left are the one-column-per-lane register builds (<float,1,8,4,...>: 0.29-0.31
        // of the HBM roofline), which the column kernel's recompute flavour beats (0.41; profiles/r06_tall_columns.md)
        if (sizeof(T) == 4 && p.nk > 264) variant = AMT_VARIANT_COLUMN;
        if (variant == AMT_VARIANT_COLUMN && p.nk > (sizeof(T) == 8 ? 240 : 264)) {
            // the speed step of the header (beyond 240 levels in fp64 / 264 in fp32 the march kernel's tile no longer fits the LDS):
            // said once per process on stderr, never silently (AMT_QUIET=1 to suppress)
            static std::atomic<bool> said{false};
            if (!said.exchange(true) && !getenv("AMT_QUIET"))
                fprintf(stderr, "amt: advance_mu_t with %d levels runs on the column kernel (about 0.41 of the HBM roofline against 0.61-0.75 for "
                                "the march kernel, which holds at most 240 levels in fp64 / 264 in fp32); see include/amt_advance_mu_t.h, "
                                "\"SPEED CLIFF\"\n", p.nk);
        }
    }
    hipError_t e;
    if (variant == AMT_VARIANT_COLUMN) {
        if ((size_t)p.nk * 64 * sizeof(T) > 160 * 1024)
            return amt_fail(AMT_ERR_PRECONDITION, "nk=%d: no kernel holds a column of more than %d levels in LDS",
                            p.nk, (int)(160 * 1024 / (64 * sizeof(T))));
        e = amt_launch_column<T>(stream, p);
        amt_march_note_kernel(sizeof(T) == 8 ? "amt_column_kernel<double>" : "amt_column_kernel<float>");
    } else if (variant == AMT_VARIANT_MARCH) {
        if (!amt_march_supported(p))
            return amt_fail(AMT_ERR_INVALID_ARG, "AMT_VARIANT_MARCH does not support nk=%d", p.nk);
        e = amt_launch_march<T>(stream, p);
    } else {
        return amt_fail(AMT_ERR_INVALID_ARG, "unknown variant %d", variant);
    }
    if (e != hipSuccess)
        return amt_fail(e == hipErrorNoDevice ? AMT_ERR_NO_DEVICE : AMT_ERR_HIP,
                        "kernel launch failed: %s", hipGetErrorString(e));
    return AMT_OK;
}

// Only the first and the last row of the tile's window (amt_grid.hip: the two rows of a j-slab that
// read a neighbour's halo), in one launch where the march kernel runs, in two otherwise.
template <typename T>
int amt_device_call_edges(void *hip_stream, int variant, const AmtArgs<T> &a)
{
    AmtParams<T> p;
    AmtWindow w;
    bool empty = false;
    int rc = amt_build_params(a, p, w, &empty);
    if (rc != AMT_OK || empty) return rc;
    if (p.j1 == p.j0) return amt_launch<T>(static_cast<hipStream_t>(hip_stream), variant, p);
    p.edges = 1;
    if ((variant == AMT_VARIANT_AUTO || variant == AMT_VARIANT_MARCH) && amt_march_supported(p))
        return amt_launch<T>(static_cast<hipStream_t>(hip_stream), AMT_VARIANT_MARCH, p);
    p.edges = 0;
    AmtParams<T> q = p;
    q.j1 = p.j0;
    rc = amt_launch<T>(static_cast<hipStream_t>(hip_stream), variant, q);
    if (rc != AMT_OK) return rc;
    q.j0 = q.j1 = p.j1;
    return amt_launch<T>(static_cast<hipStream_t>(hip_stream), variant, q);
}

template <typename T>
int amt_device_call(void *hip_stream, int variant, const AmtArgs<T> &a)
{
    AmtParams<T> p;
    AmtWindow w;
    bool empty = false;
    int rc = amt_build_params(a, p, w, &empty);
    if (rc != AMT_OK || empty) return rc;
    return amt_launch<T>(static_cast<hipStream_t>(hip_stream), variant, p);
}

// `members` same-shape patches stacked along one more, slowest, dimension in every 3-D and 2-D array, as one launch
// (amt_ensemble.hip).  Bounds, flags, scalars and the 1-D arrays are those of ONE member.
template <typename T>
int amt_device_call_ensemble(void *hip_stream, int variant, int members, const AmtArgs<T> &a)
{
    if (members < 1) return amt_fail(AMT_ERR_INVALID_ARG, "members = %d: an ensemble has at least one member", members);
    AmtParams<T> p;
    AmtWindow w;
    bool empty = false;
    int rc = amt_build_params(a, p, w, &empty);
    if (rc != AMT_OK || empty) return rc;
    if ((long)members * p.jdim > 0x7fffffffL)
        return amt_fail(AMT_ERR_PRECONDITION, "%d members of %d rows: the stacked arrays have more than 2^31 - 1 rows", members, p.jdim);
    p.members = members;
    return amt_launch<T>(static_cast<hipStream_t>(hip_stream), variant, p);
}

// The same launch when another stream's kernels are to run beside it (amt_grid.hip: the interior rows of a j-slab
// while the halo exchange and the edge rows go through the communication stream).
template <typename T>
int amt_device_call_shared(void *hip_stream, int variant, const AmtArgs<T> &a)
{
    AmtParams<T> p;
    AmtWindow w;
    bool empty = false;
    int rc = amt_build_params(a, p, w, &empty);
    if (rc != AMT_OK || empty) return rc;
    p.edges = 2;
    return amt_launch<T>(static_cast<hipStream_t>(hip_stream), variant, p);
}

template int amt_build_params<float>(const AmtArgs<float> &, AmtParams<float> &, AmtWindow &, bool *);
template int amt_build_params<double>(const AmtArgs<double> &, AmtParams<double> &, AmtWindow &, bool *);
template int amt_device_call<float>(void *, int, const AmtArgs<float> &);
template int amt_device_call<double>(void *, int, const AmtArgs<double> &);
template int amt_device_call_shared<float>(void *, int, const AmtArgs<float> &);
template int amt_device_call_shared<double>(void *, int, const AmtArgs<double> &);
template int amt_device_call_edges<float>(void *, int, const AmtArgs<float> &);
template int amt_device_call_ensemble<float>(void *, int, int, const AmtArgs<float> &);
template int amt_device_call_ensemble<double>(void *, int, int, const AmtArgs<double> &);
template int amt_device_call_edges<double>(void *, int, const AmtArgs<double> &);

extern "C" int amt_advance_mu_t_device_f32(void *hip_stream, int variant, AMT_SIG(float))
{
    AMT_PACK_ARGS(float)
    if (variant & AMT_LAUNCH_BESIDE_OTHERS) return amt_device_call_shared<float>(hip_stream, variant & ~AMT_LAUNCH_BESIDE_OTHERS, a);
    return amt_device_call<float>(hip_stream, variant, a);
}
extern "C" int amt_advance_mu_t_device_f64(void *hip_stream, int variant, AMT_SIG(double))
{
    AMT_PACK_ARGS(double)
    if (variant & AMT_LAUNCH_BESIDE_OTHERS) return amt_device_call_shared<double>(hip_stream, variant & ~AMT_LAUNCH_BESIDE_OTHERS, a);
    return amt_device_call<double>(hip_stream, variant, a);
}

// ---------------------------------------------------------------------------
// (4) synthetic inputs
// ---------------------------------------------------------------------------
template <typename T>
__global__ void amt_synth_fill_kernel(T *dst, int field, uint64_t seed,
                                      long idim, long kdim, long jdim,
                                      long gi0, long gk0, long gj0,
                                      long gidim, long gkdim, long gjdim)
{
    const long n = idim * kdim * jdim;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const long li = e % idim;
        const long lk = (e / idim) % kdim;
        const long lj = e / (idim * kdim);
        dst[e] = (T)amt_synth_value(field, seed, gi0 + li, gk0 + lk, gj0 + lj, gidim, gkdim, gjdim);
    }
}

static int amt_synth_shape(int field, long &idim, long &kdim, long &jdim, long &gi0, long &gk0, long &gj0)
{
    if (field < 0 || field >= AMT_F_COUNT) return amt_fail(AMT_ERR_INVALID_ARG, "bad field id %d", field);
    const int rank = amt_field_rank(field);
    if (rank == 2) { kdim = 1; gk0 = 0; }
    if (rank == 1) { idim = 1; jdim = 1; gi0 = 0; gj0 = 0; }
    if (idim < 0 || kdim < 0 || jdim < 0) return amt_fail(AMT_ERR_INVALID_ARG, "negative extent");
    return AMT_OK;
}

extern "C" int amt_synth_fill_host(int field, int dtype_bytes, void *dst, uint64_t seed,
                                   long idim, long kdim, long jdim,
                                   long gi0, long gk0, long gj0,
                                   long gidim, long gkdim, long gjdim)
{
    int rc = amt_synth_shape(field, idim, kdim, jdim, gi0, gk0, gj0);
    if (rc) return rc;
    if (!dst) return amt_fail(AMT_ERR_INVALID_ARG, "null destination");
    if (dtype_bytes != 4 && dtype_bytes != 8) return amt_fail(AMT_ERR_INVALID_ARG, "dtype_bytes must be 4 or 8");
    long e = 0;
    for (long lj = 0; lj < jdim; ++lj)
        for (long lk = 0; lk < kdim; ++lk)
            for (long li = 0; li < idim; ++li, ++e) {
                const double x = amt_synth_value(field, seed, gi0 + li, gk0 + lk, gj0 + lj, gidim, gkdim, gjdim);
                if (dtype_bytes == 8) static_cast<double *>(dst)[e] = x;
                else static_cast<float *>(dst)[e] = (float)x;
            }
    return AMT_OK;
}

extern "C" int amt_synth_fill_device(void *hip_stream, int field, int dtype_bytes, void *dst,
                                     uint64_t seed, long idim, long kdim, long jdim,
                                     long gi0, long gk0, long gj0,
                                     long gidim, long gkdim, long gjdim)
{
    int rc = amt_synth_shape(field, idim, kdim, jdim, gi0, gk0, gj0);
    if (rc) return rc;
    if (!dst) return amt_fail(AMT_ERR_INVALID_ARG, "null destination");
    if (dtype_bytes != 4 && dtype_bytes != 8) return amt_fail(AMT_ERR_INVALID_ARG, "dtype_bytes must be 4 or 8");
    const long n = idim * kdim * jdim;
    if (n == 0) return AMT_OK;
    long blocks = (n + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (dtype_bytes == 8)
        hipLaunchKernelGGL(amt_synth_fill_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, s,
                           static_cast<double *>(dst), field, seed, idim, kdim, jdim, gi0, gk0, gj0,
                           gidim, gkdim, gjdim);
    else
        hipLaunchKernelGGL(amt_synth_fill_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s,
                           static_cast<float *>(dst), field, seed, idim, kdim, jdim, gi0, gk0, gj0,
                           gidim, gkdim, gjdim);
    AMT_HIP(hipGetLastError());
    return AMT_OK;
}

// ---------------------------------------------------------------------------
// profiling aid: streaming copy with a chosen access width
// ---------------------------------------------------------------------------
template <typename V>
__global__ void amt_calib_copy_kernel(V *dst, const V *src, size_t n)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) dst[e] = src[e];
}

extern "C" int amt_calib_stream_copy(void *hip_stream, void *dst, const void *src, size_t nbytes, int bytes_per_lane)
{
    if (!dst || !src) return amt_fail(AMT_ERR_INVALID_ARG, "null pointer");
    if (bytes_per_lane != 4 && bytes_per_lane != 8 && bytes_per_lane != 16)
        return amt_fail(AMT_ERR_INVALID_ARG, "bytes_per_lane must be 4, 8 or 16");
    if (nbytes % bytes_per_lane) return amt_fail(AMT_ERR_INVALID_ARG, "nbytes not a multiple of the access width");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const size_t n = nbytes / bytes_per_lane;
    if (n == 0) return AMT_OK;
    const unsigned blocks = 256 * 8;
    if (bytes_per_lane == 4)
        hipLaunchKernelGGL(amt_calib_copy_kernel<float>, dim3(blocks), dim3(256), 0, s, (float *)dst, (const float *)src, n);
    else if (bytes_per_lane == 8)
        hipLaunchKernelGGL(amt_calib_copy_kernel<double>, dim3(blocks), dim3(256), 0, s, (double *)dst, (const double *)src, n);
    else
        hipLaunchKernelGGL(amt_calib_copy_kernel<double2>, dim3(blocks), dim3(256), 0, s, (double2 *)dst, (const double2 *)src, n);
    AMT_HIP(hipGetLastError());
    return AMT_OK;
}


// ---------------------------------------------------------------------------
// the box's own streaming ceilings (bench.py: roofline.box_*): a tuned copy and a read-only sweep,
// 16 bytes per lane, several loads in flight per lane, nt policy -- the configurations that measured
// fastest on gfx950 (profiles/vmm_probe.hip: copy 5.65 TB/s with 4 loads in flight and 4096 blocks,
// read-only 6.93 TB/s with 8)
// ---------------------------------------------------------------------------
typedef double amt_v2d __attribute__((ext_vector_type(2)));

template <int U>
__global__ __launch_bounds__(256) void amt_stream_copy_kernel(amt_v2d *dst, const amt_v2d *src, size_t n)
{
    const size_t chunk = (size_t)256 * U;
    for (size_t c = (size_t)blockIdx.x * chunk; c < n; c += (size_t)gridDim.x * chunk) {
        amt_v2d r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t e = c + (size_t)u * 256 + threadIdx.x;
            if (e < n) r[u] = __builtin_nontemporal_load(src + e);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t e = c + (size_t)u * 256 + threadIdx.x;
            if (e < n) __builtin_nontemporal_store(r[u], dst + e);
        }
    }
}

template <int U>
__global__ __launch_bounds__(256) void amt_stream_read_kernel(double *sink, const amt_v2d *src, size_t n)
{
    const size_t chunk = (size_t)256 * U;
    amt_v2d acc = {0, 0};
    for (size_t c = (size_t)blockIdx.x * chunk; c < n; c += (size_t)gridDim.x * chunk) {
        amt_v2d r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t e = c + (size_t)u * 256 + threadIdx.x;
            r[u] = e < n ? __builtin_nontemporal_load(src + e) : amt_v2d{0, 0};
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc += r[u];
    }
    if (acc.x + acc.y == 1.2345e300) sink[0] = acc.x;        // keeps the loads alive; never true for finite data
}

extern "C" int amt_calib_stream_rate(void *hip_stream, void *dst, const void *src, size_t nbytes, int mode)
{
    if (!dst || !src) return amt_fail(AMT_ERR_INVALID_ARG, "null pointer");
    if (nbytes % 16) return amt_fail(AMT_ERR_INVALID_ARG, "nbytes not a multiple of 16");
    if (mode != 0 && mode != 1) return amt_fail(AMT_ERR_INVALID_ARG, "mode must be 0 (copy) or 1 (read only)");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const size_t n = nbytes / 16;
    if (n == 0) return AMT_OK;
    if (mode == 0)
        hipLaunchKernelGGL(amt_stream_copy_kernel<4>, dim3(4096), dim3(256), 0, s, (amt_v2d *)dst, (const amt_v2d *)src, n);
    else
        hipLaunchKernelGGL(amt_stream_read_kernel<8>, dim3(4096), dim3(256), 0, s, (double *)dst, (const amt_v2d *)src, n);
    AMT_HIP(hipGetLastError());
    return AMT_OK;
}
