// amt_moments.hip -- ensemble mean, sample variance and envelope of a member-stacked resident field on the device
// (include/amt_advance_mu_t.h section 13).
//
// For every cell c of a BOX (header section 10) of a field stacked (i,k,j,m), with x_m = a_m[c] in member order:
//   s = double(x_0); s = s + double(x_m), m = 1..M-1;   mean_d = s / double(M);                 mean[c] = T(mean_d)
//   q = 0;  d = double(x_m) - mean_d;  q = q + d * d, m = 0..M-1;   var_d = q / double(max(M-1, 1));   var[c] = T(var_d)
//   lo[c] = the FIRST member that attains the minimum (x_m < lo replaces), hi[c] the same with >; NaN if any x_m is NaN
// Product, then sum: two roundings (the library is built with -ffp-contract=off).  The order is per cell and sequential over
// the members, so a result depends on the box contents alone: no atomics, no tickets, no workspace.
//
// A pure streaming pass: W * M * count bytes read once, W * count written per wanted output.  The box's nk * nj row runs of ni
// contiguous elements are cut into chunks of 16 bytes counted from the run's first element, as amt_diag_kernel and
// amt_bdy_kernel cut them; a work item is one chunk, lanes run along i -- every member's load of a wave is coalesced -- and
// the members are looped inside the thread.  Members are mstride elements apart and the outputs are allocations of their
// own, so whether a chunk moves as ONE 16-byte access is decided per array and per member from that address; a run's short
// last chunk and every chunk off a 16-byte boundary move element by element.  Nothing outside the box is read or written.
// The variance needs mean_d first: the members are read a second time, lines this thread loaded a moment before.
#include "amt_internal.h"
#include "amt_chunk_io.h"
#include <limits.h>
#include <math.h>

namespace {
constexpr int kMomentsThreads = 256;
constexpr long kMomentsMaxBlocks = 2048;      // 8 workgroups per CU; the rest by grid stride
#ifndef AMT_MOMENTS_AHEAD
#define AMT_MOMENTS_AHEAD 8                   // members loaded ahead of their use; 8 against 4: profiles/moments_notes.md
#endif

template <typename T>
struct AmtMomentsArgs {
    const T *a;
    T *mean, *var, *lo, *hi;                  // NULL: not wanted
    AmtBox box;
    int members;
};

// 256 threads, no LDS.  Offsets are 64-bit: a stacked fp32 array can pass 2^32 elements.
template <typename T>
__global__ __launch_bounds__(kMomentsThreads) void amt_moments_kernel(AmtMomentsArgs<T> p)
{
    typedef typename AmtVec16<T>::type V;
    constexpr int kPer = 16 / (int)sizeof(T);
    constexpr int kAhead = AMT_MOMENTS_AHEAD;
    const AmtBox &bx = p.box;
    const int M = p.members;
    const long mstride = bx.mstride;
    const long chunks = (bx.ni + kPer - 1) / kPer;
    const long total = (long)bx.nk * bx.nj * chunks;
    const bool want_var = p.var != nullptr, want_env = p.lo != nullptr || p.hi != nullptr;   // the same in every lane
    const double dm = (double)M, dm1 = (double)(M > 1 ? M - 1 : 1);

    for (long e = blockIdx.x * (long)kMomentsThreads + threadIdx.x; e < total; e += (long)gridDim.x * kMomentsThreads) {
        long r, c;                                                 // the run and the chunk inside it
        if (total <= 0xffffffffL) {
            r = (unsigned)e / (unsigned)chunks;
            c = (unsigned)e - (unsigned)r * (unsigned)chunks;
        } else {
            r = e / chunks;
            c = e - r * chunks;
        }
        const unsigned jj = (unsigned)r / (unsigned)bx.nk, kk = (unsigned)r - jj * (unsigned)bx.nk;   // r < 2^31 (host check)
        const int e0 = (int)c * kPer;
        const long at = bx.first + (long)jj * bx.jstride + (long)kk * bx.idim + e0;
        const int n = bx.ni - e0 < kPer ? bx.ni - e0 : kPer;
        const T *src = p.a + at;
        // a chunk of n elements moves as one 16-byte access where it is whole and ITS address lies on a 16-byte boundary
        // (amt_chunk_io.h: the lanes past n are 0 and never stored)
        auto wide = [&](const T *q) { return n == kPer && (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
        auto member = [&](int m) { return src + (long)m * mstride; };

        double s[kPer];
        T lo[kPer], hi[kPer];
        bool bad[kPer];
        {
            const V x = amt_chunk_load<T>(src, wide(src), n);
#pragma unroll
            for (int q = 0; q < kPer; ++q) {
                s[q] = (double)x[q];
                lo[q] = x[q];
                hi[q] = x[q];
                bad[q] = x[q] != x[q];
            }
        }
        auto take = [&](const V &x) {
#pragma unroll
            for (int q = 0; q < kPer; ++q) s[q] = s[q] + (double)x[q];
            if (want_env) {
#pragma unroll
                for (int q = 0; q < kPer; ++q) {
                    lo[q] = x[q] < lo[q] ? x[q] : lo[q];
                    hi[q] = x[q] > hi[q] ? x[q] : hi[q];
                    bad[q] = bad[q] || x[q] != x[q];
                }
            }
        };
        int m = 1;
        for (; m + kAhead <= M; m += kAhead) {
            V x[kAhead];
#pragma unroll
            for (int u = 0; u < kAhead; ++u) x[u] = amt_chunk_load<T>(member(m + u), wide(member(m + u)), n);
#pragma unroll
            for (int u = 0; u < kAhead; ++u) take(x[u]);
        }
        for (; m < M; ++m) take(amt_chunk_load<T>(member(m), wide(member(m)), n));

        double mean_d[kPer];
        V out;
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            mean_d[q] = s[q] / dm;
            out[q] = (T)mean_d[q];
        }
        if (p.mean) amt_chunk_store<T>(p.mean + at, wide(p.mean + at), n, out);

        if (want_var) {
            double sq[kPer];
#pragma unroll
            for (int q = 0; q < kPer; ++q) sq[q] = 0.0;
            auto spread = [&](const V &x) {
#pragma unroll
                for (int q = 0; q < kPer; ++q) {
                    const double d = (double)x[q] - mean_d[q];
                    const double dd = d * d;
                    sq[q] = sq[q] + dd;
                }
            };
            m = 0;
            for (; m + kAhead <= M; m += kAhead) {
                V x[kAhead];
#pragma unroll
                for (int u = 0; u < kAhead; ++u) x[u] = amt_chunk_load<T>(member(m + u), wide(member(m + u)), n);
#pragma unroll
                for (int u = 0; u < kAhead; ++u) spread(x[u]);
            }
            for (; m < M; ++m) spread(amt_chunk_load<T>(member(m), wide(member(m)), n));
#pragma unroll
            for (int q = 0; q < kPer; ++q) out[q] = (T)(sq[q] / dm1);
            amt_chunk_store<T>(p.var + at, wide(p.var + at), n, out);
        }
        if (want_env) {
            const T qnan = (T)__builtin_nan("");
            if (p.lo) {
#pragma unroll
                for (int q = 0; q < kPer; ++q) out[q] = bad[q] ? qnan : lo[q];
                amt_chunk_store<T>(p.lo + at, wide(p.lo + at), n, out);
            }
            if (p.hi) {
#pragma unroll
                for (int q = 0; q < kPer; ++q) out[q] = bad[q] ? qnan : hi[q];
                amt_chunk_store<T>(p.hi + at, wide(p.hi + at), n, out);
            }
        }
    }
}

struct MomentsOut { void *mean, *var, *lo, *hi; };

// [p, p + bytes) of two arrays share a byte
bool moments_overlap(const void *p, size_t pbytes, const void *q, size_t qbytes)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + qbytes && b < a + pbytes;
}

// the outputs against the input and against each other: host arithmetic
int moments_check_ranges(const char *who, const void *a, int members, const AmtBox &box, int wbytes, const MomentsOut &o)
{
    static const char *const names[4] = {"mean", "var", "lo", "hi"};
    const void *out[4] = {o.mean, o.var, o.lo, o.hi};
    const size_t one = (size_t)box.mstride * (size_t)wbytes;
    for (int k = 0; k < 4; ++k) {
        if (!out[k]) continue;
        if (moments_overlap(out[k], one, a, one * (size_t)members))
            return amt_fail(AMT_ERR_INVALID_ARG, "%s: the output %s overlaps the input a", who, names[k]);
        for (int l = 0; l < k; ++l)
            if (out[l] && moments_overlap(out[k], one, out[l], one))
                return amt_fail(AMT_ERR_INVALID_ARG, "%s: the outputs %s and %s overlap", who, names[l], names[k]);
    }
    return AMT_OK;
}

template <typename T>
int moments_launch(hipStream_t stream, const void *a, int members, const AmtBox &box, const MomentsOut &o)
{
    AmtMomentsArgs<T> p;
    p.a = static_cast<const T *>(a);
    p.mean = static_cast<T *>(o.mean);
    p.var = static_cast<T *>(o.var);
    p.lo = static_cast<T *>(o.lo);
    p.hi = static_cast<T *>(o.hi);
    p.box = box;
    p.members = members;
    constexpr long per = 16 / (long)sizeof(T);
    const long total = (long)box.nk * box.nj * ((box.ni + per - 1) / per);
    long blocks = (total + kMomentsThreads - 1) / kMomentsThreads;
    if (blocks > kMomentsMaxBlocks) blocks = kMomentsMaxBlocks;
    hipLaunchKernelGGL(amt_moments_kernel<T>, dim3((unsigned)blocks), dim3(kMomentsThreads), 0, stream, p);
    AMT_HIP(hipGetLastError());
    return AMT_OK;
}

int moments_device_call(const char *who, void *hip_stream, int wbytes, const void *a, int rank, int members,
                        int ims, int ime, int jms, int jme, int kms, int kme, int i0, int i1, int k0, int k1, int j0, int j1,
                        const MomentsOut &o)
{
    if (!a) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null array pointer a", who);
    if (!o.mean && !o.var && !o.lo && !o.hi)
        return amt_fail(AMT_ERR_INVALID_ARG, "%s: mean, var, lo and hi are all NULL: at least one output must be given", who);
    AmtBox box{};
    int rc = amt_box_plan(who, rank, members, ims, ime, jms, jme, kms, kme, i0, i1, k0, k1, j0, j1, &box);
    if (rc) return rc;
    if ((rc = moments_check_ranges(who, a, members, box, wbytes, o)) != AMT_OK) return rc;
    int ndev = 0;
    AMT_HIP(hipGetDeviceCount(&ndev));
    if (ndev < 1) return amt_fail(AMT_ERR_NO_DEVICE, "no HIP device visible");
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    return wbytes == 8 ? moments_launch<double>(stream, a, members, box, o) : moments_launch<float>(stream, a, members, box, o);
}
}  // namespace

#define AMT_MOMENTS_BOX_SIG int ims, int ime, int jms, int jme, int kms, int kme, int i0, int i1, int k0, int k1, int j0, int j1
#define AMT_MOMENTS_BOX_ARGS ims, ime, jms, jme, kms, kme, i0, i1, k0, k1, j0, j1

extern "C" int amt_moments_device_f32(void *hip_stream, const float *a, int rank, int members, AMT_MOMENTS_BOX_SIG,
                                      float *mean, float *var, float *lo, float *hi)
{
    return moments_device_call("amt_moments_device_f32", hip_stream, 4, a, rank, members, AMT_MOMENTS_BOX_ARGS, MomentsOut{mean, var, lo, hi});
}
extern "C" int amt_moments_device_f64(void *hip_stream, const double *a, int rank, int members, AMT_MOMENTS_BOX_SIG,
                                      double *mean, double *var, double *lo, double *hi)
{
    return moments_device_call("amt_moments_device_f64", hip_stream, 8, a, rank, members, AMT_MOMENTS_BOX_ARGS, MomentsOut{mean, var, lo, hi});
}

// What needs no handle is looked at first, so that a wrong field, region or output list is reported with or without one.
extern "C" int amt_ensemble_moments(amt_ensemble *e, int field, int region, void *mean, void *var, void *lo, void *hi)
{
    const char *who = "amt_ensemble_moments";
    if (field < 0 || field >= AMT_F_COUNT) return amt_fail(AMT_ERR_INVALID_ARG, "%s: unknown field %d", who, field);
    if (amt_field_rank(field) == 1) return amt_fail(AMT_ERR_INVALID_ARG, "%s: field %d is a rank-1 field: it has no box", who, field);
    if (region != AMT_REGION_WINDOW && region != AMT_REGION_MEMORY)
        return amt_fail(AMT_ERR_INVALID_ARG, "%s: region = %d is neither AMT_REGION_WINDOW nor AMT_REGION_MEMORY", who, region);
    if (!mean && !var && !lo && !hi)
        return amt_fail(AMT_ERR_INVALID_ARG, "%s: mean, var, lo and hi are all NULL: at least one output must be given", who);
    if (!e) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null handle", who);
    amt_domain &d = e->d;
    AmtBox box{};
    bool empty = false;
    int rc = amt_box_region(who, &d, field, region, e->members, &box, &empty);
    if (rc) return rc;
    if (empty) return amt_fail(AMT_ERR_INVALID_ARG, "%s: the compute window is empty", who);
    const MomentsOut o{mean, var, lo, hi};
    if ((rc = moments_check_ranges(who, d.field[field], e->members, box, d.dtype_bytes, o)) != AMT_OK) return rc;
    DeviceScope scope(d.device);
    return d.dtype_bytes == 8 ? moments_launch<double>(d.stream, d.field[field], e->members, box, o)
                              : moments_launch<float>(d.stream, d.field[field], e->members, box, o);
}
