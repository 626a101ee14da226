// amt_halo.hip -- the one kernel that moves halo cells (amt_halo.h; DESIGN.md sections 7.4 and 7.5): the column gather / scatter
// of the exchange engine's transports, the pack / unpack of the host-owned exchange (include/amt_advance_mu_t.h section 11) and
// the cyclic refresh (section 9) are ONE launch of it each.  A message may lie in device memory or
// (AMT_SLAB_EXTERNAL_HOST_BUFFERS) in page-locked host memory: the kernel stores to / loads from either with ordinary vector
// accesses.
#include "amt_halo.h"

namespace {
typedef unsigned int amt_halo_v4u __attribute__((ext_vector_type(4)));

template <typename W>
struct AmtHaloJobs {
    const W *src[AMT_HALO_MAX_JOBS];
    W *dst[AMT_HALO_MAX_JOBS];
    long runs[AMT_HALO_MAX_JOBS];
    long src_stride[AMT_HALO_MAX_JOBS], dst_stride[AMT_HALO_MAX_JOBS], member_stride[AMT_HALO_MAX_JOBS];
    int len[AMT_HALO_MAX_JOBS];
};

// Grid (blocks, jobs, members).  A work item is one 16-byte chunk of a run (its last chunk may be short).  Lanes run along
// (chunk, run): along i for a row -- both sides coalesced --, along (level, row) for a column: a dense side is coalesced, an
// array side touches one line per element, which is what a column is.  A whole chunk moves as ONE 16-byte access where its
// source AND its destination lie on a 16-byte boundary (decided per run, behind the member offset: chunk c of a run lies 16 c
// bytes behind its start on both sides); the tail of a run and every other run move element by element.  Nothing outside a run
// is read or written.  The elements move as unsigned integers: every bit pattern, NaN payloads included, arrives as it left.
// 256 threads, no LDS, a handful of registers: a workgroup takes a sliver of a compute unit and the launch ends before the
// march launch behind it needs the units.
template <typename W>
__global__ __launch_bounds__(256) void amt_halo_kernel(AmtHaloJobs<W> jobs)
{
    constexpr int kPer = 16 / (int)sizeof(W);
    const int q = blockIdx.y;
    const long moff = (long)blockIdx.z * jobs.member_stride[q];
    const W *src = jobs.src[q] + moff;
    W *dst = jobs.dst[q] + moff;
    const long len = jobs.len[q];
    const long chunks = (len + kPer - 1) / kPer;
    const long total = jobs.runs[q] * chunks;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long r = chunks == 1 ? e : e / chunks;
        const long first = (e - r * chunks) * kPer;                // first element of this chunk inside its run
        const W *s = src + r * jobs.src_stride[q] + first;
        W *d = dst + r * jobs.dst_stride[q] + first;
        const long left = len - first;
        if (left >= kPer && ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 15) == 0) {
            *reinterpret_cast<amt_halo_v4u *>(d) = *reinterpret_cast<const amt_halo_v4u *>(s);
        } else {
            const int n = left < kPer ? (int)left : kPer;
            for (int i = 0; i < n; ++i) d[i] = s[i];
        }
    }
}

template <typename W>
int halo_launch(hipStream_t stream, int members, const AmtHaloJob *job, int n)
{
    AmtHaloJobs<W> jobs{};
    long most = 0;
    for (int q = 0; q < n; ++q) {
        jobs.src[q] = static_cast<const W *>(job[q].src);
        jobs.dst[q] = static_cast<W *>(job[q].dst);
        jobs.runs[q] = job[q].runs;
        jobs.len[q] = job[q].len;
        jobs.src_stride[q] = job[q].src_stride;
        jobs.dst_stride[q] = job[q].dst_stride;
        jobs.member_stride[q] = job[q].member_stride;
        const long per = 16 / (long)sizeof(W);
        const long total = job[q].runs * ((job[q].len + per - 1) / per);
        most = total > most ? total : most;
    }
    if (most == 0) return AMT_OK;
    long blocks = (most + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(amt_halo_kernel<W>, dim3((unsigned)blocks, (unsigned)n, (unsigned)members), dim3(256), 0, stream, jobs);
    AMT_HIP(hipGetLastError());
    return AMT_OK;
}
}  // namespace

int amt_halo_launch(hipStream_t stream, int dtype_bytes, int members, const AmtHaloJob *jobs, int n)
{
    if (n <= 0) return AMT_OK;
    if (n > AMT_HALO_MAX_JOBS) return amt_fail(AMT_ERR_INVALID_ARG, "amt_halo_launch: %d jobs, at most %d", n, AMT_HALO_MAX_JOBS);
    if (members < 1 || members > 65535) return amt_fail(AMT_ERR_INVALID_ARG, "amt_halo_launch: %d members, 1 to 65535 per launch", members);
    for (int q = 0; q < n; ++q)
        if (!jobs[q].src || !jobs[q].dst || jobs[q].runs < 0 || jobs[q].len < 0)
            return amt_fail(AMT_ERR_INVALID_ARG, "amt_halo_launch: job %d has no array, no message or a negative extent", q);
    return dtype_bytes == 8 ? halo_launch<uint64_t>(stream, members, jobs, n) : halo_launch<uint32_t>(stream, members, jobs, n);
}
