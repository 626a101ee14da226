// amt_halo.hip -- the pack / unpack kernel of the host-owned halo exchange (include/amt_advance_mu_t.h section 11, DESIGN.md
// section 7.5).  A handle made with AMT_SLAB_TRANSPORT_EXTERNAL owns one contiguous send and one contiguous receive message per
// side that has a neighbour; ONE launch gathers everything the patch sends into its send messages, ONE launch scatters what
// arrived into the halo rows and columns.  The messages lie in device memory or (AMT_SLAB_EXTERNAL_HOST_BUFFERS) in page-locked
// host memory: the same kernel stores to / loads from either with ordinary vector accesses.
#include "amt_comm.h"

namespace {
typedef unsigned int amt_halo_v4u __attribute__((ext_vector_type(4)));

// Job q moves `runs` runs of `len` elements.  On the array side run r starts at array + r * idim (consecutive runs lie one
// memory row of i apart); the message side is dense: run r starts at msg + r * len.
//   a row of a 3-D field:    runs = kdim (one per level),  len = ni   (i fastest, then k)
//   a row of a 2-D field:    runs = 1,                     len = ni
//   a column of a 3-D field: runs = kdim * nj,             len = 1    (k fastest, then j: consecutive memory rows of i)
//   a column of a 2-D field: runs = nj,                    len = 1
template <typename W>
struct AmtHaloJobs {
    W *array[AMT_HALO_MAX_JOBS];
    W *msg[AMT_HALO_MAX_JOBS];
    long runs[AMT_HALO_MAX_JOBS];
    int len[AMT_HALO_MAX_JOBS];
    long idim;
};

// A work item is one 16-byte chunk of a run (its last chunk may be short).  Lanes run along (chunk, run): along i for a row --
// both sides coalesced --, along (level, row) for a column: the message side is coalesced, the array side touches one line per
// element, which is what a column is.  A whole chunk moves as ONE 16-byte access where the array run AND its message run start
// on a 16-byte boundary (decided per run: chunk c of a run lies 16 c bytes behind its start on both sides); the tail of a run
// and every other run move element by element.  Nothing outside a run is read or written.  The elements move as unsigned
// integers: every bit pattern, NaN payloads included, arrives as it left.  256 threads, no LDS, a handful of registers: a
// workgroup takes a sliver of a compute unit and the launch ends before the march launch behind it needs the units.
template <typename W, bool SCATTER>
__global__ __launch_bounds__(256) void amt_halo_kernel(AmtHaloJobs<W> jobs)
{
    constexpr int kPer = 16 / (int)sizeof(W);
    const int q = blockIdx.y;
    W *array = jobs.array[q];
    W *msg = jobs.msg[q];
    const long len = jobs.len[q];
    const long chunks = (len + kPer - 1) / kPer;
    const long total = jobs.runs[q] * chunks;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long r = chunks == 1 ? e : e / chunks;
        const long first = (e - r * chunks) * kPer;                // first element of this chunk inside its run
        W *a = array + r * jobs.idim + first;
        W *m = msg + r * len + first;
        const long left = len - first;
        if (left >= kPer && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(m)) & 15) == 0) {
            if (SCATTER) *reinterpret_cast<amt_halo_v4u *>(a) = *reinterpret_cast<const amt_halo_v4u *>(m);
            else *reinterpret_cast<amt_halo_v4u *>(m) = *reinterpret_cast<const amt_halo_v4u *>(a);
        } else {
            const int n = left < kPer ? (int)left : kPer;
            for (int i = 0; i < n; ++i) {
                if (SCATTER) a[i] = m[i];
                else m[i] = a[i];
            }
        }
    }
}

template <typename W>
int halo_launch(hipStream_t stream, bool scatter, long idim, const AmtHaloJob *job, int n)
{
    AmtHaloJobs<W> jobs{};
    jobs.idim = idim;
    long most = 0;
    for (int q = 0; q < n; ++q) {
        jobs.array[q] = static_cast<W *>(job[q].array);
        jobs.msg[q] = static_cast<W *>(job[q].msg);
        jobs.runs[q] = job[q].runs;
        jobs.len[q] = job[q].len;
        const long per = 16 / (long)sizeof(W);
        const long total = job[q].runs * ((job[q].len + per - 1) / per);
        most = total > most ? total : most;
    }
    if (most == 0) return AMT_OK;
    long blocks = (most + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    if (scatter) hipLaunchKernelGGL((amt_halo_kernel<W, true>), dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, stream, jobs);
    else hipLaunchKernelGGL((amt_halo_kernel<W, false>), dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, stream, jobs);
    AMT_HIP(hipGetLastError());
    return AMT_OK;
}
}  // namespace

int amt_halo_launch(hipStream_t stream, int dtype_bytes, bool scatter, long idim, const AmtHaloJob *jobs, int n)
{
    if (n <= 0) return AMT_OK;
    if (n > AMT_HALO_MAX_JOBS) return amt_fail(AMT_ERR_INVALID_ARG, "amt_halo_launch: %d jobs, at most %d", n, AMT_HALO_MAX_JOBS);
    for (int q = 0; q < n; ++q)
        if (!jobs[q].array || !jobs[q].msg || jobs[q].runs < 0 || jobs[q].len < 0)
            return amt_fail(AMT_ERR_INVALID_ARG, "amt_halo_launch: job %d has no array, no message or a negative extent", q);
    return dtype_bytes == 8 ? halo_launch<uint64_t>(stream, scatter, idim, jobs, n) : halo_launch<uint32_t>(stream, scatter, idim, jobs, n);
}
