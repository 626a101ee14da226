// amt_diag.hip -- looking at resident state on the device (include/amt_advance_mu_t.h section 10):
// statistics of a box of a field, a bit comparison of two fields, and the non-finite guard of the resident handles.
//
// One kernel, two accumulators.  A BOX is ni x nk x nj elements of a rank-3 (rank 2: nk = 1) field; its nk * nj ROW RUNS are ni
// contiguous elements each.  A run is cut into CHUNKS of 16 bytes counted from the run's first element (2 doubles, 4 floats); a
// workgroup of 256 threads is 2^s lanes along i times 256 / 2^s runs (s: the smallest power of two that covers a run's chunks,
// at most 256 lanes), and the workgroups stride over the groups of runs.  Which thread takes which element therefore depends on
// the BOX SHAPE ALONE -- not on where the array lies.  Alignment only decides how a chunk is loaded, per run as in
// amt_halo_kernel: a run whose first element lies on a 16-byte boundary moves its whole chunks as 16-byte loads; the last,
// partial chunk of a run and every chunk of a run that starts off a boundary are single-element loads.  No load touches an
// element outside the box, so nothing outside the array is read and a NaN in a halo cell cannot reach a result.
//
// Determinism: thread (elements in order) -> wave (shuffle tree) -> workgroup (its waves in order, through LDS) -> ONE partial
// per workgroup in a workspace -> the workgroup that draws the last ticket of its member folds the partials: thread t takes
// partials t, t + 256, ... in order, then the same wave / workgroup tree.  Every step is a fixed function of the box shape; there
// is no floating-point atomic.  A member's record has the same bits from run to run, on any stream, alone or stacked.
#include "amt_internal.h"
#include <limits.h>
#include <math.h>
#include <sys/syscall.h>
#include <unistd.h>
#include <type_traits>

namespace {
constexpr int kDiagThreads = 256;
constexpr int kDiagWords = 8;             // 64-bit words of a partial
constexpr unsigned kDiagMaxWg = 2048;     // workgroups per member at most
constexpr long long kNoOffset = LLONG_MAX;

struct AmtDiagBox {
    long idim;        // elements of a memory row of i
    long jstride;     // elements from row j to row j + 1: idim * kdim (rank 3), idim (rank 2)
    long mstride;     // elements from member m to member m + 1
    long first;       // offset of the box's first element from the member's base
    int ni, nk, nj;   // the box
    int shift;        // log2 of the lanes along i
    unsigned nwg;     // workgroups per member
};

// what the guard's launches carry besides the statistics (all NULL / 0 for a plain statistics launch)
struct AmtGuardPinned {                   // page-locked host memory, written by the kernel
    long long sweep;                      // 0: no finding; written LAST
    long long offset, n_nonfinite;
    int field, member;
};
struct AmtDiagGuard {
    unsigned long long *member_finding;   // [2 * members]: non-finite count, first offset
    unsigned int *launch_ticket;          // members that have finished in this launch
    unsigned int *found;                  // device-side copy of "a finding is recorded"
    AmtGuardPinned *rec;
    long long sweep;
    int field;
};

template <typename T>
struct AmtDiagArgs {
    const T *a, *b;                       // b: compare only
    AmtDiagBox box;
    unsigned long long *partials;         // [members * nwg * kDiagWords]
    unsigned int *tickets;                // [members], zero between launches
    void *out;                            // amt_field_stats / amt_field_diff [members], host-visible; NULL for a guard launch
    AmtDiagGuard guard;
};

__device__ inline unsigned long long d2u(double x) { return (unsigned long long)__double_as_longlong(x); }
__device__ inline double u2d(unsigned long long x) { return __longlong_as_double((long long)x); }
__device__ inline long long shfl_down_ll(long long x, int d) { return __shfl_down(x, d, 64); }

struct StatsAcc {
    long long n_nan, n_inf, first;
    double mn, mx, mabs, sum;
    __device__ void init() { n_nan = 0; n_inf = 0; first = kNoOffset; mn = INFINITY; mx = -INFINITY; mabs = 0.0; sum = 0.0; }
    template <typename T>
    __device__ void take(T x, T, long long off)
    {
        const bool nan = x != x;
        const bool inf = !nan && (x == (T)INFINITY || x == -(T)INFINITY);
        const bool fin = !(nan || inf);
        n_nan += nan ? 1 : 0;
        n_inf += inf ? 1 : 0;
        first = (!fin && off < first) ? off : first;
        const double d = fin ? (double)x : 0.0;       // + 0.0 never changes a sum that started at + 0.0
        const double ad = fabs(d);
        mn = (fin && d < mn) ? d : mn;
        mx = (fin && d > mx) ? d : mx;
        mabs = ad > mabs ? ad : mabs;
        sum += d;
    }
    // *this holds the elements in front of o's
    __device__ void combine(const StatsAcc &o)
    {
        n_nan += o.n_nan; n_inf += o.n_inf;
        first = o.first < first ? o.first : first;
        mn = o.mn < mn ? o.mn : mn;
        mx = o.mx > mx ? o.mx : mx;
        mabs = o.mabs > mabs ? o.mabs : mabs;
        sum += o.sum;
    }
    __device__ StatsAcc down(int d) const
    {
        StatsAcc o;
        o.n_nan = shfl_down_ll(n_nan, d); o.n_inf = shfl_down_ll(n_inf, d); o.first = shfl_down_ll(first, d);
        o.mn = __shfl_down(mn, d, 64); o.mx = __shfl_down(mx, d, 64); o.mabs = __shfl_down(mabs, d, 64); o.sum = __shfl_down(sum, d, 64);
        return o;
    }
    __device__ void to_words(unsigned long long *w) const
    {
        w[0] = (unsigned long long)n_nan; w[1] = (unsigned long long)n_inf; w[2] = (unsigned long long)first;
        w[3] = d2u(mn); w[4] = d2u(mx); w[5] = d2u(mabs); w[6] = d2u(sum); w[7] = 0;
    }
    __device__ void from_words(const unsigned long long *w)
    {
        n_nan = (long long)w[0]; n_inf = (long long)w[1]; first = (long long)w[2];
        mn = u2d(w[3]); mx = u2d(w[4]); mabs = u2d(w[5]); sum = u2d(w[6]);
    }
    __device__ void write(void *out, unsigned m, long long count) const
    {
        amt_field_stats *r = static_cast<amt_field_stats *>(out) + m;
        r->count = count; r->n_nan = n_nan; r->n_inf = n_inf;
        r->first_nonfinite = first == kNoOffset ? -1 : first;
        r->min = mn; r->max = mx; r->max_abs = mabs; r->sum = sum;
    }
};

struct DiffAcc {
    long long n_diff, first;
    double mad;
    __device__ void init() { n_diff = 0; first = kNoOffset; mad = 0.0; }
    template <typename T>
    __device__ void take(T x, T y, long long off)
    {
        typedef typename std::conditional<sizeof(T) == 8, unsigned long long, unsigned int>::type U;
        U bx, by;
        __builtin_memcpy(&bx, &x, sizeof(T));
        __builtin_memcpy(&by, &y, sizeof(T));
        const bool differ = bx != by;
        n_diff += differ ? 1 : 0;
        first = (differ && off < first) ? off : first;
        const double dx = (double)x, dy = (double)y;
        const bool fin = fabs(dx) < INFINITY && fabs(dy) < INFINITY;     // false for NaN and Inf on either side
        const double ad = fin ? fabs(dx - dy) : 0.0;
        mad = ad > mad ? ad : mad;
    }
    __device__ void combine(const DiffAcc &o)
    {
        n_diff += o.n_diff;
        first = o.first < first ? o.first : first;
        mad = o.mad > mad ? o.mad : mad;
    }
    __device__ DiffAcc down(int d) const
    {
        DiffAcc o;
        o.n_diff = shfl_down_ll(n_diff, d); o.first = shfl_down_ll(first, d); o.mad = __shfl_down(mad, d, 64);
        return o;
    }
    __device__ void to_words(unsigned long long *w) const
    {
        w[0] = (unsigned long long)n_diff; w[1] = (unsigned long long)first; w[2] = d2u(mad);
        w[3] = 0; w[4] = 0; w[5] = 0; w[6] = 0; w[7] = 0;
    }
    __device__ void from_words(const unsigned long long *w) { n_diff = (long long)w[0]; first = (long long)w[1]; mad = u2d(w[2]); }
    __device__ void write(void *out, unsigned m, long long count) const
    {
        amt_field_diff *r = static_cast<amt_field_diff *>(out) + m;
        r->count = count; r->n_diff = n_diff;
        r->first_diff = first == kNoOffset ? -1 : first;
        r->max_abs_diff = mad;
    }
};

// Folds the 256 threads' accumulators into thread 0's: lanes of a wave through shuffles, the four waves in order through LDS.
// Every thread of the workgroup calls it; lds holds 4 * kDiagWords words.
template <typename Acc>
__device__ void block_fold(Acc &acc, unsigned long long *lds)
{
    for (int d = 32; d >= 1; d >>= 1) {
        const Acc o = acc.down(d);
        acc.combine(o);
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();                                   // lds may still be read from an earlier fold
    if ((threadIdx.x & 63) == 0) acc.to_words(lds + wave * kDiagWords);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kDiagThreads / 64; ++w) {
            Acc o;
            o.from_words(lds + w * kDiagWords);
            acc.combine(o);
        }
    }
}

template <typename T, bool CMP>
__global__ __launch_bounds__(kDiagThreads) void amt_diag_kernel(AmtDiagArgs<T> p)
{
    typedef typename std::conditional<CMP, DiffAcc, StatsAcc>::type Acc;
    constexpr int kPer = 16 / (int)sizeof(T);
    typedef T V __attribute__((ext_vector_type(kPer)));
    __shared__ unsigned long long lds[(kDiagThreads / 64) * kDiagWords];
    __shared__ int flag;

    const AmtDiagBox &bx = p.box;
    const unsigned m = blockIdx.z;
    const long moff = (long)m * bx.mstride;
    const T *a = p.a + moff;
    const T *b = CMP ? p.b + moff : p.a + moff;
    const int tx = threadIdx.x & ((1 << bx.shift) - 1);
    const int ty = threadIdx.x >> bx.shift;
    const int lanes = 1 << bx.shift;
    const unsigned ry = kDiagThreads >> bx.shift;                 // runs per group
    const unsigned runs = (unsigned)bx.nk * (unsigned)bx.nj;      // < 2^31 (checked on the host)
    const unsigned groups = (runs + ry - 1) / ry;
    const int nchunk = (bx.ni + kPer - 1) / kPer;

    Acc acc;
    acc.init();
    for (unsigned g = blockIdx.x; g < groups; g += bx.nwg) {
        const unsigned r = g * ry + ty;
        if (r >= runs) continue;
        const unsigned jj = r / (unsigned)bx.nk, kk = r - jj * (unsigned)bx.nk;
        const long rowoff = bx.first + (long)jj * bx.jstride + (long)kk * bx.idim;
        const T *ra = a + rowoff, *rb = b + rowoff;
        const bool vec = ((reinterpret_cast<uintptr_t>(ra) | reinterpret_cast<uintptr_t>(rb)) & 15) == 0;
        for (int c = tx; c < nchunk; c += lanes) {
            const int e0 = c * kPer;
            if (vec && e0 + kPer <= bx.ni) {
                const V va = *reinterpret_cast<const V *>(ra + e0);
                const V vb = CMP ? *reinterpret_cast<const V *>(rb + e0) : va;
#pragma unroll
                for (int q = 0; q < kPer; ++q) acc.take((T)va[q], (T)vb[q], (long long)(rowoff + e0 + q));
            } else {
                const int e1 = e0 + kPer < bx.ni ? e0 + kPer : bx.ni;
                for (int e = e0; e < e1; ++e) {
                    const T xa = ra[e];
                    const T xb = CMP ? rb[e] : xa;
                    acc.take(xa, xb, (long long)(rowoff + e));
                }
            }
        }
    }
    block_fold(acc, lds);

    // one partial per workgroup, written through to memory; the last workgroup of the member to get here folds them
    unsigned long long *part = p.partials + ((size_t)m * bx.nwg) * kDiagWords;
    if (threadIdx.x == 0) {
        unsigned long long w[kDiagWords];
        acc.to_words(w);
        for (int q = 0; q < kDiagWords; ++q)
            __hip_atomic_store(part + (size_t)blockIdx.x * kDiagWords + q, w[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const unsigned t = __hip_atomic_fetch_add(p.tickets + m, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        flag = (t == bx.nwg - 1) ? 1 : 0;
        if (flag) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            __hip_atomic_store(p.tickets + m, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // ready for the next launch
        }
    }
    __syncthreads();
    if (!flag) return;

    acc.init();
    for (unsigned q = threadIdx.x; q < bx.nwg; q += kDiagThreads) {
        unsigned long long w[kDiagWords];
        for (int k = 0; k < kDiagWords; ++k)
            w[k] = __hip_atomic_load(part + (size_t)q * kDiagWords + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        Acc o;
        o.from_words(w);
        acc.combine(o);
    }
    block_fold(acc, lds);
    if (threadIdx.x == 0 && p.out) {
        acc.write(p.out, m, (long long)bx.ni * bx.nk * bx.nj);
        __threadfence_system();
    }

    if constexpr (!CMP) {
        // Guard launch: the member that finishes last looks at all members' findings and records the lowest member's, unless an
        // earlier launch (an earlier sweep, or an earlier field of this sweep) has recorded one already.
        const AmtDiagGuard &gd = p.guard;
        if (!gd.rec) return;
        const unsigned members = gridDim.z;
        __syncthreads();
        if (threadIdx.x == 0) {
            __hip_atomic_store(gd.member_finding + 2 * (size_t)m, (unsigned long long)(acc.n_nan + acc.n_inf), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(gd.member_finding + 2 * (size_t)m + 1, (unsigned long long)acc.first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            const unsigned t = __hip_atomic_fetch_add(gd.launch_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            flag = (t == members - 1) ? 0x7fffffff : -1;       // the last member: the lowest member with a finding goes here
            if (flag >= 0) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                __hip_atomic_store(gd.launch_ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();
        if (flag < 0) return;
        int lowest = 0x7fffffff;
        for (unsigned q = threadIdx.x; q < members; q += kDiagThreads)
            if (__hip_atomic_load(gd.member_finding + 2 * (size_t)q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 && (int)q < lowest)
                lowest = (int)q;
        if (lowest != 0x7fffffff) atomicMin(&flag, lowest);     // an integer minimum in LDS: the order does not matter
        __syncthreads();
        if (threadIdx.x == 0 && flag != 0x7fffffff &&
            __hip_atomic_load(gd.found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
            __hip_atomic_store(gd.found, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const size_t q = (size_t)flag;
            gd.rec->n_nonfinite = (long long)__hip_atomic_load(gd.member_finding + 2 * q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            gd.rec->offset = (long long)__hip_atomic_load(gd.member_finding + 2 * q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            gd.rec->field = gd.field;
            gd.rec->member = flag;
            __threadfence_system();                              // the record is in host memory before the word the host polls
            __hip_atomic_store(&gd.rec->sweep, gd.sweep, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            __threadfence_system();
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct DiagExtents { int ims, ime, jms, jme, kms, kme; };
struct DiagBoxArg { int i0, i1, k0, k1, j0, j1; };

// Argument checks and the launch plan: host arithmetic only.
int diag_plan(const char *who, int rank, int members, const DiagExtents &x, DiagBoxArg bxa, AmtDiagBox &box, int max_members = 65535)
{
    if (rank != 2 && rank != 3) return amt_fail(AMT_ERR_INVALID_ARG, "%s: rank = %d: only rank-2 and rank-3 fields have a box", who, rank);
    if (members < 1) return amt_fail(AMT_ERR_INVALID_ARG, "%s: members = %d: an ensemble has at least one member", who, members);
    if (members > max_members) return amt_fail(AMT_ERR_INVALID_ARG, "%s: %d members: one launch covers at most %d", who, members, max_members);
    if (x.ime < x.ims || x.jme < x.jms || (rank == 3 && x.kme < x.kms)) return amt_fail(AMT_ERR_INVALID_ARG, "%s: empty memory extents", who);
    if (rank == 2) { bxa.k0 = bxa.k1 = 0; }
    if (bxa.i1 < bxa.i0 || bxa.j1 < bxa.j0 || bxa.k1 < bxa.k0)
        return amt_fail(AMT_ERR_INVALID_ARG, "%s: empty box %d:%d, %d:%d, %d:%d", who, bxa.i0, bxa.i1, bxa.k0, bxa.k1, bxa.j0, bxa.j1);
    if (bxa.i0 < x.ims || bxa.i1 > x.ime || bxa.j0 < x.jms || bxa.j1 > x.jme || (rank == 3 && (bxa.k0 < x.kms || bxa.k1 > x.kme)))
        return amt_fail(AMT_ERR_INVALID_ARG, "%s: the box %d:%d, %d:%d, %d:%d is not inside memory %d:%d, %d:%d, %d:%d", who,
                        bxa.i0, bxa.i1, bxa.k0, bxa.k1, bxa.j0, bxa.j1, x.ims, x.ime, x.kms, x.kme, x.jms, x.jme);
    const long idim = (long)x.ime - x.ims + 1, kdim = rank == 3 ? (long)x.kme - x.kms + 1 : 1, jdim = (long)x.jme - x.jms + 1;
    box.idim = idim;
    box.jstride = idim * kdim;
    box.mstride = idim * kdim * jdim;
    box.ni = bxa.i1 - bxa.i0 + 1;
    box.nk = bxa.k1 - bxa.k0 + 1;
    box.nj = bxa.j1 - bxa.j0 + 1;
    box.first = ((long)(bxa.j0 - x.jms) * kdim + (rank == 3 ? (long)(bxa.k0 - x.kms) : 0)) * idim + (bxa.i0 - x.ims);
    if ((long)box.nk * box.nj > 0x7fffffffL) return amt_fail(AMT_ERR_INVALID_ARG, "%s: the box has more than 2^31 - 1 row runs", who);
    return AMT_OK;
}

// lanes along i, workgroups per member: functions of the box shape and the element size alone
void diag_shape(AmtDiagBox &box, int wbytes)
{
    const int per = 16 / wbytes;
    const int nchunk = (box.ni + per - 1) / per;
    int s = 0;
    while (s < 8 && (1 << s) < nchunk) ++s;
    box.shift = s;
    const long ry = kDiagThreads >> s;
    const long groups = ((long)box.nk * box.nj + ry - 1) / ry;
    long nwg = (groups + 3) / 4;                       // four groups of runs per workgroup where there are enough
    box.nwg = (unsigned)(nwg < 1 ? 1 : nwg > (long)kDiagMaxWg ? (long)kDiagMaxWg : nwg);
}
}  // namespace

// workspace, result records and guard state of one handle, or of one host thread for the pointer-level calls
struct AmtDiagState {
    int device = -1;
    int members = 0;                       // the tickets, findings and records hold this many members
    size_t part_words = 0;
    unsigned long long *partials = nullptr;
    unsigned int *tickets = nullptr;       // [members] member tickets, then the launch ticket, then the guard's "found"
    unsigned long long *member_finding = nullptr;
    void *records = nullptr;               // page-locked: members records of the larger kind
    AmtGuardPinned *guard = nullptr;       // page-locked
    long long sweeps = 0, checked = 0;     // since the guard was armed

    void release()
    {
        if (device < 0) return;
        int prev = -1;
        const bool sw = hipGetDevice(&prev) == hipSuccess && prev != device && hipSetDevice(device) == hipSuccess;
        if (partials) (void)hipFree(partials);
        if (tickets) (void)hipFree(tickets);
        if (member_finding) (void)hipFree(member_finding);
        if (records) (void)hipHostFree(records);
        if (guard) (void)hipHostFree(guard);
        if (sw) (void)hipSetDevice(prev);
        *this = AmtDiagState();
    }
    // room for `want_members` members of `nwg` workgroups each on the current device; grows, never shrinks
    hipError_t reserve(int want_members, unsigned nwg)
    {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (device != dev) { release(); device = dev; }
        if (want_members > members) {
            if (tickets) (void)hipFree(tickets);
            if (member_finding) (void)hipFree(member_finding);
            if (records) (void)hipHostFree(records);
            tickets = nullptr; member_finding = nullptr; records = nullptr; members = 0;
            const size_t tbytes = ((size_t)want_members + 2) * sizeof(unsigned int);
            e = hipMalloc((void **)&tickets, tbytes);
            if (e == hipSuccess) e = hipMemset(tickets, 0, tbytes);
            if (e == hipSuccess) e = hipStreamSynchronize(nullptr);        // the zeros are there before any stream's first launch
            if (e == hipSuccess) e = hipMalloc((void **)&member_finding, (size_t)want_members * 2 * sizeof(unsigned long long));
            if (e == hipSuccess) e = hipHostMalloc(&records, (size_t)want_members * sizeof(amt_field_stats), hipHostMallocDefault);
            if (e != hipSuccess) return e;
            members = want_members;
        }
        const size_t words = (size_t)want_members * nwg * kDiagWords;
        if (words > part_words) {
            if (partials) (void)hipFree(partials);
            partials = nullptr; part_words = 0;
            e = hipMalloc((void **)&partials, words * sizeof(unsigned long long));
            if (e != hipSuccess) return e;
            part_words = words;
        }
        if (!guard) {
            e = hipHostMalloc((void **)&guard, sizeof(AmtGuardPinned), hipHostMallocDefault);
            if (e != hipSuccess) { guard = nullptr; return e; }
            memset(guard, 0, sizeof *guard);
        }
        return hipSuccess;
    }
};

namespace {
static_assert(sizeof(amt_field_stats) >= sizeof(amt_field_diff), "the record buffer is sized for the larger kind");

int diag_reserve(const char *who, AmtDiagState &st, int members, unsigned nwg)
{
    const hipError_t e = st.reserve(members, nwg);
    if (e == hipSuccess) return AMT_OK;
    (void)hipGetLastError();
    return amt_fail(e == hipErrorOutOfMemory ? AMT_ERR_ALLOC : e == hipErrorNoDevice ? AMT_ERR_NO_DEVICE : AMT_ERR_HIP,
                    "%s: workspace: %s", who, hipGetErrorString(e));
}

template <typename T, bool CMP>
int diag_launch(hipStream_t stream, AmtDiagState &st, const void *a, const void *b, const AmtDiagBox &box, int members,
                void *out, const AmtDiagGuard &guard)
{
    AmtDiagArgs<T> p;
    p.a = static_cast<const T *>(a);
    p.b = static_cast<const T *>(b);
    p.box = box;
    p.partials = st.partials;
    p.tickets = st.tickets;
    p.out = out;
    p.guard = guard;
    hipLaunchKernelGGL((amt_diag_kernel<T, CMP>), dim3(box.nwg, 1, (unsigned)members), dim3(kDiagThreads), 0, stream, p);
    AMT_HIP(hipGetLastError());
    return AMT_OK;
}

// enqueue, wait for the stream, copy the records to the caller; the state's workspace must not be in use by another stream
int diag_run(const char *who, hipStream_t stream, AmtDiagState &st, int dtype_bytes, bool cmp, const void *a, const void *b,
             AmtDiagBox box, int members, void *out)
{
    diag_shape(box, dtype_bytes);
    int rc = diag_reserve(who, st, members, box.nwg);
    if (rc) return rc;
    const AmtDiagGuard none{};
    if (cmp) rc = dtype_bytes == 8 ? diag_launch<double, true>(stream, st, a, b, box, members, st.records, none)
                                   : diag_launch<float, true>(stream, st, a, b, box, members, st.records, none);
    else rc = dtype_bytes == 8 ? diag_launch<double, false>(stream, st, a, b, box, members, st.records, none)
                               : diag_launch<float, false>(stream, st, a, b, box, members, st.records, none);
    if (rc) return rc;
    AMT_HIP(hipStreamSynchronize(stream));
    memcpy(out, st.records, (size_t)members * (cmp ? sizeof(amt_field_diff) : sizeof(amt_field_stats)));
    return AMT_OK;
}

// the pointer-level calls keep their workspace per calling host thread, as the one-shot calls do
struct ThreadDiag {
    AmtDiagState st;
    // a worker thread's workspace goes with the thread; the main thread's is left to the operating system at process exit
    ~ThreadDiag() { if ((long)syscall(SYS_gettid) != (long)getpid()) st.release(); }
};
thread_local ThreadDiag tl_diag;

int diag_device_call(const char *who, void *hip_stream, int dtype_bytes, bool cmp, const void *a, const void *b, int rank, int members,
                     const DiagExtents &x, const DiagBoxArg &bxa, void *out)
{
    AmtDiagBox box{};
    const int rc = diag_plan(who, rank, members, x, bxa, box);
    if (rc) return rc;
    if (!out) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null out pointer", who);
    if (!a || (cmp && !b)) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null array pointer", who);
    int ndev = 0;
    AMT_HIP(hipGetDeviceCount(&ndev));
    if (ndev < 1) return amt_fail(AMT_ERR_NO_DEVICE, "no HIP device visible");
    return diag_run(who, static_cast<hipStream_t>(hip_stream), tl_diag.st, dtype_bytes, cmp, a, b, box, members, out);
}

// the box of a region of a field of a handle; AMT_OK with *empty set when the compute window holds no cell
int diag_region(const char *who, const amt_domain *d, int field, int region, int members, AmtDiagBox &box, bool *empty, int max_members = 65535)
{
    *empty = false;
    if (field < 0 || field >= AMT_F_COUNT) return amt_fail(AMT_ERR_INVALID_ARG, "%s: unknown field %d", who, field);
    const int rank = amt_field_rank(field);
    if (rank == 1) return amt_fail(AMT_ERR_INVALID_ARG, "%s: field %d is a rank-1 field: it has no box", who, field);
    DiagBoxArg b;
    if (region == AMT_REGION_MEMORY) {
        b = DiagBoxArg{d->ims, d->ime, d->kms, d->kme, d->jms, d->jme};
    } else if (region == AMT_REGION_WINDOW) {
        const AmtWindow w = amt_window(d->periodic_x, d->specified, d->nested, d->ids, d->ide, d->jds, d->jde, d->its, d->ite,
                                       d->jts, d->jte, d->kts, d->kte);
        b = DiagBoxArg{w.i_start, w.i_end, w.k_start, w.k_end, w.j_start, w.j_end};
        if (b.i1 < b.i0 || b.j1 < b.j0 || (rank == 3 && b.k1 < b.k0)) { *empty = true; return AMT_OK; }
    } else {
        return amt_fail(AMT_ERR_INVALID_ARG, "%s: region = %d is neither AMT_REGION_WINDOW nor AMT_REGION_MEMORY", who, region);
    }
    return diag_plan(who, rank, members, DiagExtents{d->ims, d->ime, d->jms, d->jme, d->kms, d->kme}, b, box, max_members);
}

int diag_state(const char *who, amt_domain *d)
{
    if (d->diag) return AMT_OK;
    d->diag = new (std::nothrow) AmtDiagState;
    return d->diag ? AMT_OK : amt_fail(AMT_ERR_ALLOC, "%s: host allocation failed", who);
}

int handle_stats(const char *who, amt_domain *d, int members, int field, int region, amt_field_stats *out)
{
    if (!d) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null handle", who);
    if (!out) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null out pointer", who);
    AmtDiagBox box{};
    bool empty = false;
    int rc = diag_region(who, d, field, region, members, box, &empty);
    if (rc) return rc;
    if (empty) return amt_fail(AMT_ERR_INVALID_ARG, "%s: the compute window is empty", who);
    DeviceScope scope(d->device);
    if ((rc = diag_state(who, d)) != AMT_OK) return rc;
    return diag_run(who, d->stream, *d->diag, d->dtype_bytes, false, d->field[field], nullptr, box, members, out);
}

bool same_shape(const amt_domain *a, const amt_domain *b)
{
    return a->dtype_bytes == b->dtype_bytes && a->periodic_x == b->periodic_x && a->specified == b->specified && a->nested == b->nested &&
           a->ids == b->ids && a->ide == b->ide && a->jds == b->jds && a->jde == b->jde && a->kde == b->kde && a->ims == b->ims &&
           a->ime == b->ime && a->jms == b->jms && a->jme == b->jme && a->kms == b->kms && a->kme == b->kme && a->its == b->its &&
           a->ite == b->ite && a->jts == b->jts && a->jte == b->jte && a->kts == b->kts && a->kte == b->kte;
}

int handle_compare(const char *who, amt_domain *a, amt_domain *b, int members_a, int members_b, int field, int region, amt_field_diff *out)
{
    if (!a || !b) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null handle", who);
    if (!out) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null out pointer", who);
    if (!same_shape(a, b) || members_a != members_b)
        return amt_fail(AMT_ERR_INVALID_ARG, "%s: the two handles differ in dtype, flags, bounds or member count", who);
    if (a->device != b->device) return amt_fail(AMT_ERR_INVALID_ARG, "%s: the two handles live on devices %d and %d", who, a->device, b->device);
    AmtDiagBox box{};
    bool empty = false;
    int rc = diag_region(who, a, field, region, members_a, box, &empty);
    if (rc) return rc;
    if (empty) return amt_fail(AMT_ERR_INVALID_ARG, "%s: the compute window is empty", who);
    DeviceScope scope(a->device);
    if ((rc = diag_state(who, a)) != AMT_OK) return rc;
    if (b->stream != a->stream) AMT_HIP(hipStreamSynchronize(b->stream));      // b's field is final before a's stream reads it
    return diag_run(who, a->stream, *a->diag, a->dtype_bytes, true, a->field[field], b->field[field], box, members_a, out);
}

const int kGuardFields[] = {AMT_F_WW, AMT_F_T, AMT_F_MU};          // the order of "first"
const char *const kGuardNames[] = {"ww", "t", "mu"};

int handle_set_guard(const char *who, amt_domain *d, int members, int every)
{
    if (!d) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null handle", who);
    if (every < 0) return amt_fail(AMT_ERR_INVALID_ARG, "%s: every = %d: 0 turns the guard off, n >= 1 checks after every n-th sweep", who, every);
    DeviceScope scope(d->device);
    if (every == 0 && !d->diag) { d->guard_every = 0; return AMT_OK; }
    int rc = diag_state(who, d);
    if (rc) return rc;
    AmtDiagState &st = *d->diag;
    // everything the checks will need is allocated here: the step path allocates nothing
    unsigned nwg = 1;
    for (int f : kGuardFields) {
        AmtDiagBox box{};
        bool empty = false;
        if ((rc = diag_region(who, d, f, AMT_REGION_WINDOW, members, box, &empty)) != AMT_OK) return rc;
        if (empty) continue;
        diag_shape(box, d->dtype_bytes);
        nwg = box.nwg > nwg ? box.nwg : nwg;
    }
    if ((rc = diag_reserve(who, st, members, nwg)) != AMT_OK) return rc;
    // a check of the previous arming may still be in flight: let it finish, then clear what it may have found
    AMT_HIP(hipStreamSynchronize(d->stream));
    AMT_HIP(hipMemsetAsync(st.tickets + st.members, 0, 2 * sizeof(unsigned int), d->stream));
    AMT_HIP(hipStreamSynchronize(d->stream));
    memset(st.guard, 0, sizeof *st.guard);
    st.sweeps = 0;
    st.checked = 0;
    d->guard_every = every;
    return AMT_OK;
}

int handle_guard_report(const char *who, amt_domain *d, amt_guard_report *out)
{
    if (!d) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null handle", who);
    if (!out) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null out pointer", who);
    memset(out, 0, sizeof *out);
    if (!d->guard_every || !d->diag) return AMT_OK;
    DeviceScope scope(d->device);
    AMT_HIP(hipStreamSynchronize(d->stream));
    const AmtDiagState &st = *d->diag;
    out->sweeps_checked = st.checked;
    const long long sweep = __atomic_load_n(&st.guard->sweep, __ATOMIC_ACQUIRE);
    if (sweep) {
        out->sweep = sweep;
        out->field = st.guard->field;
        out->member = st.guard->member;
        out->offset = st.guard->offset;
        out->n_nonfinite = st.guard->n_nonfinite;
    }
    return AMT_OK;
}
}  // namespace

int amt_diag_guard_status(const char *who, const amt_domain *d)
{
    if (!d->guard_every || !d->diag || !d->diag->guard) return AMT_OK;
    const AmtGuardPinned *g = d->diag->guard;
    const long long sweep = __atomic_load_n(&g->sweep, __ATOMIC_ACQUIRE);
    if (!sweep) return AMT_OK;
    const long idim = d->ime - d->ims + 1, kdim = d->kme - d->kms + 1;
    const int which = g->field == AMT_F_WW ? 0 : g->field == AMT_F_T ? 1 : 2;
    const long long off = g->offset;
    if (which == 2)
        return amt_fail(AMT_ERR_NONFINITE, "%s: non-finite guard: sweep %lld, field mu, member %d, (i,j) = (%lld,%lld), %lld non-finite", who,
                        sweep, g->member, off % idim + d->ims, off / idim + d->jms, g->n_nonfinite);
    return amt_fail(AMT_ERR_NONFINITE, "%s: non-finite guard: sweep %lld, field %s, member %d, (i,k,j) = (%lld,%lld,%lld), %lld non-finite", who,
                    sweep, kGuardNames[which], g->member, off % idim + d->ims, (off / idim) % kdim + d->kms, off / (idim * kdim) + d->jms,
                    g->n_nonfinite);
}

int amt_diag_after_sweep(const char *who, amt_domain *d, int members)
{
    AmtDiagState &st = *d->diag;                      // set_guard made it
    if (++st.sweeps % d->guard_every) return AMT_OK;
    for (int f : kGuardFields) {
        AmtDiagBox box{};
        bool empty = false;
        int rc = diag_region(who, d, f, AMT_REGION_WINDOW, members, box, &empty);
        if (rc) return rc;
        if (empty) continue;
        diag_shape(box, d->dtype_bytes);
        AmtDiagGuard g;
        g.member_finding = st.member_finding;
        g.launch_ticket = st.tickets + st.members;
        g.found = st.tickets + st.members + 1;
        g.rec = st.guard;
        g.sweep = st.sweeps;
        g.field = f;
        rc = d->dtype_bytes == 8 ? diag_launch<double, false>(d->stream, st, d->field[f], nullptr, box, members, nullptr, g)
                                 : diag_launch<float, false>(d->stream, st, d->field[f], nullptr, box, members, nullptr, g);
        if (rc) return rc;
    }
    ++st.checked;
    return AMT_OK;
}

void amt_diag_release(amt_domain *d)
{
    if (!d->diag) return;
    d->diag->release();
    delete d->diag;
    d->diag = nullptr;
    d->guard_every = 0;
}

// the same checks for the passes that keep no member axis in their grid (amt_moments.hip): any member count
static void diag_box_out(const AmtDiagBox &b, AmtBox *box)
{
    *box = AmtBox{b.idim, b.jstride, b.mstride, b.first, b.ni, b.nk, b.nj};
}
int amt_box_plan(const char *who, int rank, int members, int ims, int ime, int jms, int jme, int kms, int kme,
                 int i0, int i1, int k0, int k1, int j0, int j1, AmtBox *box)
{
    AmtDiagBox b{};
    const int rc = diag_plan(who, rank, members, DiagExtents{ims, ime, jms, jme, kms, kme}, DiagBoxArg{i0, i1, k0, k1, j0, j1}, b, INT_MAX);
    if (rc == AMT_OK) diag_box_out(b, box);
    return rc;
}
int amt_box_region(const char *who, const amt_domain *d, int field, int region, int members, AmtBox *box, bool *empty)
{
    AmtDiagBox b{};
    const int rc = diag_region(who, d, field, region, members, b, empty, INT_MAX);
    if (rc == AMT_OK && !*empty) diag_box_out(b, box);
    return rc;
}

#define AMT_DIAG_BOX_SIG int ims, int ime, int jms, int jme, int kms, int kme, int i0, int i1, int k0, int k1, int j0, int j1
#define AMT_DIAG_BOX_ARGS DiagExtents{ims, ime, jms, jme, kms, kme}, DiagBoxArg{i0, i1, k0, k1, j0, j1}

extern "C" int amt_stats_device_f32(void *hip_stream, const float *a, int rank, int members, AMT_DIAG_BOX_SIG, amt_field_stats *out)
{
    return diag_device_call("amt_stats_device_f32", hip_stream, 4, false, a, nullptr, rank, members, AMT_DIAG_BOX_ARGS, out);
}
extern "C" int amt_stats_device_f64(void *hip_stream, const double *a, int rank, int members, AMT_DIAG_BOX_SIG, amt_field_stats *out)
{
    return diag_device_call("amt_stats_device_f64", hip_stream, 8, false, a, nullptr, rank, members, AMT_DIAG_BOX_ARGS, out);
}
extern "C" int amt_compare_device_f32(void *hip_stream, const float *a, const float *b, int rank, int members, AMT_DIAG_BOX_SIG, amt_field_diff *out)
{
    return diag_device_call("amt_compare_device_f32", hip_stream, 4, true, a, b, rank, members, AMT_DIAG_BOX_ARGS, out);
}
extern "C" int amt_compare_device_f64(void *hip_stream, const double *a, const double *b, int rank, int members, AMT_DIAG_BOX_SIG, amt_field_diff *out)
{
    return diag_device_call("amt_compare_device_f64", hip_stream, 8, true, a, b, rank, members, AMT_DIAG_BOX_ARGS, out);
}

extern "C" int amt_domain_field_stats(amt_domain *d, int field, int region, amt_field_stats *out)
{
    return handle_stats("amt_domain_field_stats", d, 1, field, region, out);
}
extern "C" int amt_ensemble_field_stats(amt_ensemble *e, int field, int region, amt_field_stats *out)
{
    return handle_stats("amt_ensemble_field_stats", e ? &e->d : nullptr, e ? e->members : 1, field, region, out);
}
extern "C" int amt_domain_compare(amt_domain *a, amt_domain *b, int field, int region, amt_field_diff *out)
{
    return handle_compare("amt_domain_compare", a, b, 1, 1, field, region, out);
}
extern "C" int amt_ensemble_compare(amt_ensemble *a, amt_ensemble *b, int field, int region, amt_field_diff *out)
{
    return handle_compare("amt_ensemble_compare", a ? &a->d : nullptr, b ? &b->d : nullptr, a ? a->members : 1, b ? b->members : 1,
                          field, region, out);
}
extern "C" int amt_domain_set_guard(amt_domain *d, int every) { return handle_set_guard("amt_domain_set_guard", d, 1, every); }
extern "C" int amt_ensemble_set_guard(amt_ensemble *e, int every)
{
    return handle_set_guard("amt_ensemble_set_guard", e ? &e->d : nullptr, e ? e->members : 1, every);
}
extern "C" int amt_domain_guard_report(amt_domain *d, amt_guard_report *out) { return handle_guard_report("amt_domain_guard_report", d, out); }
extern "C" int amt_ensemble_guard_report(amt_ensemble *e, amt_guard_report *out)
{
    return handle_guard_report("amt_ensemble_guard_report", e ? &e->d : nullptr, out);
}
