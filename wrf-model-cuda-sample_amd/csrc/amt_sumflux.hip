// amt_sumflux.hip -- the acoustic loop's flux averages on the device (include/amt_advance_mu_t.h section 14, DESIGN.md
// section 7.7).  In WRF's solve_em every acoustic sub-step ends with sumflux: u, v and ww of the sub-step are added into the
// time-averaged mass fluxes ru_m, rv_m, ww_m, and the last sub-step turns the sums into the averages that scalar advection uses:
//   s = (iteration == 1) ? 0 + x : acc + x;      iteration < n:  acc = s
//   iteration == n, q = s / n:   ru_m = q + (muu * u_1) / msfuy;   rv_m = q + (muv * v_1) * msfvx_inv;   ww_m = q + ww_1
// every operation rounded once in the arrays' type (the library is built with -ffp-contract=off).  Each accumulator has its
// own range inside the tile box its..ite, kts..kte, jts..jte (ru_m: all of i, rv_m: all of j, ww_m: all of k; otherwise
// one short of the domain's end); at iteration 1 the tile's cells outside it become +0.0.  ONE launch does the three
// accumulators, times the members of an ensemble.  A separate streaming pass behind the sweep: the march kernel is not touched.
#include "amt_internal.h"
#include "amt_chunk_io.h"

namespace {
enum { AMT_SUMFLUX_JOBS = 3 };              // ru_m, rv_m, ww_m

// Job q works on the tile box of its accumulator: nk * nj runs of `ni` contiguous elements, run r = (k, j) = (r % nk, r / nk)
// of member m starting at element m * mstride3 + j * jstride3 + k * idim + first3 of acc, x and x1 alike (the three 3-D arrays
// of a job have one layout) and at m * mstride2 + j * idim + first2 of the two 2-D factors.  Element (i, k, j) of the box is
// in the accumulator's range when i < ilen[q], k < klen[q] and j < jlen[q].
template <typename T>
struct AmtSumfluxJobs {
    T *acc[AMT_SUMFLUX_JOBS];
    const T *x[AMT_SUMFLUX_JOBS], *x1[AMT_SUMFLUX_JOBS];
    const T *fa[AMT_SUMFLUX_JOBS], *fb[AMT_SUMFLUX_JOBS];          // muu, msfuy / muv, msfvx_inv / none
    int ilen[AMT_SUMFLUX_JOBS], klen[AMT_SUMFLUX_JOBS], jlen[AMT_SUMFLUX_JOBS];
    int ni, nk, nj;
    long idim, jstride3, mstride3, mstride2, first3, first2;
    T n;                                                           // n_small_steps in the arrays' type
    int first, last;                                               // iteration == 1, iteration == n
};

// what the last sub-step adds to the average: job 0 (muu * u_1) / msfuy, job 1 (muv * v_1) * msfvx_inv, job 2 ww_1
template <typename T>
__device__ __forceinline__ T amt_sumflux_base(int q, T x1, T fa, T fb)
{
    if (q == 2) return x1;
    const T p = fa * x1;
    return q == 0 ? p / fb : p * fb;
}

// Grid (blocks, 3 jobs, members).  A work item is one 16-byte chunk of a run (its last chunk may be short), lanes run along
// (chunk, k, j): along i first, so that every stream of a wave is coalesced.  `live` of a chunk's `cnt` elements lie inside
// the accumulator's range: none in a run outside it in k or j, all but the cell past it in i otherwise.  Load, add, average and
// store happen over `live`, once, on the lanes of a vector (amt_chunk_io.h); at the first iteration the tile's elements
// live..cnt-1 become +0.0, otherwise they are not touched.  A chunk moves as ONE 16-byte access per 3-D stream where it is
// whole, all or none of it is live and every address it touches lies on a 16-byte boundary (decided per chunk, behind the
// member offset); every other chunk goes element by element.  The 2-D factors are loaded at the last iteration only.
// Nothing outside the tile box is read or written.  Offsets are 64-bit.  256 threads, no LDS.
template <typename T>
__global__ __launch_bounds__(256) void amt_sumflux_kernel(AmtSumfluxJobs<T> jobs)
{
    typedef typename AmtVec16<T>::type V;
    constexpr int kPer = 16 / (int)sizeof(T);
    const int q = blockIdx.y;
    const long moff3 = (long)blockIdx.z * jobs.mstride3 + jobs.first3, moff2 = (long)blockIdx.z * jobs.mstride2 + jobs.first2;
    T *acc = jobs.acc[q] + moff3;
    const T *x = jobs.x[q] + moff3, *x1 = jobs.x1[q] + moff3;
    const T *fa = q == 2 ? nullptr : jobs.fa[q] + moff2, *fb = q == 2 ? nullptr : jobs.fb[q] + moff2;
    const bool first = jobs.first != 0, last = jobs.last != 0;
    const T n = jobs.n;
    const long ni = jobs.ni, nk = jobs.nk, ilen = jobs.ilen[q];
    const int klen = jobs.klen[q], jlen = jobs.jlen[q];
    const long chunks = (ni + kPer - 1) / kPer;
    const long total = nk * (long)jobs.nj * chunks;
    const bool narrow = total <= 0x7fffffffL;                      // wave-uniform: 32-bit divisions where they suffice
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const AmtChunk c = amt_chunk_index<kPer>(e, chunks, nk, ni, narrow);
        const long at3 = c.j * jobs.jstride3 + c.k * jobs.idim + c.i0, at2 = c.j * jobs.idim + c.i0;
        const int cnt = c.cnt;
        const long in = c.k >= klen || c.j >= jlen ? 0 : ilen - c.i0;
        const int live = in < 0 ? 0 : in < cnt ? (int)in : cnt;
        if (live == 0 && !first) continue;                         // nothing of the range: only the first iteration zeroes it
        T *a = acc + at3;
        const T *xs = x + at3, *x1s = x1 + at3;
        uintptr_t bits = reinterpret_cast<uintptr_t>(a);
        if (live) bits |= reinterpret_cast<uintptr_t>(xs);
        if (live && last) bits |= reinterpret_cast<uintptr_t>(x1s);
        const bool wide = cnt == kPer && (live == kPer || live == 0) && (bits & 15) == 0;
        V s = T(0);
        if (live) {
            // every load of the chunk is issued before the first use of one
            V b = s, f0 = s, f1 = s;                               // not used unless loaded: job 2 has no factors
            const V xv = amt_chunk_load<T>(xs, wide, live);
            if (!first) s = amt_chunk_load<T>(a, wide, live);
            if (last) {
                b = amt_chunk_load<T>(x1s, wide, live);
                if (q != 2) {
                    f0 = amt_chunk_load<T>(fa + at2, false, live);
                    f1 = amt_chunk_load<T>(fb + at2, false, live);
                }
            }
            for (int i = 0; i < kPer; ++i) s[i] = s[i] + xv[i];    // T(0) + x at the first iteration: -0.0 becomes +0.0
            if (last)
                for (int i = 0; i < kPer; ++i) {
                    const T avg = s[i] / n;
                    s[i] = avg + amt_sumflux_base<T>(q, b[i], f0[i], f1[i]);
                }
        }
        if (first)                                                 // the tile's cells outside the range
            for (int i = 0; i < kPer; ++i) s[i] = i < live ? s[i] : T(0);
        amt_chunk_store<T>(a, wide, first ? cnt : live, s);
    }
}

struct SumfluxArrays {
    void *ru_m, *rv_m, *ww_m;
    const void *u, *v, *ww, *u_1, *v_1, *ww_1, *muu, *muv, *msfuy, *msfvx_inv;
};

// a tile with one level holds cells of ww_m, one whose mass range is empty holds cells of ru_m or rv_m
const AmtPassRules kSumfluxRules = {1, false, "two accumulators overlap", "an accumulator overlaps an input array"};

// Argument and precondition checks (amt_pass.h): host arithmetic only.  *empty: the tile box holds no cell (nothing to do).
int sumflux_check(const char *who, const amt_domain &s, int members, const SumfluxArrays &a, int iteration, int n, bool *empty)
{
    // an accumulator may overlap no other array of the call (the inputs may alias one another)
    const AmtPassArray arr[13] = {{a.ru_m, 3, true, false}, {a.rv_m, 3, true, false}, {a.ww_m, 3, true, false}, {a.u, 3, false, false},
                                  {a.v, 3, false, false}, {a.ww, 3, false, false}, {a.u_1, 3, false, false}, {a.v_1, 3, false, false},
                                  {a.ww_1, 3, false, false}, {a.muu, 2, false, false}, {a.muv, 2, false, false}, {a.msfuy, 2, false, false},
                                  {a.msfvx_inv, 2, false, false}};
    const int rc = amt_pass_check_arrays(who, members, arr, 13);
    if (rc) return rc;
    if (n < 1) return amt_fail(AMT_ERR_INVALID_ARG, "%s: n_small_steps = %d: an acoustic loop has at least one sub-step", who, n);
    if (iteration < 1 || iteration > n) return amt_fail(AMT_ERR_INVALID_ARG, "%s: iteration %d is not in 1..%d", who, iteration, n);
    return amt_pass_check_box(who, s, members, arr, 13, kSumfluxRules, empty);
}

template <typename T>
int sumflux_launch(const amt_domain &d, int members, const SumfluxArrays &a, int iteration, int n)
{
    AmtSumfluxJobs<T> jobs{};
    jobs.acc[0] = static_cast<T *>(a.ru_m); jobs.x[0] = static_cast<const T *>(a.u); jobs.x1[0] = static_cast<const T *>(a.u_1);
    jobs.acc[1] = static_cast<T *>(a.rv_m); jobs.x[1] = static_cast<const T *>(a.v); jobs.x1[1] = static_cast<const T *>(a.v_1);
    jobs.acc[2] = static_cast<T *>(a.ww_m); jobs.x[2] = static_cast<const T *>(a.ww); jobs.x1[2] = static_cast<const T *>(a.ww_1);
    jobs.fa[0] = static_cast<const T *>(a.muu); jobs.fb[0] = static_cast<const T *>(a.msfuy);
    jobs.fa[1] = static_cast<const T *>(a.muv); jobs.fb[1] = static_cast<const T *>(a.msfvx_inv);
    jobs.ni = d.ite - d.its + 1; jobs.nk = d.kte - d.kts + 1; jobs.nj = d.jte - d.jts + 1;
    int imass, jmass;                                              // may be <= 0: no cell of the range
    amt_pass_mass_lengths(d, &imass, &jmass);
    jobs.ilen[0] = jobs.ni; jobs.klen[0] = jobs.nk - 1; jobs.jlen[0] = jmass;
    jobs.ilen[1] = imass;   jobs.klen[1] = jobs.nk - 1; jobs.jlen[1] = jobs.nj;
    jobs.ilen[2] = imass;   jobs.klen[2] = jobs.nk;     jobs.jlen[2] = jmass;
    amt_pass_set_layout(d, jobs);
    jobs.n = (T)n;
    jobs.first = iteration == 1; jobs.last = iteration == n;
    constexpr long per = 16 / (long)sizeof(T);
    const long total = (long)jobs.nk * jobs.nj * ((jobs.ni + per - 1) / per);
    hipLaunchKernelGGL(amt_sumflux_kernel<T>, dim3(amt_pass_blocks(total), AMT_SUMFLUX_JOBS, (unsigned)members), dim3(256), 0, d.stream, jobs);
    AMT_HIP(hipGetLastError());
    return AMT_OK;
}

// the checks, then the launch (amt_pass_run)
int sumflux_run(const char *who, const amt_domain &d, int members, const SumfluxArrays &a, int iteration, int n, bool pointer_level)
{
    bool empty = false;
    const int rc = sumflux_check(who, d, members, a, iteration, n, &empty);
    return amt_pass_run(rc, empty, d, pointer_level, [&](auto t) { return sumflux_launch<decltype(t)>(d, members, a, iteration, n); });
}

SumfluxArrays sumflux_of_domain(const amt_domain *d)
{
    return SumfluxArrays{d->sumflux_acc[0], d->sumflux_acc[1], d->sumflux_acc[2], d->field[AMT_F_U], d->field[AMT_F_V], d->field[AMT_F_WW],
                         d->field[AMT_F_U_1], d->field[AMT_F_V_1], d->field[AMT_F_WW_1], d->field[AMT_F_MUU], d->field[AMT_F_MUV],
                         d->field[AMT_F_MSFUY], d->field[AMT_F_MSFVX_INV]};
}

// the three accumulators in the handle: one 3-D field's extents each, times the members
AmtPassSetting sumflux_setting(amt_domain *d, int members)
{
    const size_t bytes = d->count(AMT_F_WW) * (size_t)members * (size_t)d->dtype_bytes;
    return AmtPassSetting{d->sumflux_acc, &d->sumflux_owned, 3, {bytes, bytes, bytes}, "three accumulators", "an accumulator",
                          "the flux averages", "three arrays"};
}
}  // namespace

// what the handles and the steppers call: one accumulation of `members` member-stacked patches of the domain's shape, on the
// domain's stream; the counter goes 1..n and wraps.  Off (n == 0): AMT_ERR_INVALID_ARG.
int amt_sumflux_accumulate_domain(const char *who, amt_domain *d, int members)
{
    if (d->sumflux_n < 1) return amt_fail(AMT_ERR_INVALID_ARG, "%s: the flux averages are off (amt_*_set_sumflux)", who);
    const int rc = sumflux_run(who, *d, members, sumflux_of_domain(d), d->sumflux_next, d->sumflux_n, false);
    if (rc == AMT_OK) d->sumflux_next = d->sumflux_next == d->sumflux_n ? 1 : d->sumflux_next + 1;
    return rc;
}

void amt_sumflux_release(amt_domain *d)
{
    amt_pass_setting_release(sumflux_setting(d, 1));
    d->sumflux_n = 0;
    d->sumflux_next = 1;
}

// amt_*_set_sumflux.  A refusal changes nothing.
int amt_sumflux_set_domain(const char *who, amt_domain *d, int members, int n, void *ru_m, void *rv_m, void *ww_m)
{
    if (n < 0) return amt_fail(AMT_ERR_INVALID_ARG, "%s: n_small_steps = %d", who, n);
    if (n == 0) { amt_sumflux_release(d); return AMT_OK; }
    void *const acc[3] = {ru_m, rv_m, ww_m};
    const AmtPassSetting s = sumflux_setting(d, members);
    int given;
    bool same;                                                     // the library's own arrays handed back (amt_*_sumflux_ptr): they stay
    int rc = amt_pass_setting_offer(who, s, acc, &given, &same);
    if (rc) return rc;
    rc = amt_pass_setting_take(who, d, members, s, acc, given, same, [&](void *const *arr) {
        amt_domain probe = *d;
        memcpy(probe.sumflux_acc, arr, sizeof probe.sumflux_acc);
        bool empty = false;
        return sumflux_check(who, probe, members, sumflux_of_domain(&probe), 1, n, &empty);
    });
    if (rc) return rc;
    d->sumflux_n = n;                                              // also for the library's own arrays: n and the counter are set anew
    d->sumflux_next = 1;
    return AMT_OK;
}

#define AMT_SUMFLUX_SIG(T)                                                                                     \
    void *hip_stream, int members, T *ru_m, T *rv_m, T *ww_m, const T *u, const T *v, const T *ww,             \
    const T *u_1, const T *v_1, const T *ww_1, const T *muu, const T *muv, const T *msfuy, const T *msfvx_inv, \
    int iteration, int n_small_steps, AMT_BOUNDS_SIG
#define AMT_SUMFLUX_BODY(T, name)                                                                              \
    return sumflux_run(name, amt_pass_domain((int)sizeof(T), hip_stream, AMT_BOUNDS_ARGS), members,            \
                       SumfluxArrays{ru_m, rv_m, ww_m, u, v, ww, u_1, v_1, ww_1, muu, muv, msfuy, msfvx_inv}, iteration, n_small_steps, true);

extern "C" int amt_sumflux_device_f32(AMT_SUMFLUX_SIG(float)) { AMT_SUMFLUX_BODY(float, "amt_sumflux_device_f32") }
extern "C" int amt_sumflux_device_f64(AMT_SUMFLUX_SIG(double)) { AMT_SUMFLUX_BODY(double, "amt_sumflux_device_f64") }

// ---- the handles -------------------------------------------------------------------------------------------------------
extern "C" int amt_domain_set_sumflux(amt_domain *d, int n_small_steps, void *ru_m, void *rv_m, void *ww_m)
{
    if (!d) return amt_fail(AMT_ERR_INVALID_ARG, "null domain");
    DeviceScope scope(d->device);
    return amt_sumflux_set_domain("amt_domain_set_sumflux", d, 1, n_small_steps, ru_m, rv_m, ww_m);
}

extern "C" int amt_domain_sumflux_accumulate(amt_domain *d)
{
    if (!d) return amt_fail(AMT_ERR_INVALID_ARG, "null domain");
    DeviceScope scope(d->device);
    return amt_sumflux_accumulate_domain("amt_domain_sumflux_accumulate", d, 1);
}

extern "C" int amt_domain_sumflux_state(const amt_domain *d, int *n, int *next_iteration)
{
    if (!d) return amt_fail(AMT_ERR_INVALID_ARG, "null domain");
    if (n) *n = d->sumflux_n;
    if (next_iteration) *next_iteration = d->sumflux_next;
    return AMT_OK;
}

extern "C" void *amt_domain_sumflux_ptr(amt_domain *d, int which)
{
    if (!d || which < 0 || which > 2) return nullptr;
    return d->sumflux_acc[which];
}

extern "C" int amt_ensemble_set_sumflux(amt_ensemble *e, int n_small_steps, void *ru_m, void *rv_m, void *ww_m)
{
    if (!e) return amt_fail(AMT_ERR_INVALID_ARG, "null ensemble");
    DeviceScope scope(e->d.device);
    return amt_sumflux_set_domain("amt_ensemble_set_sumflux", &e->d, e->members, n_small_steps, ru_m, rv_m, ww_m);
}

extern "C" int amt_ensemble_sumflux_accumulate(amt_ensemble *e)
{
    if (!e) return amt_fail(AMT_ERR_INVALID_ARG, "null ensemble");
    DeviceScope scope(e->d.device);
    return amt_sumflux_accumulate_domain("amt_ensemble_sumflux_accumulate", &e->d, e->members);
}

extern "C" int amt_ensemble_sumflux_state(const amt_ensemble *e, int *n, int *next_iteration)
{
    if (!e) return amt_fail(AMT_ERR_INVALID_ARG, "null ensemble");
    return amt_domain_sumflux_state(&e->d, n, next_iteration);
}

extern "C" void *amt_ensemble_sumflux_ptr(amt_ensemble *e, int which) { return e ? amt_domain_sumflux_ptr(&e->d, which) : nullptr; }
