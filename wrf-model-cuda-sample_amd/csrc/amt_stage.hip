// amt_stage.hip -- the bracket of a Runge-Kutta stage on the device (include/amt_advance_mu_t.h section 15, DESIGN.md
// section 7.8).  In WRF's solve_em every Runge-Kutta stage opens its acoustic loop with small_step_prep, which turns the full
// fields into the perturbation form advance_mu_t works on, and closes it with small_step_finish, which turns them back.  For
// the arrays this library owns (t = t_2, t_1 = t_save, ww_1 = ww1, mu = mu_2; t_old = WRF's t_1, mu_old = WRF's mu_1):
//   prep, rk_step == 1:  mu_old = m; muts = mub + m; mu_save = m; mu = m - m; mudf = 0          (m the old mu)
//         rk_step  > 1:  muts = mub + mu_old; mu_save = m; mu = mu_old - m
//         cells:         [t_old = x;]  t_1 = x;  t = (s * t_old) - (mut * x);   ww_1 = ww        (x the old t, s the NEW muts)
//   finish:              t = ((t - ((dts * n) * mut) * h_diabatic) + (t_1 * mut)) / muts    or   t = (t + (t_1 * mut)) / muts
//                        ww = ww + ww_1;  mu = mu + mu_save
// over the columns its..min(ite, ide-1), jts..min(jte, jde-1), t on levels kts..kte-1 and ww on kts..kte; every operation
// rounded once in the arrays' type (the library is built with -ffp-contract=off), copies are bit copies.
// The 3-D pass of prep needs the OLD mu and works out s = mub + m itself -- the same rounding as the stored muts --, while the
// 2-D pass overwrites mu, mu_old, mu_save and muts: in one launch the two would race between workgroups.  So prep is TWO
// launches in stream order, the 3-D pass first (it never reads the stored muts), and finish, which has no such dependency, is
// ONE.  Separate streaming passes around the acoustic loop: the march kernel is not touched.
#include "amt_internal.h"
#include "amt_chunk_io.h"

namespace {
// A job works on a box of nk * nj runs of `ni` contiguous elements, run r = (k, j) = (r % nk, r / nk) of member m starting at
// element m * mstride3 + j * jstride3 + k * idim + first3 of every 3-D array (they have one layout) and at
// m * mstride2 + j * idim + first2 of every 2-D array.  Job t covers the levels kts..kte-1 (nk - 1 of them), job ww all nk;
// the 2-D job is one run per row j.
template <typename T>
struct AmtStageJobs {
    T *t, *t_1, *t_old, *ww, *ww_1;
    T *mu, *mu_old, *mu_save, *muts, *mudf;
    const T *mut, *mub, *h;
    int ni, nk, nj;
    long idim, jstride3, mstride3, mstride2, first3, first2;
    T c;                                                           // finish: dts * T(n_small_steps), rounded once in T
    int first, with_h;                                             // rk_step == 1; h_diabatic given
};

// Work item e of a 3-D job: one 16-byte chunk of a run, counted from the run's first element (the run's last chunk may be
// short); lanes run along (chunk, k, j), along i first, so that every stream of a wave is coalesced.  Offsets are 64-bit.
template <int kPer>
__device__ __forceinline__ void amt_stage_chunk(long e, long chunks, long nk, long ni, bool narrow, long idim, long jstride3,
                                                long &at3, long &at2, int &cnt)
{
    const AmtChunk c = amt_chunk_index<kPer>(e, chunks, nk, ni, narrow);   // narrow is wave-uniform
    at3 = c.j * jstride3 + c.k * idim + c.i0;
    at2 = c.j * idim + c.i0;
    cnt = c.cnt;
}

// The common 16-byte phase of a job's 3-D streams behind the member offset (wave-uniform), or -1 where they differ.  A chunk at
// element offset `at` has ALL its 3-D addresses on a 16-byte boundary exactly when the phase is common and phase + at * sizeof(T)
// is a multiple of 16.
__device__ __forceinline__ int amt_stage_phase(const void *a, const void *b, const void *c)
{
    const int pa = (int)(reinterpret_cast<uintptr_t>(a) & 15), pb = (int)(reinterpret_cast<uintptr_t>(b) & 15), pc = (int)(reinterpret_cast<uintptr_t>(c) & 15);
    return pa == pb && pa == pc ? pa : -1;
}
template <typename T>
__device__ __forceinline__ bool amt_stage_aligned(int phase, long at)
{
    return phase >= 0 && (((long)phase + at * (long)sizeof(T)) & 15) == 0;
}

// what prep stores into t: two products, then one subtraction
template <typename T>
__device__ __forceinline__ T amt_stage_prep_t(T s, T told, T mut, T x)
{
    const T a = s * told, b = mut * x;
    return a - b;
}

// what finish stores into t; c = dts * T(n)
template <typename T>
__device__ __forceinline__ T amt_stage_finish_t(bool with_h, T x, T c, T mut, T h, T t1, T muts)
{
    T acc = x;
    if (with_h) {
        const T a = c * mut;
        const T b = a * h;
        acc = x - b;
    }
    const T e = t1 * mut;
    const T f = acc + e;
    return f / muts;
}

// The 3-D pass of prep.  Grid (blocks, 2 jobs, members): job 0 is t (reads mu or mu_old, mub, mut; never muts), job 1 the copy
// ww_1 = ww.  A whole chunk moves as ONE 16-byte access per 3-D stream where all the 3-D addresses it touches lie on a 16-byte
// boundary (decided per chunk from the streams' common phase behind the member offset); a run's short last chunk and every other
// chunk go element by element.  Either way the chunk lives in the lanes of one vector (amt_chunk_io.h) and the arithmetic is
// stated once.  The 2-D operands are loaded element by element, for the chunk's own elements only.  256 threads, no LDS.
template <typename T>
__global__ __launch_bounds__(256) void amt_stage_prep3_kernel(AmtStageJobs<T> jobs)
{
    typedef typename AmtVec16<T>::type V;
    constexpr int kPer = 16 / (int)sizeof(T);
    const int q = blockIdx.y;
    const long moff3 = (long)blockIdx.z * jobs.mstride3 + jobs.first3, moff2 = (long)blockIdx.z * jobs.mstride2 + jobs.first2;
    const bool first = jobs.first != 0;
    const long ni = jobs.ni, nk = q == 0 ? jobs.nk - 1 : jobs.nk;
    const long chunks = (ni + kPer - 1) / kPer;
    const long total = nk * (long)jobs.nj * chunks;
    const bool narrow = total <= 0x7fffffffL;
    if (q == 1) {                                                  // ww_1 = ww
        const T *ww = jobs.ww + moff3;
        T *ww_1 = jobs.ww_1 + moff3;
        const int phase = amt_stage_phase(ww, ww_1, ww);
        for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
            long at3, at2;
            int cnt;
            amt_stage_chunk<kPer>(e, chunks, nk, ni, narrow, jobs.idim, jobs.jstride3, at3, at2, cnt);
            const bool wide = cnt == kPer && amt_stage_aligned<T>(phase, at3);
            amt_chunk_store<T>(ww_1 + at3, wide, cnt, amt_chunk_load<T>(ww + at3, wide, cnt));
        }
        return;
    }
    const T *m2 = (first ? jobs.mu : jobs.mu_old) + moff2, *mub = jobs.mub + moff2, *mut = jobs.mut + moff2;
    T *t = jobs.t + moff3, *t_1 = jobs.t_1 + moff3, *t_old = jobs.t_old + moff3;
    const int phase = amt_stage_phase(t, t_1, t_old);
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        long at3, at2;
        int cnt;
        amt_stage_chunk<kPer>(e, chunks, nk, ni, narrow, jobs.idim, jobs.jstride3, at3, at2, cnt);
        const bool wide = cnt == kPer && amt_stage_aligned<T>(phase, at3);
        // every load of the chunk is issued before the first use of one
        V old = T(0), out;
        if (!first) old = amt_chunk_load<T>(t_old + at3, wide, cnt);
        const V x = amt_chunk_load<T>(t + at3, wide, cnt);
        const V b = amt_chunk_load<T>(mub + at2, false, cnt), m = amt_chunk_load<T>(m2 + at2, false, cnt);
        const V mt = amt_chunk_load<T>(mut + at2, false, cnt);
        for (int i = 0; i < kPer; ++i) {
            const T s = b[i] + m[i];
            out[i] = amt_stage_prep_t<T>(s, first ? x[i] : old[i], mt[i], x[i]);
        }
        if (first) amt_chunk_store<T>(t_old + at3, wide, cnt, x);
        amt_chunk_store<T>(t_1 + at3, wide, cnt, x);
        amt_chunk_store<T>(t + at3, wide, cnt, out);
    }
}

// The 2-D pass of prep, behind the 3-D pass in stream order.  Grid (blocks, 1, members), one column per lane, lanes along i.
template <typename T>
__global__ __launch_bounds__(256) void amt_stage_prep2_kernel(AmtStageJobs<T> jobs)
{
    const long moff2 = (long)blockIdx.z * jobs.mstride2 + jobs.first2;
    const bool first = jobs.first != 0;
    const long ni = jobs.ni, total = ni * (long)jobs.nj;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long j = e / ni;
        const long at = moff2 + j * jobs.idim + (e - j * ni);
        const T m = jobs.mu[at];
        if (first) {
            jobs.mu_old[at] = m;
            jobs.muts[at] = jobs.mub[at] + m;
            jobs.mu_save[at] = m;
            jobs.mu[at] = m - m;
            jobs.mudf[at] = T(0);
        } else {
            const T old = jobs.mu_old[at];
            jobs.muts[at] = jobs.mub[at] + old;
            jobs.mu_save[at] = m;
            jobs.mu[at] = old - m;
        }
    }
}

// finish.  Grid (blocks, 3 jobs, members): job 0 is t, job 1 ww = ww + ww_1 (chunks as in the 3-D pass of prep), job 2
// mu = mu + mu_save (one column per lane).  No job reads what another writes.
template <typename T>
__global__ __launch_bounds__(256) void amt_stage_finish_kernel(AmtStageJobs<T> jobs)
{
    typedef typename AmtVec16<T>::type V;
    constexpr int kPer = 16 / (int)sizeof(T);
    const int q = blockIdx.y;
    const long moff3 = (long)blockIdx.z * jobs.mstride3 + jobs.first3, moff2 = (long)blockIdx.z * jobs.mstride2 + jobs.first2;
    const long ni = jobs.ni;
    if (q == 2) {
        const long total = ni * (long)jobs.nj;
        for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
            const long j = e / ni;
            const long at = moff2 + j * jobs.idim + (e - j * ni);
            jobs.mu[at] = jobs.mu[at] + jobs.mu_save[at];
        }
        return;
    }
    const bool with_h = jobs.with_h != 0;
    const T c = jobs.c;
    const long nk = q == 0 ? jobs.nk - 1 : jobs.nk;
    const long chunks = (ni + kPer - 1) / kPer;
    const long total = nk * (long)jobs.nj * chunks;
    const bool narrow = total <= 0x7fffffffL;
    if (q == 1) {                                                  // ww = ww + ww_1
        T *ww = jobs.ww + moff3;
        const T *ww_1 = jobs.ww_1 + moff3;
        const int phase = amt_stage_phase(ww, ww_1, ww);
        for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
            long at3, at2;
            int cnt;
            amt_stage_chunk<kPer>(e, chunks, nk, ni, narrow, jobs.idim, jobs.jstride3, at3, at2, cnt);
            const bool wide = cnt == kPer && amt_stage_aligned<T>(phase, at3);
            V a = amt_chunk_load<T>(ww + at3, wide, cnt);
            const V b = amt_chunk_load<T>(ww_1 + at3, wide, cnt);
            for (int i = 0; i < kPer; ++i) a[i] = a[i] + b[i];
            amt_chunk_store<T>(ww + at3, wide, cnt, a);
        }
        return;
    }
    const T *mut = jobs.mut + moff2, *muts = jobs.muts + moff2;
    T *t = jobs.t + moff3;
    const T *t_1 = jobs.t_1 + moff3, *h = with_h ? jobs.h + moff3 : t_1;
    const int phase = amt_stage_phase(t, t_1, h);
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        long at3, at2;
        int cnt;
        amt_stage_chunk<kPer>(e, chunks, nk, ni, narrow, jobs.idim, jobs.jstride3, at3, at2, cnt);
        const bool wide = cnt == kPer && amt_stage_aligned<T>(phase, at3);
        V hv = T(0);                                               // every load is issued before the first use of one
        if (with_h) hv = amt_chunk_load<T>(h + at3, wide, cnt);
        V x = amt_chunk_load<T>(t + at3, wide, cnt);
        const V t1 = amt_chunk_load<T>(t_1 + at3, wide, cnt);
        const V mt = amt_chunk_load<T>(mut + at2, false, cnt), ms = amt_chunk_load<T>(muts + at2, false, cnt);
        for (int i = 0; i < kPer; ++i) x[i] = amt_stage_finish_t<T>(with_h, x[i], c, mt[i], hv[i], t1[i], ms[i]);
        amt_chunk_store<T>(t + at3, wide, cnt, x);
    }
}

// a tile with one level holds cells of ww and the columns of mu; one without a mass column holds nothing
const AmtPassRules kStageRules = {1, true, "an output array overlaps another array of the call", "an output array overlaps another array of the call"};

// Argument and precondition checks (amt_pass.h): host arithmetic only.  *empty: the range holds no column (nothing to do).
int stage_check(const char *who, const amt_domain &s, int members, const AmtPassArray *arr, int narr, const char *count_name, int count,
                bool *empty)
{
    const int rc = amt_pass_check_arrays(who, members, arr, narr);
    if (rc) return rc;
    if (count < 1) return amt_fail(AMT_ERR_INVALID_ARG, "%s: %s = %d: at least 1", who, count_name, count);
    return amt_pass_check_box(who, s, members, arr, narr, kStageRules, empty);
}

struct StagePrepArrays {
    void *t, *t_1, *t_old;
    const void *ww;
    void *ww_1, *mu, *mu_old, *mu_save, *muts, *mudf;
    const void *mut, *mub;
};
struct StageFinishArrays {
    void *t;
    const void *t_1;
    void *ww;
    const void *ww_1;
    void *mu;
    const void *mu_save, *muts, *mut, *h;
};

int stage_prep_check(const char *who, const amt_domain &d, int members, const StagePrepArrays &a, int rk_step, bool *empty)
{
    const bool first = rk_step == 1;
    // mudf at rk_step > 1 is neither read nor written: it takes no part in the checks
    const AmtPassArray arr[12] = {{a.t, 3, true, false}, {a.t_1, 3, true, false}, {a.t_old, 3, first, false},
                                  {a.ww, 3, false, false}, {a.ww_1, 3, true, false}, {a.mu, 2, true, false},
                                  {a.mu_old, 2, first, false}, {a.mu_save, 2, true, false}, {a.muts, 2, true, false},
                                  {first ? a.mudf : nullptr, 2, true, !first}, {a.mut, 2, false, false}, {a.mub, 2, false, false}};
    return stage_check(who, d, members, arr, 12, "rk_step", rk_step, empty);
}

int stage_finish_check(const char *who, const amt_domain &d, int members, const StageFinishArrays &a, int n, bool *empty)
{
    const AmtPassArray arr[9] = {{a.t, 3, true, false}, {a.t_1, 3, false, false}, {a.ww, 3, true, false},
                                 {a.ww_1, 3, false, false}, {a.mu, 2, true, false}, {a.mu_save, 2, false, false},
                                 {a.muts, 2, false, false}, {a.mut, 2, false, false}, {a.h, 3, false, true}};
    return stage_check(who, d, members, arr, 9, "n_small_steps", n, empty);
}

template <typename T>
void stage_box(const amt_domain &d, AmtStageJobs<T> &jobs)
{
    amt_pass_mass_lengths(d, &jobs.ni, &jobs.nj);
    jobs.nk = d.kte - d.kts + 1;
    amt_pass_set_layout(d, jobs);
}

template <typename T>
int stage_prep_launch(const amt_domain &d, int members, const StagePrepArrays &a, int rk_step)
{
    AmtStageJobs<T> jobs{};
    jobs.t = static_cast<T *>(a.t); jobs.t_1 = static_cast<T *>(a.t_1); jobs.t_old = static_cast<T *>(a.t_old);
    jobs.ww = static_cast<T *>(const_cast<void *>(a.ww)); jobs.ww_1 = static_cast<T *>(a.ww_1);
    jobs.mu = static_cast<T *>(a.mu); jobs.mu_old = static_cast<T *>(a.mu_old); jobs.mu_save = static_cast<T *>(a.mu_save);
    jobs.muts = static_cast<T *>(a.muts); jobs.mudf = static_cast<T *>(a.mudf);
    jobs.mut = static_cast<const T *>(a.mut); jobs.mub = static_cast<const T *>(a.mub);
    jobs.first = rk_step == 1;
    stage_box<T>(d, jobs);
    constexpr long per = 16 / (long)sizeof(T);
    const long most = (long)jobs.nk * jobs.nj * ((jobs.ni + per - 1) / per);               // job ww, the larger of the two
    hipLaunchKernelGGL(amt_stage_prep3_kernel<T>, dim3(amt_pass_blocks(most), 2, (unsigned)members), dim3(256), 0, d.stream, jobs);
    AMT_HIP(hipGetLastError());
    hipLaunchKernelGGL(amt_stage_prep2_kernel<T>, dim3(amt_pass_blocks((long)jobs.ni * jobs.nj), 1, (unsigned)members), dim3(256), 0, d.stream, jobs);
    AMT_HIP(hipGetLastError());
    return AMT_OK;
}

template <typename T>
int stage_finish_launch(const amt_domain &d, int members, const StageFinishArrays &a, double dts, int n)
{
    AmtStageJobs<T> jobs{};
    jobs.t = static_cast<T *>(a.t); jobs.t_1 = static_cast<T *>(const_cast<void *>(a.t_1));
    jobs.ww = static_cast<T *>(a.ww); jobs.ww_1 = static_cast<T *>(const_cast<void *>(a.ww_1));
    jobs.mu = static_cast<T *>(a.mu); jobs.mu_save = static_cast<T *>(const_cast<void *>(a.mu_save));
    jobs.muts = static_cast<T *>(const_cast<void *>(a.muts));
    jobs.mut = static_cast<const T *>(a.mut); jobs.h = static_cast<const T *>(a.h);
    jobs.with_h = a.h != nullptr;
    const T dts_t = (T)dts, n_t = (T)n;
    jobs.c = dts_t * n_t;
    stage_box<T>(d, jobs);
    constexpr long per = 16 / (long)sizeof(T);
    const long most = (long)jobs.nk * jobs.nj * ((jobs.ni + per - 1) / per);
    hipLaunchKernelGGL(amt_stage_finish_kernel<T>, dim3(amt_pass_blocks(most), 3, (unsigned)members), dim3(256), 0, d.stream, jobs);
    AMT_HIP(hipGetLastError());
    return AMT_OK;
}

// the checks, then the launch (amt_pass_run)
int stage_prep_run(const char *who, const amt_domain &d, int members, const StagePrepArrays &a, int rk_step, bool pointer_level)
{
    bool empty = false;
    const int rc = stage_prep_check(who, d, members, a, rk_step, &empty);
    return amt_pass_run(rc, empty, d, pointer_level, [&](auto t) { return stage_prep_launch<decltype(t)>(d, members, a, rk_step); });
}

int stage_finish_run(const char *who, const amt_domain &d, int members, const StageFinishArrays &a, double dts, int n, bool pointer_level)
{
    bool empty = false;
    const int rc = stage_finish_check(who, d, members, a, n, &empty);
    return amt_pass_run(rc, empty, d, pointer_level, [&](auto t) { return stage_finish_launch<decltype(t)>(d, members, a, dts, n); });
}

StagePrepArrays stage_prep_of_domain(const amt_domain *d)
{
    return StagePrepArrays{d->field[AMT_F_T], d->field[AMT_F_T_1], d->stage_arr[0], d->field[AMT_F_WW], d->field[AMT_F_WW_1],
                           d->field[AMT_F_MU], d->stage_arr[1], d->stage_arr[2], d->field[AMT_F_MUTS], d->field[AMT_F_MUDF],
                           d->field[AMT_F_MUT], d->stage_arr[3]};
}

// the four arrays in the handle: t_old one 3-D field's extents, mu_old, mu_save and mub one 2-D field's, times the members
AmtPassSetting stage_setting(amt_domain *d, int members)
{
    const size_t b3 = d->count(AMT_F_T) * (size_t)members * (size_t)d->dtype_bytes, b2 = d->count(AMT_F_MU) * (size_t)members * (size_t)d->dtype_bytes;
    return AmtPassSetting{d->stage_arr, &d->stage_owned, 4, {b3, b2, b2, b2}, "four arrays", "an array", "the stage bracket", "an array"};
}
}  // namespace

// ---- what the handles call (amt_handle_stage_* of amt_domain.hip) ---------------------------------------------------------
int amt_stage_prep_domain(const char *who, amt_domain *d, int members, int rk_step)
{
    if (!d->stage_on) return amt_fail(AMT_ERR_PRECONDITION, "%s: the stage bracket is off (amt_*_set_stage)", who);
    return stage_prep_run(who, *d, members, stage_prep_of_domain(d), rk_step, false);
}

int amt_stage_finish_domain(const char *who, amt_domain *d, int members, int n_small_steps, const void *h_diabatic)
{
    if (!d->stage_on) return amt_fail(AMT_ERR_PRECONDITION, "%s: the stage bracket is off (amt_*_set_stage)", who);
    const StageFinishArrays a{d->field[AMT_F_T], d->field[AMT_F_T_1], d->field[AMT_F_WW], d->field[AMT_F_WW_1], d->field[AMT_F_MU],
                              d->stage_arr[2], d->field[AMT_F_MUTS], d->field[AMT_F_MUT], h_diabatic};
    return stage_finish_run(who, *d, members, a, d->dts, n_small_steps, false);
}

void amt_stage_release(amt_domain *d)
{
    amt_pass_setting_release(stage_setting(d, 1));
    d->stage_on = false;
}

// amt_*_set_stage.  A refusal changes nothing.
int amt_stage_set_domain(const char *who, amt_domain *d, int members, int on, void *t_old, void *mu_old, void *mu_save, void *mub)
{
    if (!on) {
        DeviceScope scope(d->device);
        amt_stage_release(d);
        return AMT_OK;
    }
    void *const arr[4] = {t_old, mu_old, mu_save, mub};
    const AmtPassSetting s = stage_setting(d, members);
    int given;
    bool same;
    int rc = amt_pass_setting_offer(who, s, arr, &given, &same);
    if (rc) return rc;
    if (same) return AMT_OK;                                       // the library's own arrays handed back (amt_*_stage_ptr): nothing changes
    rc = amt_pass_setting_take(who, d, members, s, arr, given, same, [&](void *const *theirs) {
        amt_domain probe = *d;
        memcpy(probe.stage_arr, theirs, sizeof probe.stage_arr);
        bool empty = false;
        return stage_prep_check(who, probe, members, stage_prep_of_domain(&probe), 1, &empty);
    });
    if (rc) return rc;
    d->stage_on = true;
    return AMT_OK;
}

// ---- pointer level -------------------------------------------------------------------------------------------------------
#define AMT_STAGE_PREP_SIG(T)                                                                                   \
    void *hip_stream, int members, T *t, T *t_1, T *t_old, const T *ww, T *ww_1, T *mu, T *mu_old, T *mu_save,  \
    T *muts, T *mudf, const T *mut, const T *mub, int rk_step, AMT_BOUNDS_SIG
#define AMT_STAGE_FINISH_SIG(T)                                                                                 \
    void *hip_stream, int members, T *t, const T *t_1, T *ww, const T *ww_1, T *mu, const T *mu_save,           \
    const T *muts, const T *mut, T dts, int n_small_steps, const T *h_diabatic, AMT_BOUNDS_SIG
#define AMT_STAGE_PREP_BODY(T, name)                                                                            \
    return stage_prep_run(name, amt_pass_domain((int)sizeof(T), hip_stream, AMT_BOUNDS_ARGS), members,          \
                          StagePrepArrays{t, t_1, t_old, ww, ww_1, mu, mu_old, mu_save, muts, mudf, mut, mub}, rk_step, true);
#define AMT_STAGE_FINISH_BODY(T, name)                                                                          \
    return stage_finish_run(name, amt_pass_domain((int)sizeof(T), hip_stream, AMT_BOUNDS_ARGS), members,        \
                            StageFinishArrays{t, t_1, ww, ww_1, mu, mu_save, muts, mut, h_diabatic}, (double)dts, n_small_steps, true);

extern "C" int amt_stage_prep_device_f32(AMT_STAGE_PREP_SIG(float)) { AMT_STAGE_PREP_BODY(float, "amt_stage_prep_device_f32") }
extern "C" int amt_stage_prep_device_f64(AMT_STAGE_PREP_SIG(double)) { AMT_STAGE_PREP_BODY(double, "amt_stage_prep_device_f64") }
extern "C" int amt_stage_finish_device_f32(AMT_STAGE_FINISH_SIG(float)) { AMT_STAGE_FINISH_BODY(float, "amt_stage_finish_device_f32") }
extern "C" int amt_stage_finish_device_f64(AMT_STAGE_FINISH_SIG(double)) { AMT_STAGE_FINISH_BODY(double, "amt_stage_finish_device_f64") }
