// amt_p_rho.hip -- the pressure diagnosis that closes every acoustic sub-step, on the device (include/amt_advance_mu_t.h
// section 16).  In WRF's solve_em calc_p_rho follows every advance_mu_t (and small_step_prep, with
// step = 0): from t = t_2, t_old = t_1, mu = mu_2 and muts it diagnoses the inverse density al and the pressure p, and in its
// hydrostatic branch integrates the geopotential ph up the column.  For every cell of the columns its..min(ite, ide-1),
// jts..min(jte, jde-1), k = kts..kte-1:
//   q = (alt * (t - (mu * t_old))) / (muts * (t0 + t_old))
//   mode 1:  al = (T(-1) / muts) * ((alt * mu) + (rdnw(k) * (ph(k+1) - ph(k))));   p = c2a * (q - al)
//   mode 2:  p = mu * znu(k);   al = q - (p / c2a);   ph(k+1) = ph(k) - (dnw(k) * ((muts * al) + (mu * alt)))     k ascending
//   both:    x = p;  step == 0:  p = x, pm1 = x;   step != 0:  p = x + (smdiv * (x - pm1)), pm1 = x
// every operation rounded once in the arrays' type (the library is built with -ffp-contract=off), IEEE divides.
// One streaming pass in the family of amt_stage.hip and amt_sumflux.hip; unlike them a work item WALKS k: it owns one 16-byte
// chunk of a row (element by element where the addresses do not allow that) and carries it through the levels of its group.  In mode 2 the group is the whole column: the running ph stays
// in registers and the serial chain costs one subtraction per level, every load and every other operation of a level is
// independent of it.  In mode 1 the column is cut into groups of AMT_P_RHO_GROUP levels, one per blockIdx.y, and ph(k+1)
// becomes the next level's ph(k) in registers: ph is read once per group plus one level.  The level index is uniform in a
// workgroup, so rdnw, znu and dnw come through scalar loads.
#include "amt_internal.h"

// the levels of one group of mode 1 (tests/test_gpu_41_p_rho.py covers kde - 1 = G, G + 1, 2G - 1)
#define AMT_P_RHO_GROUP 8

namespace {
// A call works on a box of nj rows of `ni` contiguous elements and nk = kte - kts cells above one another: the cell (i, k, j) of
// member m is element m * mstride3 + j * jstride3 + k * idim + first3 + i of every 3-D array (they have one layout), its column
// element m * mstride2 + j * idim + first2 + i of mu and muts.  rdnw, znu, dnw point at level kts.
template <typename T>
struct AmtPRhoJob {
    T *al, *p, *ph, *pm1;
    const T *alt, *c2a, *t, *t_old, *mu, *muts, *rdnw, *znu, *dnw;
    int ni, nk, nj;
    long idim, jstride3, mstride3, mstride2, first3, first2;
    T t0, smdiv;
    int step0;                                                     // step == 0: the old pm1 is not read
};

// what a lane moves at once: 16 bytes
template <typename T> struct AmtPRhoVec;
template <> struct AmtPRhoVec<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct AmtPRhoVec<double> { typedef double type __attribute__((ext_vector_type(2))); };

// A wave-uniform pointer, said so to the compiler: the address stays in scalar registers and a lane adds its 32-bit offset in
// the access itself, instead of one 64-bit address per stream and lane in vector registers.  The result points into global
// memory by its type, which the round trip through integers would otherwise hide from the compiler.
#define AMT_GLOBAL __attribute__((address_space(1)))
template <typename P>
__device__ __forceinline__ AMT_GLOBAL P *amt_p_rho_uniform(P *p)
{
    const uintptr_t v = reinterpret_cast<uintptr_t>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return reinterpret_cast<AMT_GLOBAL P *>(((uintptr_t)hi << 32) | lo);
}

// A chunk of `cnt` elements at u + at into the lanes of a 16-byte vector and back: one access where `wide`, element by
// element otherwise (the lanes behind cnt are not read and hold zero; what is computed in them is never stored).
template <typename T>
__device__ __forceinline__ typename AmtPRhoVec<T>::type amt_p_rho_load(const AMT_GLOBAL T *u, unsigned at, bool wide, int cnt)
{
    typedef typename AmtPRhoVec<T>::type V;
    constexpr int kPer = 16 / (int)sizeof(T);
    if (wide) return *reinterpret_cast<const AMT_GLOBAL V *>(u + at);
    V v;
    for (int i = 0; i < kPer; ++i) v[i] = i < cnt ? u[at + i] : T(0);
    return v;
}
template <typename T>
__device__ __forceinline__ void amt_p_rho_store(AMT_GLOBAL T *u, unsigned at, bool wide, int cnt, typename AmtPRhoVec<T>::type v)
{
    typedef typename AmtPRhoVec<T>::type V;
    constexpr int kPer = 16 / (int)sizeof(T);
    if (wide) {
        *reinterpret_cast<AMT_GLOBAL V *>(u + at) = v;
    } else {
        for (int i = 0; i < kPer; ++i)
            if (i < cnt) u[at + i] = v[i];
    }
}

// the term both modes share
template <typename T>
__device__ __forceinline__ T amt_p_rho_q(T alt, T t, T told, T mu, T muts, T t0)
{
    const T a = mu * told;
    const T b = t - a;
    const T num = alt * b;
    const T c = t0 + told;
    const T den = muts * c;
    return num / den;
}

// the divergence damping at step != 0: x is the pressure just diagnosed, the return value what p gets; pm1 always gets x
template <typename T>
__device__ __forceinline__ T amt_p_rho_damp(T x, T pm1, T smdiv)
{
    const T d = x - pm1;
    const T s = smdiv * d;
    return x + s;
}

// The levels k0 .. k0 + nlev - 1 (counted from kts) of one chunk of `cnt` elements (0: a lane behind the row's end, which
// moves nothing): the pointers are the wave's (uniform) at level k0 and come back nlev levels further, `li` is the lane's first
// element behind them.  Both ways of
// moving a chunk feed the same arithmetic, element by element of the vector, so the bits do not depend on the path.
template <typename T, int MODE>
__device__ __forceinline__ void amt_p_rho_walk(const AmtPRhoJob<T> &job, T *&al, T *&p, T *&pm1, T *&ph, const T *&alt, const T *&c2a,
                                               const T *&t, const T *&told, const T *mu2, const T *muts2, int li, bool wide, int cnt,
                                               int k0, int nlev)
{
    typedef typename AmtPRhoVec<T>::type V;
    constexpr int kPer = 16 / (int)sizeof(T);
    const bool step0 = job.step0 != 0;
    const T t0 = job.t0, smdiv = job.smdiv;
    const long idim = job.idim;
    V mu, muts, rmuts;                                             // once per column; a 2-D array's phase is its own
    for (int i = 0; i < kPer; ++i) {
        mu[i] = i < cnt ? mu2[li + i] : T(0);
        muts[i] = i < cnt ? muts2[li + i] : T(0);
    }
    if (MODE == 1)                                                 // T(-1) / muts: the same bits on every level
        for (int i = 0; i < kPer; ++i) rmuts[i] = T(-1) / muts[i];
    const unsigned at = (unsigned)li;                              // the pointers walk k (scalar additions), the lane's offset stays
    V phk = amt_p_rho_load<T>(amt_p_rho_uniform(ph), at, wide, cnt);            // ph(k): read once, then carried in registers
#pragma unroll 1
    for (int kk = 0; kk < nlev; ++kk) {
        const int k = k0 + kk;
        AMT_GLOBAL T *ual = amt_p_rho_uniform(al), *up = amt_p_rho_uniform(p), *upm1 = amt_p_rho_uniform(pm1);
        AMT_GLOBAL T *uph1 = amt_p_rho_uniform(ph + idim);
        const AMT_GLOBAL T *ualt = amt_p_rho_uniform(alt), *uc2a = amt_p_rho_uniform(c2a);
        const AMT_GLOBAL T *ut = amt_p_rho_uniform(t), *uold = amt_p_rho_uniform(told);
        V vpm1, vph1;
        if (!step0) vpm1 = amt_p_rho_load<T>(upm1, at, wide, cnt);
        const V valt = amt_p_rho_load<T>(ualt, at, wide, cnt), vc2a = amt_p_rho_load<T>(uc2a, at, wide, cnt);
        const V vt = amt_p_rho_load<T>(ut, at, wide, cnt), vold = amt_p_rho_load<T>(uold, at, wide, cnt);
        V val, vp, vx;
        if (MODE == 1) {
            vph1 = amt_p_rho_load<T>(uph1, at, wide, cnt);
            const T rdnw = job.rdnw[k];
            for (int i = 0; i < kPer; ++i) {
                const T q = amt_p_rho_q<T>(valt[i], vt[i], vold[i], mu[i], muts[i], t0);
                const T a = valt[i] * mu[i];
                const T d = vph1[i] - phk[i];
                const T b = rdnw * d;
                const T c = a + b;
                val[i] = rmuts[i] * c;
                const T e = q - val[i];
                vx[i] = vc2a[i] * e;
            }
        } else {
            const T znu = job.znu[k], dnw = job.dnw[k];
            for (int i = 0; i < kPer; ++i) {
                const T q = amt_p_rho_q<T>(valt[i], vt[i], vold[i], mu[i], muts[i], t0);
                vx[i] = mu[i] * znu;
                const T r = vx[i] / vc2a[i];
                val[i] = q - r;
                const T a = muts[i] * val[i];
                const T b = mu[i] * valt[i];
                const T c = a + b;
                const T d = dnw * c;
                vph1[i] = phk[i] - d;                              // the chain: one subtraction per level
            }
        }
        for (int i = 0; i < kPer; ++i) vp[i] = step0 ? vx[i] : amt_p_rho_damp<T>(vx[i], vpm1[i], smdiv);
        amt_p_rho_store<T>(ual, at, wide, cnt, val);
        amt_p_rho_store<T>(up, at, wide, cnt, vp);
        amt_p_rho_store<T>(upm1, at, wide, cnt, vx);
        if (MODE == 2) amt_p_rho_store<T>(uph1, at, wide, cnt, vph1);
        phk = vph1;
        al += idim; p += idim; pm1 += idim; ph += idim; alt += idim; c2a += idim; t += idim; told += idim;
    }
}

// Grid (blocks <= 1024, level groups, members), 256 threads, no LDS.  A WAVE owns a segment of 64 consecutive 16-byte chunks of
// one row, counted from the run's first element (a row's last segment and its last chunk may be short), and strides over the
// nj * segments of the box, so that row, level group and segment are wave-uniform: every address is a scalar base plus the
// lane's 32-bit offset, and walking k costs scalar additions.  A lane moves its chunk as 16-byte accesses where ALL the 3-D
// addresses it touches lie on a 16-byte boundary -- the eight arrays have one phase behind the member offset, a row is a
// multiple of 16 bytes long and the chunk starts on a boundary -- and element by element otherwise, and in a run's short last
// chunk.  mu and muts are loaded once per column, element by element.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void amt_p_rho_kernel(AmtPRhoJob<T> job)
{
    constexpr int kPer = 16 / (int)sizeof(T);
    const long moff3 = (long)blockIdx.z * job.mstride3 + job.first3, moff2 = (long)blockIdx.z * job.mstride2 + job.first2;
    const int k0 = MODE == 1 ? (int)blockIdx.y * AMT_P_RHO_GROUP : 0;
    const int left = job.nk - k0;
    const int nlev = MODE == 1 && left > AMT_P_RHO_GROUP ? AMT_P_RHO_GROUP : left;
    const long lev0 = moff3 + (long)k0 * job.idim;
    T *al = job.al + lev0, *p = job.p + lev0, *ph = job.ph + lev0, *pm1 = job.pm1 + lev0;
    const T *alt = job.alt + lev0, *c2a = job.c2a + lev0, *t = job.t + lev0, *told = job.t_old + lev0;
    const T *mu2 = job.mu + moff2, *muts2 = job.muts + moff2;
    const uintptr_t ph0 = reinterpret_cast<uintptr_t>(job.ph + lev0) & 15;
    const auto same = [&](const T *q) { return (reinterpret_cast<uintptr_t>(q + lev0) & 15) == ph0; };
    const bool phase = same(job.al) && same(job.p) && same(job.pm1) && same(job.alt) && same(job.c2a) && same(job.t) &&
                       same(job.t_old) && ((job.idim * (long)sizeof(T)) & 15) == 0;
    constexpr unsigned kSeg = 64 * kPer;                           // the elements of a full segment
    const unsigned ni = (unsigned)job.ni, nj = (unsigned)job.nj;
    const unsigned segs = (ni + kSeg - 1) / kSeg;
    const int li = (int)(threadIdx.x & 63) * kPer;                 // the lane's first element inside its wave's segment
    // wave w takes the units w, w + waves, ... of the nj * segs; unit = j * segs + s, kept as (j, s) without a division per unit
    const unsigned waves = gridDim.x * (blockDim.x >> 6);
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const unsigned dj = waves / segs, ds = waves - dj * segs;
    unsigned j = (unsigned)__builtin_amdgcn_readfirstlane((int)(wave / segs));
    unsigned sg = wave - j * segs;
    // The eight pointers stay where the last unit's walk has left them and move on by the difference to the next unit's
    // first level: the wave holds one set of addresses, not a base and a current one.
    long cur = 0;
    while (j < nj) {
        const unsigned i0 = sg * kSeg;                             // the segment's first element inside its row
        const long at3 = (long)j * job.jstride3 + i0, at2 = (long)j * job.idim + i0;
        const long move = at3 - cur;
        al += move; p += move; pm1 += move; ph += move; alt += move; c2a += move; t += move; told += move;
        cur = at3 + (long)nlev * job.idim;
        const int rest = (int)(ni - i0) - li;
        const int cnt = rest < 0 ? 0 : rest < kPer ? rest : kPer;
        const bool wide = phase && cnt == kPer && (((long)ph0 + at3 * (long)sizeof(T)) & 15) == 0;
        amt_p_rho_walk<T, MODE>(job, al, p, pm1, ph, alt, c2a, t, told, mu2 + at2, muts2 + at2, li, wide, cnt, k0, nlev);
        j += dj;
        sg += ds;
        if (sg >= segs) { sg -= segs; ++j; }
    }
}

struct PRhoArrays {
    void *al, *p, *ph, *pm1;
    const void *alt, *c2a, *t, *t_old, *mu, *muts, *rdnw, *znu, *dnw;
};

// Argument and precondition checks: host arithmetic only.  *empty: the range holds no cell (nothing to do).
int p_rho_check(const char *who, const amt_domain &s, int members, int mode, int step, const PRhoArrays &a, bool *empty)
{
    *empty = false;
    // rank 3, 2 or 1; an output may overlap nothing, inputs may alias one another.  ph is written in mode 2 only.
    const struct { const void *p; int rank; bool output; } arr[13] = {
        {a.al, 3, true}, {a.p, 3, true}, {a.ph, 3, mode == 2}, {a.pm1, 3, true}, {a.alt, 3, false}, {a.c2a, 3, false},
        {a.t, 3, false}, {a.t_old, 3, false}, {a.mu, 2, false}, {a.muts, 2, false}, {a.rdnw, 1, false}, {a.znu, 1, false},
        {a.dnw, 1, false}};
    for (const auto &x : arr)
        if (!x.p) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null array pointer", who);
    if (members < 1) return amt_fail(AMT_ERR_INVALID_ARG, "%s: members = %d: an ensemble has at least one member", who, members);
    if (mode != 1 && mode != 2) return amt_fail(AMT_ERR_INVALID_ARG, "%s: mode = %d: 1 (non-hydrostatic) or 2 (hydrostatic)", who, mode);
    if (step < 0) return amt_fail(AMT_ERR_INVALID_ARG, "%s: step = %d: at least 0", who, step);
    if (s.ime < s.ims || s.jme < s.jms || s.kme < s.kms) return amt_fail(AMT_ERR_PRECONDITION, "%s: empty memory extents", who);
    const size_t idim = s.ime - s.ims + 1, kdim = s.kme - s.kms + 1, jdim = s.jme - s.jms + 1, wb = (size_t)s.dtype_bytes;
    const size_t bytes[4] = {0, kdim * wb, idim * jdim * (size_t)members * wb, idim * kdim * jdim * (size_t)members * wb};
    for (int k = 0; k < 13; ++k) {
        const uintptr_t p0 = reinterpret_cast<uintptr_t>(arr[k].p), pb = bytes[arr[k].rank];
        for (int m = k + 1; m < 13; ++m) {
            if (!(arr[k].output || arr[m].output)) continue;
            const uintptr_t r0 = reinterpret_cast<uintptr_t>(arr[m].p), rb = bytes[arr[m].rank];
            if (p0 < r0 + rb && r0 < p0 + pb) return amt_fail(AMT_ERR_INVALID_ARG, "%s: an output array overlaps another array of the call", who);
        }
    }
    if (s.kts != 1) return amt_fail(AMT_ERR_PRECONDITION, "%s: kts = %d, the library needs kts == 1", who, s.kts);
    if (s.kte != s.kde) return amt_fail(AMT_ERR_PRECONDITION, "%s: kte = %d is not kde = %d", who, s.kte, s.kde);
    if (s.kme < s.kte || s.kms > s.kts) return amt_fail(AMT_ERR_PRECONDITION, "%s: levels kts:kte = %d:%d are not inside memory kms:kme = %d:%d", who, s.kts, s.kte, s.kms, s.kme);
    if (s.ite < s.its || s.jte < s.jts || s.kte <= s.kts) { *empty = true; return AMT_OK; }
    if (s.its < s.ims || s.ite > s.ime || s.jts < s.jms || s.jte > s.jme)
        return amt_fail(AMT_ERR_PRECONDITION, "%s: the tile %d:%d, %d:%d is not inside memory %d:%d, %d:%d", who,
                        s.its, s.ite, s.jts, s.jte, s.ims, s.ime, s.jms, s.jme);
    if (members > 65535) return amt_fail(AMT_ERR_PRECONDITION, "%s: %d members: one launch covers at most 65535", who, members);
    const int ihi = s.ite < s.ide - 1 ? s.ite : s.ide - 1, jhi = s.jte < s.jde - 1 ? s.jte : s.jde - 1;
    if (ihi < s.its || jhi < s.jts) *empty = true;
    return AMT_OK;
}

template <typename T>
int p_rho_launch(const amt_domain &d, int members, int mode, int step, const PRhoArrays &a, double t0, double smdiv)
{
    const long idim = d.ime - d.ims + 1, kdim = d.kme - d.kms + 1, jdim = d.jme - d.jms + 1;
    AmtPRhoJob<T> job{};
    job.al = static_cast<T *>(a.al); job.p = static_cast<T *>(a.p); job.ph = static_cast<T *>(a.ph); job.pm1 = static_cast<T *>(a.pm1);
    job.alt = static_cast<const T *>(a.alt); job.c2a = static_cast<const T *>(a.c2a);
    job.t = static_cast<const T *>(a.t); job.t_old = static_cast<const T *>(a.t_old);
    job.mu = static_cast<const T *>(a.mu); job.muts = static_cast<const T *>(a.muts);
    job.rdnw = static_cast<const T *>(a.rdnw) + (d.kts - d.kms);
    job.znu = static_cast<const T *>(a.znu) + (d.kts - d.kms);
    job.dnw = static_cast<const T *>(a.dnw) + (d.kts - d.kms);
    job.ni = (d.ite < d.ide - 1 ? d.ite : d.ide - 1) - d.its + 1;
    job.nk = d.kte - d.kts;
    job.nj = (d.jte < d.jde - 1 ? d.jte : d.jde - 1) - d.jts + 1;
    job.idim = idim; job.jstride3 = kdim * idim; job.mstride3 = idim * kdim * jdim; job.mstride2 = idim * jdim;
    job.first3 = ((long)(d.jts - d.jms) * kdim + (d.kts - d.kms)) * idim + (d.its - d.ims);
    job.first2 = (long)(d.jts - d.jms) * idim + (d.its - d.ims);
    job.t0 = (T)t0; job.smdiv = (T)smdiv;
    job.step0 = step == 0;
    constexpr long seg = 64 * 16 / (long)sizeof(T);                 // the elements of a wave's segment
    const long units = (long)job.nj * ((job.ni + seg - 1) / seg);
    long blocks = (units + 3) / 4;                                 // four waves to a block
    if (blocks > 1024) blocks = 1024;
    if (mode == 1) {
        const unsigned groups = (unsigned)((job.nk + AMT_P_RHO_GROUP - 1) / AMT_P_RHO_GROUP);
        hipLaunchKernelGGL((amt_p_rho_kernel<T, 1>), dim3((unsigned)blocks, groups, (unsigned)members), dim3(256), 0, d.stream, job);
    } else {
        hipLaunchKernelGGL((amt_p_rho_kernel<T, 2>), dim3((unsigned)blocks, 1, (unsigned)members), dim3(256), 0, d.stream, job);
    }
    AMT_HIP(hipGetLastError());
    return AMT_OK;
}

// with_device_check: the pointer-level calls, which may be the first HIP call of a process, report a missing device
// themselves -- behind the argument errors, which need none -- and run on the caller's current device
int p_rho_run(const char *who, const amt_domain &d, int members, int mode, int step, const PRhoArrays &a, double t0, double smdiv,
              bool with_device_check)
{
    bool empty = false;
    const int rc = p_rho_check(who, d, members, mode, step, a, &empty);
    if (rc != AMT_OK || empty) return rc;
    int dev = d.device;
    if (with_device_check) {
        int ndev = 0;
        AMT_HIP(hipGetDeviceCount(&ndev));
        if (ndev < 1) return amt_fail(AMT_ERR_NO_DEVICE, "no HIP device visible");
        (void)hipGetDevice(&dev);
    }
    DeviceScope scope(dev);
    return d.dtype_bytes == 8 ? p_rho_launch<double>(d, members, mode, step, a, t0, smdiv)
                              : p_rho_launch<float>(d, members, mode, step, a, t0, smdiv);
}

// what a handle's call works on: al, p, ph, pm1, alt, c2a, znu, dnw are the setting's, t_old the stage bracket's
PRhoArrays p_rho_of_domain(const amt_domain *d)
{
    void *const *x = d->p_rho_arr;
    return PRhoArrays{x[0], x[1], x[2], x[3], x[4], x[5], d->field[AMT_F_T], d->stage_arr[0], d->field[AMT_F_MU], d->field[AMT_F_MUTS],
                      d->field[AMT_F_RDNW], x[6], x[7]};
}
}  // namespace

// ---- what the handles call (amt_handle_*p_rho of amt_domain.hip) ----------------------------------------------------------
int amt_p_rho_domain(const char *who, amt_domain *d, int members, int step)
{
    if (!d->p_rho_mode) return amt_fail(AMT_ERR_PRECONDITION, "%s: the pressure diagnosis is off (amt_*_set_p_rho)", who);
    if (!d->stage_on) return amt_fail(AMT_ERR_PRECONDITION, "%s: the stage bracket, whose t_old the diagnosis reads, is off (amt_*_set_stage)", who);
    return p_rho_run(who, *d, members, d->p_rho_mode, step, p_rho_of_domain(d), d->p_rho_t0, d->p_rho_smdiv, false);
}

void amt_p_rho_release(amt_domain *d)
{
    for (void *&q : d->p_rho_arr) {
        if (q && d->p_rho_owned) (void)hipFree(q);
        q = nullptr;
    }
    d->p_rho_mode = 0;
    d->p_rho_per_sweep = 0;
    d->p_rho_owned = false;
}

// amt_*_set_p_rho.  A refusal changes nothing.
int amt_p_rho_set_domain(const char *who, amt_domain *d, int members, int mode, int per_sweep, double t0, double smdiv, void *const given_arr[8])
{
    if (mode == 0) {
        DeviceScope scope(d->device);
        amt_p_rho_release(d);
        return AMT_OK;
    }
    if (mode != 1 && mode != 2) return amt_fail(AMT_ERR_INVALID_ARG, "%s: mode = %d: 0 (off), 1 (non-hydrostatic) or 2 (hydrostatic)", who, mode);
    void *arr[8];
    int given = 0;
    for (int k = 0; k < 8; ++k) given += (arr[k] = given_arr[k]) != nullptr;
    if (given != 0 && given != 8)
        return amt_fail(AMT_ERR_INVALID_ARG, "%s: give all eight arrays or none (the library then allocates them)", who);
    if (!d->stage_on) return amt_fail(AMT_ERR_PRECONDITION, "%s: the stage bracket, whose t_old the diagnosis reads, is off (amt_*_set_stage)", who);
    // the library's own arrays handed back (amt_*_p_rho_ptr): they stay the library's, the mode and the scalars are set anew;
    // some of them among the caller's would be freed under the caller
    const bool same = given == 8 && d->p_rho_owned && memcmp(arr, d->p_rho_arr, sizeof arr) == 0;
    if (given == 8 && d->p_rho_owned && !same)
        for (void *mine : d->p_rho_arr)
            for (void *theirs : arr)
                if (mine == theirs) return amt_fail(AMT_ERR_INVALID_ARG, "%s: an array the library allocated, mixed with others", who);
    if (given == 8) {
        amt_domain probe = *d;                                     // the checks against the caller's arrays, nothing enqueued
        memcpy(probe.p_rho_arr, arr, sizeof arr);
        bool empty = false;
        const int rc = p_rho_check(who, probe, members, mode, 0, p_rho_of_domain(&probe), &empty);
        if (rc) return rc;
    } else {
        if (members > 65535) return amt_fail(AMT_ERR_PRECONDITION, "%s: %d members: one launch covers at most 65535", who, members);
        if (d->kts != 1 || d->kte != d->kde || d->kme < d->kte || d->kms > d->kts || d->its < d->ims || d->ite > d->ime || d->jts < d->jms || d->jte > d->jme)
            return amt_fail(AMT_ERR_PRECONDITION, "%s: the handle's tile does not admit the pressure diagnosis (kts == 1, kte == kde, tile inside memory)", who);
    }
    DeviceScope scope(d->device);                                  // behind every refusal but a failed allocation
    if (given == 0) {
        for (int k = 0; k < 8; ++k) {
            const size_t bytes = (k < 6 ? d->count(AMT_F_T) * (size_t)members : d->count(AMT_F_DNW)) * (size_t)d->dtype_bytes;
            arr[k] = nullptr;
            if (hipMalloc(&arr[k], bytes) != hipSuccess) {
                (void)hipGetLastError();
                for (int m = 0; m < k; ++m) (void)hipFree(arr[m]);
                return amt_fail(AMT_ERR_ALLOC, "%s: no room for an array of %zu bytes", who, bytes);
            }
        }
    }
    if (!same) {
        amt_p_rho_release(d);
        memcpy(d->p_rho_arr, arr, sizeof arr);
        d->p_rho_owned = given == 0;
    }
    d->p_rho_mode = mode;
    d->p_rho_per_sweep = per_sweep != 0;
    d->p_rho_t0 = t0;
    d->p_rho_smdiv = smdiv;
    return AMT_OK;
}

// ---- pointer level -------------------------------------------------------------------------------------------------------
#define AMT_P_RHO_SIG(T)                                                                                        \
    void *hip_stream, int members, int mode, int step, T *al, T *p, T *ph, T *pm1, const T *alt, const T *c2a,  \
    const T *t, const T *t_old, const T *mu, const T *muts, const T *rdnw, const T *znu, const T *dnw,          \
    T t0, T smdiv,                                                                                              \
    int ids, int ide, int jds, int jde, int kde, int ims, int ime, int jms, int jme, int kms, int kme,          \
    int its, int ite, int jts, int jte, int kts, int kte
#define AMT_P_RHO_BODY(T, name)                                                                                 \
    amt_domain d{(int)sizeof(T), 0, 0, 0, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte}; \
    d.stream = static_cast<hipStream_t>(hip_stream);                                                            \
    return p_rho_run(name, d, members, mode, step, PRhoArrays{al, p, ph, pm1, alt, c2a, t, t_old, mu, muts, rdnw, znu, dnw}, \
                     (double)t0, (double)smdiv, true);

extern "C" int amt_p_rho_device_f32(AMT_P_RHO_SIG(float)) { AMT_P_RHO_BODY(float, "amt_p_rho_device_f32") }
extern "C" int amt_p_rho_device_f64(AMT_P_RHO_SIG(double)) { AMT_P_RHO_BODY(double, "amt_p_rho_device_f64") }
