// amt_p_rho_kernel.h -- the device text of the pressure diagnosis (amt_p_rho.hip, which states the arithmetic and launches
// it): the job, the 16-byte accesses, the walk over k and the kernel.  Included by amt_p_rho.hip behind amt_internal.h, and by
// tests/p_rho_host_check.cpp behind stand-ins for the thread indices, readfirstlane and AMT_GLOBAL, which runs this text on
// the host under the address and undefined-behaviour sanitizers (tests/test_prho_host.py; the precedent is
// amt_chunk_index.h).  The text is in an unnamed namespace, as it was inside amt_p_rho.hip.
#ifndef AMT_P_RHO_KERNEL_H
#define AMT_P_RHO_KERNEL_H

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
#ifndef AMT_GLOBAL
#define AMT_GLOBAL __attribute__((address_space(1)))
#endif
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
}  // namespace

#endif  // AMT_P_RHO_KERNEL_H
