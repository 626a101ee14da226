// amt_uv_kernel.h -- the device text of the acoustic loop's momentum update (amt_uv.hip, which states the contract and launches
// it): the job, the access to a chunk and its neighbour, the walk over k and the kernel.  Included by amt_uv.hip behind
// amt_internal.h, and by tests/uv_host_check.cpp behind stand-ins for the thread indices, readfirstlane and AMT_GLOBAL, which
// runs this text on the host under the address and undefined-behaviour sanitizers (tests/test_uv_host.py).  The 16-byte vector,
// the wave-uniform pointer and the chunk accesses over a uniform base with a 32-bit lane offset are amt_p_rho_kernel.h's.
#ifndef AMT_UV_KERNEL_H
#define AMT_UV_KERNEL_H

#include <cstddef>
#include <type_traits>

#include "amt_p_rho_kernel.h"

// the levels of one group (tests/test_gpu_43_advance_uv.py covers kde - 1 = G, G + 1, 2G - 1)
#define AMT_UV_GROUP 8

namespace {
// The u part and the v part are one text: a cell and its NEIGHBOUR, which lies nb3 elements in front of it in a 3-D array and
// nb2 in a 2-D one (u: 1 and 1, the cell at i-1; v: a memory row of k levels and a memory row, the cell at j-1).  A part works
// on nj rows of ni contiguous cells that start i0 columns and j0 rows behind the tile's first cell.  The distances follow
// from the part and are not kept in the job.
template <typename T>
struct AmtUvPart {
    T *out;                                                        // u | v
    const T *tend, *cq, *mass, *msf_num, *msf_den, *msf_md;        // ru_tend cqu muu msfux msfuy msfuy | rv_tend cqv muv msfvy msfvx msfvx_inv
    T rd, md_scale;                                                // rdx | rdy;  (-emdiv) * dx | (-emdiv) * dy
    int i0, j0, ni, nj;
};

// The cell (i, k, j) of member m is element m * mstride3 + j * jstride3 + k * idim + first3 + i of every 3-D array, counted
// from the tile's first cell (they have one layout), its column element m * mstride2 + j * idim + first2 + i of the 2-D
// arrays.  fnm, fnp, rdnw point at level kts.  nk = kte - kts cells above one another.
template <typename T>
struct AmtUvJob {
    AmtUvPart<T> part[2];
    const T *p, *pb, *ph, *php, *alt, *al, *mu, *mudf, *fnm, *fnp, *rdnw;
    int nk;
    long idim, jstride3, mstride3, mstride2, first3, first2;
    T dts, cf1, cf2, cf3;
};

// A chunk of `cnt` elements at base + at and the chunk of its neighbours.  PART 0: the neighbour of element i is element i - 1
// of the same row -- the chunk shifted by one lane of the vector, and ONE more element in front of it.  PART 1: the same chunk
// one row below, which moves as the chunk itself does (a memory row of a `wide` call is a multiple of 16 bytes long).
template <typename T, int PART>
__device__ __forceinline__ void amt_uv_load2(const T *base, unsigned at, long nb, bool wide, int cnt, typename AmtPRhoVec<T>::type &own,
                                             typename AmtPRhoVec<T>::type &nbr)
{
    constexpr int kPer = 16 / (int)sizeof(T);
    own = amt_p_rho_load<T>(amt_p_rho_uniform(base), at, wide, cnt);
    if (PART == 0) {
        const AMT_GLOBAL T *before = amt_p_rho_uniform(base - 1);
        nbr[0] = cnt > 0 ? before[at] : T(0);
        for (int i = 1; i < kPer; ++i) nbr[i] = own[i - 1];
    } else {
        nbr = amt_p_rho_load<T>(amt_p_rho_uniform(base - nb), at, wide, cnt);
    }
}

// own + nbr and own - nbr of p at one level: all the walk keeps of it
template <typename T, int PART>
__device__ __forceinline__ void amt_uv_p(const T *p, unsigned at, long nb, bool wide, int cnt, typename AmtPRhoVec<T>::type &sum,
                                         typename AmtPRhoVec<T>::type &diff)
{
    constexpr int kPer = 16 / (int)sizeof(T);
    typename AmtPRhoVec<T>::type own, nbr;
    amt_uv_load2<T, PART>(p, at, nb, wide, cnt, own, nbr);
    for (int i = 0; i < kPer; ++i) {
        sum[i] = own[i] + nbr[i];
        diff[i] = own[i] - nbr[i];
    }
}

// The job's words as the kernel argument holds them, read ANEW behind this point: what a unit needs of the job -- fifteen base
// pointers, the strides -- is then loaded from the kernel argument segment (scalar loads that hit the scalar cache) when the
// unit starts, instead of staying in scalar registers across the units, where it does not fit beside the walk's own.  The
// host stand-in is the identity.
#ifndef AMT_UV_CONST
#define AMT_UV_CONST __attribute__((address_space(4)))
#endif
#ifndef AMT_UV_FRESH
#define AMT_UV_FRESH(q) asm volatile("" : "+s"(q))
#endif

// The levels k0 .. k0 + nlev - 1 (counted from kts) of one chunk of `cnt` elements (0: a lane behind the row's end, which
// moves nothing): the 3-D pointers are the wave's at level k0 and come back nlev levels further, the 2-D ones the wave's at
// the unit's first column; `li` is the lane's first element behind them.  Both ways of moving a chunk feed the same
// arithmetic, element by element of the vector.  What k shares stays in registers: ph(k+1) - ph'(k+1) is the next level's
// ph(k) - ph'(k); of p the walk holds the sum s and the difference of the levels k and k+1 and reads level k+2 while it works
// on k, so that dpn(k+1) comes from registers, dpn(kts) finds s(1..3) and no level is read twice.
template <typename T, int PART, bool NH>
__device__ __forceinline__ void amt_uv_walk(const AMT_UV_CONST AmtUvJob<T> *job, T *&out, const T *&tend, const T *&cq,
                                            const T *&p, const T *&pb, const T *&ph, const T *&php, const T *&alt, const T *&al,
                                            const T *mu2, const T *mudf2, const T *mass2, const T *num2, const T *den2, const T *md2,
                                            int li, bool wide, int cnt, int k0, int nlev)
{
    typedef typename AmtPRhoVec<T>::type V;
    constexpr int kPer = 16 / (int)sizeof(T);
    const long idim = job->idim, nb3 = PART == 0 ? 1 : job->jstride3, nb2 = PART == 0 ? 1 : idim;
    const T dts = job->dts, rd = job->part[PART].rd, half = T(0.5);
    const int nk = job->nk;
    V c, md, mrd, hm;                                              // once per column; a 2-D array's phase is its own
    for (int i = 0; i < kPer; ++i) {
        const bool on = i < cnt;
        const T num = on ? num2[li + i] : T(0), den = on ? den2[li + i] : T(0), mass = on ? mass2[li + i] : T(0);
        const T dfo = on ? mudf2[li + i] : T(0), dfn = on ? mudf2[li + i - nb2] : T(0), msf = on ? md2[li + i] : T(0);
        const T mr = num / den;
        const T c1 = mr * half;
        const T c2 = c1 * rd;
        c[i] = c2 * mass;
        const T dd = dfo - dfn;
        const T m1 = job->part[PART].md_scale * dd;
        md[i] = PART == 0 ? m1 / msf : m1 * msf;
        if (NH) {
            const T muo = on ? mu2[li + i] : T(0), mun = on ? mu2[li + i - nb2] : T(0);
            mrd[i] = mr * rd;
            const T ms = mun + muo;
            hm[i] = half * ms;
        }
    }
    const unsigned at = (unsigned)li;                              // the pointers walk k (scalar additions), the lane's offset stays
    V dphk;                                                        // ph(k) - ph'(k)
    {
        V o, n;
        amt_uv_load2<T, PART>(ph, at, nb3, wide, cnt, o, n);
        for (int i = 0; i < kPer; ++i) dphk[i] = o[i] - n[i];
    }
    V sa = {}, da = {}, sb = {}, db = {}, sc = {}, dc = {}, dpnk = {};   // NH: s and p - p' of the levels k, k+1, k+2; dpn(k)
    if (NH) {
        amt_uv_p<T, PART>(p, at, nb3, wide, cnt, sa, da);
        if (k0 + 1 < nk) amt_uv_p<T, PART>(p + idim, at, nb3, wide, cnt, sb, db);
        if (k0 == 0) {                                             // dpn(kts) from s(1..3): nk >= 3, the first group holds three levels
            amt_uv_p<T, PART>(p + 2 * idim, at, nb3, wide, cnt, sc, dc);
            const T cf1 = job->cf1, cf2 = job->cf2, cf3 = job->cf3;
            for (int i = 0; i < kPer; ++i) {
                const T a = cf1 * sa[i];
                const T b = cf2 * sb[i];
                const T e = cf3 * sc[i];
                const T f = a + b;
                const T g = f + e;
                dpnk[i] = half * g;
            }
        } else {                                                   // dpn(k0) from s(k0) and s(k0 - 1)
            V sp, dp;
            amt_uv_p<T, PART>(p - idim, at, nb3, wide, cnt, sp, dp);
            const T fnm = job->fnm[k0], fnp = job->fnp[k0];
            for (int i = 0; i < kPer; ++i) {
                const T a = fnm * sa[i];
                const T b = fnp * sp[i];
                const T e = a + b;
                dpnk[i] = half * e;
            }
        }
    }
#pragma unroll 1
    for (int kk = 0; kk < nlev; ++kk) {
        const int k = k0 + kk;
        V dpn1;
        if (NH) {
            if (k > 0 && k + 2 < nk && kk + 1 < nlev) amt_uv_p<T, PART>(p + 2 * idim, at, nb3, wide, cnt, sc, dc);   // kts: read above
            if (k + 1 < nk) {
                const T fnm = job->fnm[k + 1], fnp = job->fnp[k + 1];
                for (int i = 0; i < kPer; ++i) {
                    const T a = fnm * sb[i];
                    const T b = fnp * sa[i];
                    const T e = a + b;
                    dpn1[i] = half * e;
                }
            } else {
                for (int i = 0; i < kPer; ++i) dpn1[i] = T(0);     // dpn(kte)
            }
        } else {
            amt_uv_p<T, PART>(p, at, nb3, wide, cnt, sa, da);
        }
        V ph1o, ph1n, alto, altn, alo, aln, pbo, pbn, phpo, phpn;
        amt_uv_load2<T, PART>(ph + idim, at, nb3, wide, cnt, ph1o, ph1n);
        amt_uv_load2<T, PART>(alt, at, nb3, wide, cnt, alto, altn);
        amt_uv_load2<T, PART>(al, at, nb3, wide, cnt, alo, aln);
        amt_uv_load2<T, PART>(pb, at, nb3, wide, cnt, pbo, pbn);
        if (NH) amt_uv_load2<T, PART>(php, at, nb3, wide, cnt, phpo, phpn);
        AMT_GLOBAL T *uout = amt_p_rho_uniform(out);
        const V vout = amt_p_rho_load<T>(uout, at, wide, cnt);
        const V vtend = amt_p_rho_load<T>(amt_p_rho_uniform(tend), at, wide, cnt), vcq = amt_p_rho_load<T>(amt_p_rho_uniform(cq), at, wide, cnt);
        const T rdnw = NH ? job->rdnw[k] : T(0);
        V res;
        for (int i = 0; i < kPer; ++i) {
            const T dph1 = ph1o[i] - ph1n[i];
            const T g1 = dph1 + dphk[i];
            const T a1 = alto[i] + altn[i];
            const T a2 = a1 * da[i];
            const T g2 = g1 + a2;
            const T b1 = alo[i] + aln[i];
            const T b2 = pbo[i] - pbn[i];
            const T b3 = b1 * b2;
            const T g = g2 + b3;
            T dpxy = c[i] * g;
            if (NH) {
                const T w1 = phpo[i] - phpn[i];
                const T w = mrd[i] * w1;
                const T e1 = dpn1[i] - dpnk[i];
                const T e2 = rdnw * e1;
                const T e = e2 - hm[i];
                const T we = w * e;
                dpxy = dpxy + we;
            }
            const T x1 = dts * vtend[i];
            const T x2 = vout[i] + x1;
            const T y1 = dts * vcq[i];
            const T y2 = y1 * dpxy;
            const T x3 = x2 - y2;
            res[i] = x3 + md[i];
            dphk[i] = dph1;
        }
        amt_p_rho_store<T>(uout, at, wide, cnt, res);
        if (NH) { dpnk = dpn1; sa = sb; da = db; sb = sc; db = dc; }
        out += idim; tend += idim; cq += idim; p += idim; pb += idim; ph += idim; php += idim; alt += idim; al += idim;
    }
}

// One part of the launch: the level group `group` of member blockIdx.z.  A WAVE owns a segment of 64 consecutive 16-byte
// chunks of one row of the part, counted from the row's first cell, and strides over the nj * segments of the part, as in
// amt_p_rho_kernel: row, level group and segment are wave-uniform.  A lane moves its chunk as 16-byte accesses where ALL the
// 3-D addresses it touches lie on a 16-byte boundary -- the arrays the part reads have one phase behind the member offset, a
// memory row is a multiple of 16 bytes long and the chunk starts on a boundary -- and element by element otherwise, and in a
// row's short last chunk.  The 2-D arrays are loaded once per column and group, element by element.
template <typename T, int PART, bool NH>
__device__ __forceinline__ void amt_uv_part(const AMT_UV_CONST AmtUvJob<T> *jp, int group)
{
    constexpr int kPer = 16 / (int)sizeof(T);
    constexpr unsigned kSeg = 64 * kPer;                           // the elements of a full segment
    const unsigned ni = (unsigned)jp->part[PART].ni, nj = (unsigned)jp->part[PART].nj;
    if (ni < 1 || nj < 1) return;
    const int k0 = group * AMT_UV_GROUP;
    const int left = jp->nk - k0;
    const int nlev = left > AMT_UV_GROUP ? AMT_UV_GROUP : left;
    const unsigned segs = (ni + kSeg - 1) / kSeg;
    const int li = (int)(threadIdx.x & 63) * kPer;                 // the lane's first element inside its wave's segment
    // wave w takes the units w, w + waves, ... of the nj * segs; unit = j * segs + s, kept as (j, s) without a division per unit
    const unsigned waves = gridDim.x * (blockDim.x >> 6);
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const unsigned dj = waves / segs, ds = waves - dj * segs;
    unsigned j = (unsigned)__builtin_amdgcn_readfirstlane((int)(wave / segs));
    unsigned sg = wave - j * segs;
    while (j < nj) {
        AMT_UV_FRESH(jp);
        const AMT_UV_CONST AmtUvJob<T> *job = jp;
        const AMT_UV_CONST AmtUvPart<T> *pt = &jp->part[PART];
        const unsigned i0 = sg * kSeg;                             // the segment's first element inside its row
        const long row = (long)pt->j0 + j;
        const long at2 = (long)blockIdx.z * job->mstride2 + job->first2 + row * job->idim + pt->i0 + i0;
        const long at3 = (long)blockIdx.z * job->mstride3 + job->first3 + row * job->jstride3 + (long)k0 * job->idim + pt->i0 + i0;
        T *out = pt->out + at3;
        const T *tend = pt->tend + at3, *cq = pt->cq + at3, *p = job->p + at3, *pb = job->pb + at3, *ph = job->ph + at3;
        const T *php = job->php + at3, *alt = job->alt + at3, *al = job->al + at3;
        const uintptr_t ph0 = reinterpret_cast<uintptr_t>(out) & 15;
        const auto same = [&](const T *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == ph0; };
        const bool phase = ph0 == 0 && same(tend) && same(cq) && same(p) && same(pb) && same(ph) && (!NH || same(php)) && same(alt) &&
                           same(al) && ((job->idim * (long)sizeof(T)) & 15) == 0;
        const int rest = (int)(ni - i0) - li;
        const int cnt = rest < 0 ? 0 : rest < kPer ? rest : kPer;
        const bool wide = phase && cnt == kPer;
        amt_uv_walk<T, PART, NH>(job, out, tend, cq, p, pb, ph, php, alt, al, job->mu + at2, job->mudf + at2, pt->mass + at2,
                                 pt->msf_num + at2, pt->msf_den + at2, pt->msf_md + at2, li, wide, cnt, k0, nlev);
        j += dj;
        sg += ds;
        if (sg >= segs) { sg -= segs; ++j; }
    }
}

// Grid (blocks <= 1024, 2 * level groups, members), 256 threads, no LDS: blockIdx.y counts the level groups of the u part,
// then those of the v part.  AMT_UV_JOB: where the job lies -- on the device the kernel argument segment, which it opens.
#ifndef AMT_UV_JOB
#define AMT_UV_JOB(T, job) ((const AMT_UV_CONST AmtUvJob<T> *)__builtin_amdgcn_kernarg_segment_ptr())
#endif
// `job` is the kernel's ONLY argument and no argument may be placed in front of it: AMT_UV_JOB reads it at offset 0 of the
// kernel-argument segment, in the layout the host passed -- a trivially copyable struct of pointers, longs, ints and T.
static_assert(std::is_trivially_copyable<AmtUvJob<float>>::value && std::is_trivially_copyable<AmtUvJob<double>>::value &&
              std::is_standard_layout<AmtUvJob<double>>::value && alignof(AmtUvJob<double>) == 8 && offsetof(AmtUvJob<double>, part) == 0,
              "the job is read from the kernel-argument segment as the host laid it out");
template <typename T, bool NH>
__global__ __launch_bounds__(256) void amt_uv_kernel(AmtUvJob<T> job)
{
    const AMT_UV_CONST AmtUvJob<T> *jp = AMT_UV_JOB(T, job);
    const int groups = (jp->nk + AMT_UV_GROUP - 1) / AMT_UV_GROUP;
    if ((int)blockIdx.y < groups) amt_uv_part<T, 0, NH>(jp, (int)blockIdx.y);
    else amt_uv_part<T, 1, NH>(jp, (int)blockIdx.y - groups);
}
}  // namespace

#endif  // AMT_UV_KERNEL_H
