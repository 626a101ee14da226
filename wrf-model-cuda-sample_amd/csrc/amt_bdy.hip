// amt_bdy.hip -- specified / nested lateral boundaries: the boundary-zone update on the device (include/amt_advance_mu_t.h
// section 12).  With `specified` or `nested` advance_mu_t clips its compute window by one cell at every
// domain edge (module_small_step_em.f90:97-106) and leaves the outer ring to the caller; in WRF's acoustic loop three
// spec_bdyupdate calls of zone width 1 advance it after every call:
//   t += dts * ft (levels kts..kte-1),  mu += dts * mu_tend,  muts += dts * mu_tend
// over the BOUNDARY ZONE of the tile: every cell of its..min(ite, ide-1), jts..min(jte, jde-1) that is not in the compute
// window.  The zone is cut into at most four strips that share no cell -- rows below and above the window over the tile's whole
// width (they own the corners), columns left and right of it over the window's rows; the whole tile where the window is empty --
// and ONE launch does the three fields of every strip, times the members of an ensemble.  Product, then sum: two roundings
// (the library is built with -ffp-contract=off).
#include "amt_internal.h"
#include "amt_chunk_io.h"

namespace {
enum { AMT_BDY_MAX_JOBS = 12 };             // 4 strips x 3 fields

// Job q updates `runs` runs of `len` contiguous elements: run r of member m starts at element
//   m * member_stride + (r / levels) * row_stride + (r % levels) * stride
// of dst and of tend alike (a field and its tendency have one layout).  With idim = elements of a memory row of i:
//   a strip of a 3-D field: levels = kte - kts, stride = idim, row_stride = kdim * idim  (level kte is never touched)
//   a strip of a 2-D field: levels = 1, row_stride = idim
//   rows: len = the tile's width;  columns: len = 1 (one element per run, at stride idim)
template <typename T>
struct AmtBdyJobs {
    T *dst[AMT_BDY_MAX_JOBS];
    const T *tend[AMT_BDY_MAX_JOBS];
    long runs[AMT_BDY_MAX_JOBS], levels[AMT_BDY_MAX_JOBS];
    long stride[AMT_BDY_MAX_JOBS], row_stride[AMT_BDY_MAX_JOBS], member_stride[AMT_BDY_MAX_JOBS];
    int len[AMT_BDY_MAX_JOBS];
    T dts;
};

// Grid (blocks, jobs, members).  A work item is one 16-byte chunk of a run (its last chunk may be short), lanes run along
// (chunk, level, row): along i for a row strip -- all three streams coalesced --, along (level, row) for a column, which touches
// one line per element.  A whole chunk is ONE 16-byte load of each operand and one 16-byte store where dst AND tend lie on a
// 16-byte boundary (decided per chunk from its two addresses, behind the member offset); a run's short last chunk and every
// other chunk go element by element, into and out of the same vector (amt_chunk_io.h).
// Nothing outside a run is read or written.  Offsets are 64-bit.  256 threads, no LDS.
template <typename T>
__global__ __launch_bounds__(256) void amt_bdy_kernel(AmtBdyJobs<T> jobs)
{
    typedef typename AmtVec16<T>::type V;
    constexpr int kPer = 16 / (int)sizeof(T);
    const int q = blockIdx.y;
    const long moff = (long)blockIdx.z * jobs.member_stride[q];
    T *dst = jobs.dst[q] + moff;
    const T *tend = jobs.tend[q] + moff;
    const T dts = jobs.dts;
    const long len = jobs.len[q], levels = jobs.levels[q];
    const long chunks = (len + kPer - 1) / kPer;
    const long total = jobs.runs[q] * chunks;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long r = chunks == 1 ? e : e / chunks;
        const long first = (e - r * chunks) * kPer;                // first element of this chunk inside its run
        const long row = levels == 1 ? r : r / levels;
        const long at = row * jobs.row_stride[q] + (r - row * levels) * jobs.stride[q] + first;
        T *d = dst + at;
        const T *s = tend + at;
        const long left = len - first;
        const int cnt = left < kPer ? (int)left : kPer;
        const bool wide = cnt == kPer && ((reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(s)) & 15) == 0;
        const V old = amt_chunk_load<T>(d, wide, cnt), tn = amt_chunk_load<T>(s, wide, cnt);
        V out;
        for (int i = 0; i < kPer; ++i) {
            const T step = dts * tn[i];
            out[i] = old[i] + step;
        }
        amt_chunk_store<T>(d, wide, cnt, out);
    }
}

struct BdyArrays {
    void *t;
    const void *ft;
    void *mu, *muts;
    const void *mu_tend;
};

// The strips of the zone, Fortran indices: rows j0..j1 x columns i0..i1 each, no cell twice.  Host arithmetic.
struct BdyStrip { int i0, i1, j0, j1; };
int bdy_strips(const amt_domain &s, BdyStrip out[4])
{
    const AmtWindow w = amt_window(s.periodic_x, s.specified, s.nested, s.ids, s.ide, s.jds, s.jde, s.its, s.ite, s.jts, s.jte, s.kts, s.kte);
    const int ihi = s.ite < s.ide - 1 ? s.ite : s.ide - 1, jhi = s.jte < s.jde - 1 ? s.jte : s.jde - 1;
    if (ihi < s.its || jhi < s.jts) return 0;                                          // the tile holds no mass point
    if (w.i_end < w.i_start || w.j_end < w.j_start) {                                  // no window: every cell is zone
        out[0] = BdyStrip{s.its, ihi, s.jts, jhi};
        return 1;
    }
    int n = 0;
    if (w.j_start > s.jts) out[n++] = BdyStrip{s.its, ihi, s.jts, w.j_start - 1};      // below: the tile's whole width
    if (w.j_end < jhi) out[n++] = BdyStrip{s.its, ihi, w.j_end + 1, jhi};              // above
    if (w.i_start > s.its) out[n++] = BdyStrip{s.its, w.i_start - 1, w.j_start, w.j_end};   // left: the window's rows
    if (w.i_end < ihi) out[n++] = BdyStrip{w.i_end + 1, ihi, w.j_start, w.j_end};      // right
    return n;
}

// Argument and precondition checks: host arithmetic only.  *n: the number of strips (0: empty zone, nothing to do).
int bdy_check(const char *who, int members, const amt_domain &s, BdyStrip strips[4], int *n)
{
    *n = 0;
    if (members < 1) return amt_fail(AMT_ERR_INVALID_ARG, "%s: members = %d: an ensemble has at least one member", who, members);
    if (!s.specified && !s.nested)
        return amt_fail(AMT_ERR_PRECONDITION, "%s: neither specified nor nested: the compute window is not clipped, there is no boundary zone", who);
    if (s.ime < s.ims || s.jme < s.jms || s.kme < s.kms) return amt_fail(AMT_ERR_PRECONDITION, "%s: empty memory extents", who);
    const int ihi = s.ite < s.ide - 1 ? s.ite : s.ide - 1, jhi = s.jte < s.jde - 1 ? s.jte : s.jde - 1;
    if (ihi >= s.its && jhi >= s.jts) {
        if (s.its < s.ims || ihi > s.ime || s.jts < s.jms || jhi > s.jme)
            return amt_fail(AMT_ERR_PRECONDITION, "%s: the tile %d:%d, %d:%d is not inside memory %d:%d, %d:%d", who,
                            s.its, ihi, s.jts, jhi, s.ims, s.ime, s.jms, s.jme);
        if (s.kte > s.kts && (s.kts < s.kms || s.kte - 1 > s.kme))
            return amt_fail(AMT_ERR_PRECONDITION, "%s: levels kts:kte-1 = %d:%d are not inside memory kms:kme = %d:%d", who,
                            s.kts, s.kte - 1, s.kms, s.kme);
    }
    *n = bdy_strips(s, strips);
    return AMT_OK;
}

template <typename T>
int bdy_launch(const char *who, const amt_domain &d, int members, const BdyStrip *strips, int nstrips, const BdyArrays &a)
{
    if (members > 65535) return amt_fail(AMT_ERR_PRECONDITION, "%s: %d members: one update launch covers at most 65535", who, members);
    const long idim = d.ime - d.ims + 1, kdim = d.kme - d.kms + 1, jdim = d.jme - d.jms + 1;
    const long nk = d.kte > d.kts ? d.kte - d.kts : 0;
    AmtBdyJobs<T> jobs{};
    jobs.dts = (T)d.dts;
    int n = 0;
    long most = 0;
    constexpr long per = 16 / (long)sizeof(T);
    for (int k = 0; k < nstrips; ++k) {
        const BdyStrip &st = strips[k];
        const long rows = st.j1 - st.j0 + 1, len = st.i1 - st.i0 + 1;
        if (rows < 1 || len < 1) continue;
        const long at2 = (long)(st.j0 - d.jms) * idim + (st.i0 - d.ims);
        const long at3 = ((long)(st.j0 - d.jms) * kdim + (d.kts - d.kms)) * idim + (st.i0 - d.ims);
        auto add = [&](void *dst, const void *tend, long at, long levels, long stride, long row_stride, long member_stride) {
            if (levels < 1) return;
            jobs.dst[n] = static_cast<T *>(dst) + at;
            jobs.tend[n] = static_cast<const T *>(tend) + at;
            jobs.runs[n] = rows * levels;
            jobs.levels[n] = levels;
            jobs.len[n] = (int)len;
            jobs.stride[n] = stride;
            jobs.row_stride[n] = row_stride;
            jobs.member_stride[n] = member_stride;
            const long total = rows * levels * ((len + per - 1) / per);
            most = total > most ? total : most;
            ++n;
        };
        add(a.t, a.ft, at3, nk, idim, kdim * idim, idim * kdim * jdim);
        add(a.mu, a.mu_tend, at2, 1, 0, idim, idim * jdim);
        add(a.muts, a.mu_tend, at2, 1, 0, idim, idim * jdim);
    }
    if (n == 0 || most == 0) return AMT_OK;
    long blocks = (most + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(amt_bdy_kernel<T>, dim3((unsigned)blocks, (unsigned)n, (unsigned)members), dim3(256), 0, d.stream, jobs);
    AMT_HIP(hipGetLastError());
    return AMT_OK;
}

// the checks, then the launch (nothing for an empty zone).  with_device_check: the pointer-level calls, which may be the first
// HIP call of a process, report a missing device themselves -- behind the argument errors, which need none
int bdy_update(const char *who, const amt_domain &d, int members, const BdyArrays &a, bool with_device_check)
{
    if (!a.t || !a.ft || !a.mu || !a.muts || !a.mu_tend) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null array pointer", who);
    BdyStrip strips[4];
    int n = 0;
    const int rc = bdy_check(who, members, d, strips, &n);
    if (rc != AMT_OK || n == 0) return rc;
    if (with_device_check) {
        int ndev = 0;
        AMT_HIP(hipGetDeviceCount(&ndev));
        if (ndev < 1) return amt_fail(AMT_ERR_NO_DEVICE, "no HIP device visible");
    }
    return d.dtype_bytes == 8 ? bdy_launch<double>(who, d, members, strips, n, a) : bdy_launch<float>(who, d, members, strips, n, a);
}

int bdy_update_device(const char *who, void *hip_stream, int members, amt_domain d, double dts, const BdyArrays &a)
{
    d.stream = static_cast<hipStream_t>(hip_stream);
    d.dts = dts;
    return bdy_update(who, d, members, a, true);
}
}  // namespace

// what the handles and the steppers call: one update of `members` member-stacked patches of the domain's shape, on the
// domain's stream, with the domain's dts
int amt_bdy_update_domain(const char *who, amt_domain *d, int members)
{
    return bdy_update(who, *d, members, BdyArrays{d->field[AMT_F_T], d->field[AMT_F_FT], d->field[AMT_F_MU], d->field[AMT_F_MUTS], d->field[AMT_F_MU_TEND]}, false);
}

// the checks alone (amt_*_set_spec_bdy: a combination the handle does not admit is refused when it is set)
int amt_bdy_check_domain(const char *who, const amt_domain *d, int members)
{
    BdyStrip strips[4];
    int n = 0;
    return bdy_check(who, members, *d, strips, &n);
}

#define AMT_BDY_SIG(T)                                                                                         \
    void *hip_stream, int members, T *t, const T *ft, T *mu, T *muts, const T *mu_tend, T dts,                 \
    int periodic_x, int specified, int nested, int ids, int ide, int jds, int jde, int kde,                    \
    int ims, int ime, int jms, int jme, int kms, int kme, int its, int ite, int jts, int jte, int kts, int kte
// a stack amt_domain that holds the element size and the bounds only: its first members, in the order of the arguments
#define AMT_BDY_BOUNDS(T)                                                                                      \
    amt_domain{(int)sizeof(T), periodic_x, specified, nested, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte}

extern "C" int amt_spec_bdy_update_device_f32(AMT_BDY_SIG(float))
{
    return bdy_update_device("amt_spec_bdy_update_device_f32", hip_stream, members, AMT_BDY_BOUNDS(float), (double)dts, BdyArrays{t, ft, mu, muts, mu_tend});
}
extern "C" int amt_spec_bdy_update_device_f64(AMT_BDY_SIG(double))
{
    return bdy_update_device("amt_spec_bdy_update_device_f64", hip_stream, members, AMT_BDY_BOUNDS(double), dts, BdyArrays{t, ft, mu, muts, mu_tend});
}
