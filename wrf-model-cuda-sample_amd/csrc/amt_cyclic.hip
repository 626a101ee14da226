// amt_cyclic.hip -- cyclic (periodic) lateral boundaries refreshed on the device (include/amt_advance_mu_t.h section 9,
// DESIGN.md section 7.4).  advance_mu_t reads one cell past its compute window i_start..i_end, j_start..j_end:
//   column i_end+1 of u, u_1, t_1, muu, msfuy      module_small_step_em.f90:145-146, :244
//   column i_start-1 of t_1                         :245
//   row j_end+1 of v, v_1, t_1, muv, msfvx_inv      :143-144, :241
//   row j_start-1 of t_1                            :242
// On a domain that is periodic in a direction and held whole in that direction by ONE patch those cells are copies of the
// patch's own first / last column or row (in WRF the periodic-boundary exchange writes them before every call):
//   cyclic x, period ide - ids: column ide <- column ids (the five fields), column ids-1 <- column ide-1 (t_1), rows
//                               j_start..j_end, every memory level
//   cyclic y, period jde - jds: row jde <- row jds (the five fields), row jds-1 <- row jde-1 (t_1), columns i_start..i_end,
//                               every memory level
// The stencil reads no diagonals: corner cells are not written, no cell is written by two copies and no copy reads a cell
// another one writes, so ONE launch does a whole refresh -- up to 6 column and 6 row jobs, times the members of an ensemble.
#include "amt_internal.h"

namespace {
typedef unsigned int amt_cyc_v4u __attribute__((ext_vector_type(4)));

// Job q copies `runs` runs of `len` elements; run r starts at src + r * idim and goes to dst + r * idim (idim = elements of
// a memory row of i), member m of an ensemble lies mstride elements further on both sides.
//   a row of a 3-D field:    runs = kdim (one per level),   len = the window's columns  (contiguous: 16-byte pieces)
//   a row of a 2-D field:    runs = 1,                      len = the window's columns
//   a column of a 3-D field: runs = kdim * rows,            len = 1   (levels and rows are consecutive memory rows of i)
//   a column of a 2-D field: runs = rows,                   len = 1
// vec = 1: every run of the job starts on a 16-byte boundary on both sides, in every member; its first nvec 16-byte pieces
// move as such and the `tail` elements behind them one by one.  vec = 0: element accesses only.
template <typename W>
struct AmtCyclicJobs {
    const W *src[12];
    W *dst[12];
    long runs[12];
    long mstride[12];
    int len[12];
    int vec[12];
    long idim;
    int n;
};

// Lanes run along (piece of a run, run): along i for a row, along (level, row) for a column -- one line per element there,
// which is what a column is.  The elements move as unsigned integers: every bit pattern, NaN payloads included, arrives as
// it left.  256 threads, no LDS, a handful of registers: a workgroup of this kernel takes a sliver of a compute unit.
template <typename W>
__global__ __launch_bounds__(256) void amt_cyclic_kernel(AmtCyclicJobs<W> jobs)
{
    constexpr int kPer = 16 / (int)sizeof(W);                  // elements per 16-byte piece
    const int q = blockIdx.y;
    const long moff = (long)blockIdx.z * jobs.mstride[q];
    const W *src = jobs.src[q] + moff;
    W *dst = jobs.dst[q] + moff;
    const long len = jobs.len[q];
    const long nvec = jobs.vec[q] ? len / kPer : 0;
    const long units = nvec + (len - nvec * kPer);             // work items of one run: 16-byte pieces, then single elements
    const long total = jobs.runs[q] * units;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long r = e / units, p = e - r * units;
        const long base = r * jobs.idim;
        if (p < nvec) {
            const amt_cyc_v4u *s16 = reinterpret_cast<const amt_cyc_v4u *>(src + base) + p;
            amt_cyc_v4u *d16 = reinterpret_cast<amt_cyc_v4u *>(dst + base) + p;
            *d16 = *s16;
        } else {
            const long i = nvec * kPer + (p - nvec);
            dst[base + i] = src[base + i];
        }
    }
}

struct CyclicShape {
    int periodic_x, specified, nested;
    int ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte;
};

// Argument and precondition checks: host arithmetic only.  *empty: the compute window holds no column, nothing to refresh.
int cyclic_check(const char *who, int axes, int members, const CyclicShape &s, AmtWindow &w, bool *empty)
{
    if (axes < 0 || (axes & ~(AMT_CYCLIC_X | AMT_CYCLIC_Y)))
        return amt_fail(AMT_ERR_INVALID_ARG, "%s: axes = %d is not a combination of AMT_CYCLIC_X and AMT_CYCLIC_Y", who, axes);
    if (members < 1) return amt_fail(AMT_ERR_INVALID_ARG, "%s: members = %d: an ensemble has at least one member", who, members);
    if (s.ime < s.ims || s.jme < s.jms || s.kme < s.kms) return amt_fail(AMT_ERR_PRECONDITION, "%s: empty memory extents", who);
    if ((long)members * (s.jme - s.jms + 1) > 0x7fffffffL)
        return amt_fail(AMT_ERR_PRECONDITION, "%s: %d members of %d rows: the stacked arrays have more than 2^31 - 1 rows", who, members, s.jme - s.jms + 1);
    w = amt_window(s.periodic_x, s.specified, s.nested, s.ids, s.ide, s.jds, s.jde, s.its, s.ite, s.jts, s.jte, s.kts, s.kte);
    *empty = (w.i_end < w.i_start) || (w.j_end < w.j_start);
    const bool clipped = s.specified || s.nested;
    if ((axes & AMT_CYCLIC_X) && !s.periodic_x && clipped)
        return amt_fail(AMT_ERR_PRECONDITION, "%s: cyclic x needs an unclipped i window: periodic_x, or neither specified nor nested", who);
    if ((axes & AMT_CYCLIC_Y) && clipped)
        return amt_fail(AMT_ERR_PRECONDITION, "%s: cyclic y needs an unclipped j window: neither specified nor nested", who);
    if (*empty) return AMT_OK;
    if (w.i_start < s.ims || w.i_end > s.ime || w.j_start < s.jms || w.j_end > s.jme)
        return amt_fail(AMT_ERR_PRECONDITION, "%s: the compute window %d:%d, %d:%d is not inside memory %d:%d, %d:%d", who,
                        w.i_start, w.i_end, w.j_start, w.j_end, s.ims, s.ime, s.jms, s.jme);
    if (axes & AMT_CYCLIC_X) {
        // the window decides, not ite: a last patch may end at ide-1 or at ide
        if (w.i_start != s.ids || w.i_end != s.ide - 1)
            return amt_fail(AMT_ERR_PRECONDITION, "%s: cyclic x needs the whole period in one patch: the i window is %d:%d, the domain's "
                            "columns are %d:%d", who,
                            w.i_start, w.i_end, s.ids, s.ide - 1);
        if (s.ids - 1 < s.ims || s.ide > s.ime)
            return amt_fail(AMT_ERR_PRECONDITION, "%s: memory ims:ime=%d:%d does not hold the cyclic columns ids-1=%d and ide=%d", who,
                            s.ims, s.ime, s.ids - 1, s.ide);
    }
    if (axes & AMT_CYCLIC_Y) {
        if (w.j_start != s.jds || w.j_end != s.jde - 1)
            return amt_fail(AMT_ERR_PRECONDITION, "%s: cyclic y needs the whole period in one patch: the j window is %d:%d, the domain's "
                            "rows are %d:%d", who,
                            w.j_start, w.j_end, s.jds, s.jde - 1);
        if (s.jds - 1 < s.jms || s.jde > s.jme)
            return amt_fail(AMT_ERR_PRECONDITION, "%s: memory jms:jme=%d:%d does not hold the cyclic rows jds-1=%d and jde=%d", who,
                            s.jms, s.jme, s.jds - 1, s.jde);
    }
    return AMT_OK;
}

const int kCyclicFromRight[] = {AMT_F_U, AMT_F_U_1, AMT_F_T_1, AMT_F_MUU, AMT_F_MSFUY};        // column ide <- column ids
const int kCyclicFromLeft[] = {AMT_F_T_1};                                                       // column ids-1 <- column ide-1
const int kCyclicFromAbove[] = {AMT_F_V, AMT_F_V_1, AMT_F_T_1, AMT_F_MUV, AMT_F_MSFVX_INV};      // row jde <- row jds
const int kCyclicFromBelow[] = {AMT_F_T_1};                                                      // row jds-1 <- row jde-1

template <typename W>
int cyclic_launch(hipStream_t stream, int axes, int members, void *const *field, const CyclicShape &s, const AmtWindow &w)
{
    const long idim = s.ime - s.ims + 1, kdim = s.kme - s.kms + 1, jdim = s.jme - s.jms + 1;
    AmtCyclicJobs<W> jobs{};
    jobs.idim = idim;
    long most = 0;
    auto add = [&](int f, long src_off, long dst_off, long runs, int len) {
        const int q = jobs.n++;
        const bool r3 = amt_field_rank(f) == 3;
        const W *base = static_cast<const W *>(field[f]);
        jobs.src[q] = base + src_off;
        jobs.dst[q] = static_cast<W *>(field[f]) + dst_off;
        jobs.runs[q] = runs;
        jobs.len[q] = len;
        jobs.mstride[q] = jdim * (r3 ? kdim : 1) * idim;
        // 16-byte pieces where BOTH ends of every run are 16-byte aligned: the first run of member 0, and with it every other
        // one when the distances between runs and between members are multiples of 16 bytes
        const uintptr_t a = reinterpret_cast<uintptr_t>(jobs.src[q]) | reinterpret_cast<uintptr_t>(jobs.dst[q]);
        const bool strides_ok = (runs == 1 || (idim * sizeof(W)) % 16 == 0) && (members == 1 || (jobs.mstride[q] * sizeof(W)) % 16 == 0);
        jobs.vec[q] = (len >= (int)(16 / sizeof(W)) && (a & 15) == 0 && strides_ok) ? 1 : 0;
        const long nvec = jobs.vec[q] ? len / (long)(16 / sizeof(W)) : 0;
        const long total = runs * (nvec + (len - nvec * (long)(16 / sizeof(W))));
        most = total > most ? total : most;
    };
    // memory offset of element (i, kms, j) of a 3-D field / (i, j) of a 2-D one
    auto at = [&](int f, int i, int j) { return ((long)(j - s.jms) * (amt_field_rank(f) == 3 ? kdim : 1)) * idim + (i - s.ims); };
    const long nrows = w.j_end - w.j_start + 1;
    const int ncols = w.i_end - w.i_start + 1;
    if (axes & AMT_CYCLIC_X) {
        for (int f : kCyclicFromRight) add(f, at(f, s.ids, w.j_start), at(f, s.ide, w.j_start), nrows * (amt_field_rank(f) == 3 ? kdim : 1), 1);
        for (int f : kCyclicFromLeft) add(f, at(f, s.ide - 1, w.j_start), at(f, s.ids - 1, w.j_start), nrows * kdim, 1);
    }
    if (axes & AMT_CYCLIC_Y) {
        for (int f : kCyclicFromAbove) add(f, at(f, w.i_start, s.jds), at(f, w.i_start, s.jde), amt_field_rank(f) == 3 ? kdim : 1, ncols);
        for (int f : kCyclicFromBelow) add(f, at(f, w.i_start, s.jde - 1), at(f, w.i_start, s.jds - 1), kdim, ncols);
    }
    if (jobs.n == 0 || most == 0) return AMT_OK;
    long blocks = (most + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(amt_cyclic_kernel<W>, dim3((unsigned)blocks, (unsigned)jobs.n, (unsigned)members), dim3(256), 0, stream, jobs);
    AMT_HIP(hipGetLastError());
    return AMT_OK;
}

int cyclic_refresh(const char *who, hipStream_t stream, int axes, int members, int dtype_bytes, void *const *field, const CyclicShape &s)
{
    AmtWindow w;
    bool empty = false;
    const int rc = cyclic_check(who, axes, members, s, w, &empty);
    if (rc != AMT_OK || empty || axes == 0) return rc;
    if (members > 65535) return amt_fail(AMT_ERR_PRECONDITION, "%s: %d members: one refresh launch covers at most 65535", who, members);
    if (axes & AMT_CYCLIC_X) {
        for (int f : kCyclicFromRight) if (!field[f]) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null array pointer (field %d)", who, f);
        for (int f : kCyclicFromLeft) if (!field[f]) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null array pointer (field %d)", who, f);
    }
    if (axes & AMT_CYCLIC_Y) {
        for (int f : kCyclicFromAbove) if (!field[f]) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null array pointer (field %d)", who, f);
        for (int f : kCyclicFromBelow) if (!field[f]) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null array pointer (field %d)", who, f);
    }
    return dtype_bytes == 8 ? cyclic_launch<uint64_t>(stream, axes, members, field, s, w)
                            : cyclic_launch<uint32_t>(stream, axes, members, field, s, w);
}

CyclicShape shape_of(const amt_domain *d)
{
    return CyclicShape{d->periodic_x, d->specified, d->nested, d->ids, d->ide, d->jds, d->jde, d->kde, d->ims, d->ime,
                       d->jms, d->jme, d->kms, d->kme, d->its, d->ite, d->jts, d->jte, d->kts, d->kte};
}

int cyclic_fill_device(const char *who, void *hip_stream, int axes, int members, int dtype_bytes,
                       const void *u, const void *u_1, const void *v, const void *v_1, const void *t_1,
                       const void *muu, const void *muv, const void *msfuy, const void *msfvx_inv, const CyclicShape &s)
{
    void *field[AMT_F_COUNT] = {};
    field[AMT_F_U] = const_cast<void *>(u); field[AMT_F_U_1] = const_cast<void *>(u_1);
    field[AMT_F_V] = const_cast<void *>(v); field[AMT_F_V_1] = const_cast<void *>(v_1);
    field[AMT_F_T_1] = const_cast<void *>(t_1);
    field[AMT_F_MUU] = const_cast<void *>(muu); field[AMT_F_MUV] = const_cast<void *>(muv);
    field[AMT_F_MSFUY] = const_cast<void *>(msfuy); field[AMT_F_MSFVX_INV] = const_cast<void *>(msfvx_inv);
    AmtWindow w;
    bool empty = false;
    const int rc = cyclic_check(who, axes, members, s, w, &empty);      // argument errors are reported with or without a device
    if (rc != AMT_OK) return rc;
    int ndev = 0;
    AMT_HIP(hipGetDeviceCount(&ndev));
    if (ndev < 1) return amt_fail(AMT_ERR_NO_DEVICE, "no HIP device visible");
    return cyclic_refresh(who, static_cast<hipStream_t>(hip_stream), axes, members, dtype_bytes, field, s);
}
}  // namespace

// what the handles call: one refresh of `members` member-stacked patches of the domain's shape, on the domain's stream
int amt_cyclic_refresh_domain(const char *who, amt_domain *d, int axes, int members)
{
    return cyclic_refresh(who, d->stream, axes, members, d->dtype_bytes, d->field, shape_of(d));
}

// the checks alone (amt_*_set_cyclic: a combination the handle's shape does not admit is refused when it is set)
int amt_cyclic_check_domain(const char *who, const amt_domain *d, int axes, int members)
{
    AmtWindow w;
    bool empty = false;
    return cyclic_check(who, axes, members, shape_of(d), w, &empty);
}

#define AMT_CYCLIC_SIG(T)                                                                                     \
    void *hip_stream, int axes, int members, T *u, T *u_1, T *v, T *v_1, T *t_1, T *muu, T *muv, T *msfuy,    \
    T *msfvx_inv, int periodic_x, int specified, int nested, int ids, int ide, int jds, int jde, int kde,     \
    int ims, int ime, int jms, int jme, int kms, int kme, int its, int ite, int jts, int jte, int kts, int kte
#define AMT_CYCLIC_SHAPE                                                                                      \
    CyclicShape{periodic_x, specified, nested, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte}

extern "C" int amt_cyclic_fill_device_f32(AMT_CYCLIC_SIG(float))
{
    return cyclic_fill_device("amt_cyclic_fill_device_f32", hip_stream, axes, members, 4, u, u_1, v, v_1, t_1, muu, muv, msfuy, msfvx_inv, AMT_CYCLIC_SHAPE);
}
extern "C" int amt_cyclic_fill_device_f64(AMT_CYCLIC_SIG(double))
{
    return cyclic_fill_device("amt_cyclic_fill_device_f64", hip_stream, axes, members, 8, u, u_1, v, v_1, t_1, muu, muv, msfuy, msfvx_inv, AMT_CYCLIC_SHAPE);
}
