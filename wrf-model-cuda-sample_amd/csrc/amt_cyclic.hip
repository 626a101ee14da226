// amt_cyclic.hip -- cyclic (periodic) lateral boundaries refreshed on the device (include/amt_advance_mu_t.h section 9,
// DESIGN.md section 7.4).  advance_mu_t reads one cell past its compute window i_start..i_end, j_start..j_end: the halo cells
// and fields of amt_halo.h's table.
// On a domain that is periodic in a direction and held whole in that direction by ONE patch those cells are copies of the
// patch's own first / last column or row (in WRF the periodic-boundary exchange writes them before every call):
//   cyclic x, period ide - ids: column ide <- column ids (the five fields), column ids-1 <- column ide-1 (t_1), rows
//                               j_start..j_end, every memory level
//   cyclic y, period jde - jds: row jde <- row jds (the five fields), row jds-1 <- row jde-1 (t_1), columns i_start..i_end,
//                               every memory level
// The stencil reads no diagonals: corner cells are not written, no cell is written by two copies and no copy reads a cell
// another one writes, so ONE launch does a whole refresh -- up to 6 column and 6 row jobs, times the members of an ensemble.
#include "amt_halo.h"

namespace {
// Argument and precondition checks: host arithmetic only.  *empty: the compute window holds no column, nothing to refresh.
int cyclic_check(const char *who, int axes, int members, const amt_domain &s, AmtWindow &w, bool *empty)
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

// One launch of the mover (amt_halo.hip) for every cyclic direction, all members.  d: bounds, dtype_bytes, stream and the
// pointers of the fields that wrap (a handle's own amt_domain, or a stack one that holds nothing else).
int cyclic_refresh(const char *who, const amt_domain &d, int axes, int members)
{
    AmtWindow w;
    bool empty = false;
    const int rc = cyclic_check(who, axes, members, d, w, &empty);
    if (rc != AMT_OK || empty || axes == 0) return rc;
    if (members > 65535) return amt_fail(AMT_ERR_PRECONDITION, "%s: %d members: one refresh launch covers at most 65535", who, members);
    const long idim = d.ime - d.ims + 1, kdim = d.kme - d.kms + 1;
    const long nrows = w.j_end - w.j_start + 1;
    const int ncols = w.i_end - w.i_start + 1;
    const size_t es = (size_t)d.dtype_bytes;
    AmtHaloJob jobs[AMT_HALO_MAX_JOBS];
    int n = 0;
    for (int side : {AMT_HALO_RIGHT, AMT_HALO_LEFT, AMT_HALO_ABOVE, AMT_HALO_BELOW}) {
        const bool column = amt_halo_is_column(side);
        if (!(axes & (column ? AMT_CYCLIC_X : AMT_CYCLIC_Y))) continue;
        // the halo cell of that side <- the patch's own cell one period away: column ide <- ids, ids-1 <- ide-1, row jde <- jds,
        // jds-1 <- jde-1
        const bool high = side == AMT_HALO_RIGHT || side == AMT_HALO_ABOVE;
        const int si = column ? (high ? d.ids : d.ide - 1) : w.i_start, di = column ? (high ? d.ide : d.ids - 1) : w.i_start;
        const int sj = column ? w.j_start : (high ? d.jds : d.jde - 1), dj = column ? w.j_start : (high ? d.jde : d.jds - 1);
        for (int q = 0; q < amt_halo_recv(side).n; ++q) {
            const int f = amt_halo_recv(side).field[q];
            if (!d.field[f]) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null array pointer (field %d)", who, f);
            char *base = static_cast<char *>(d.field[f]);
            const long levels = amt_halo_levels(f, kdim);
            jobs[n++] = AmtHaloJob{base + (size_t)amt_halo_at(d, f, si, sj) * es, base + (size_t)amt_halo_at(d, f, di, dj) * es,
                                   column ? nrows * levels : levels, column ? 1 : ncols, idim, idim, (long)d.count(f)};
        }
    }
    return amt_halo_launch(d.stream, d.dtype_bytes, members, jobs, n);
}

int cyclic_fill_device(const char *who, void *hip_stream, int axes, int members, amt_domain d,
                       const void *u, const void *u_1, const void *v, const void *v_1, const void *t_1,
                       const void *muu, const void *muv, const void *msfuy, const void *msfvx_inv)
{
    d.stream = static_cast<hipStream_t>(hip_stream);
    d.field[AMT_F_U] = const_cast<void *>(u); d.field[AMT_F_U_1] = const_cast<void *>(u_1);
    d.field[AMT_F_V] = const_cast<void *>(v); d.field[AMT_F_V_1] = const_cast<void *>(v_1);
    d.field[AMT_F_T_1] = const_cast<void *>(t_1);
    d.field[AMT_F_MUU] = const_cast<void *>(muu); d.field[AMT_F_MUV] = const_cast<void *>(muv);
    d.field[AMT_F_MSFUY] = const_cast<void *>(msfuy); d.field[AMT_F_MSFVX_INV] = const_cast<void *>(msfvx_inv);
    AmtWindow w;
    bool empty = false;
    const int rc = cyclic_check(who, axes, members, d, w, &empty);      // argument errors are reported with or without a device
    if (rc != AMT_OK) return rc;
    int ndev = 0;
    AMT_HIP(hipGetDeviceCount(&ndev));
    if (ndev < 1) return amt_fail(AMT_ERR_NO_DEVICE, "no HIP device visible");
    return cyclic_refresh(who, d, axes, members);
}
}  // namespace

// what the handles call: one refresh of `members` member-stacked patches of the domain's shape, on the domain's stream
int amt_cyclic_refresh_domain(const char *who, amt_domain *d, int axes, int members) { return cyclic_refresh(who, *d, axes, members); }

// the checks alone (amt_*_set_cyclic: a combination the handle's shape does not admit is refused when it is set)
int amt_cyclic_check_domain(const char *who, const amt_domain *d, int axes, int members)
{
    AmtWindow w;
    bool empty = false;
    return cyclic_check(who, axes, members, *d, w, &empty);
}

#define AMT_CYCLIC_SIG(T)                                                                                     \
    void *hip_stream, int axes, int members, T *u, T *u_1, T *v, T *v_1, T *t_1, T *muu, T *muv, T *msfuy,    \
    T *msfvx_inv, int periodic_x, int specified, int nested, int ids, int ide, int jds, int jde, int kde,     \
    int ims, int ime, int jms, int jme, int kms, int kme, int its, int ite, int jts, int jte, int kts, int kte
// a stack amt_domain that holds the element size and the bounds only: its first members, in the order of the arguments
#define AMT_CYCLIC_BOUNDS(T)                                                                                  \
    amt_domain{(int)sizeof(T), periodic_x, specified, nested, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte}

extern "C" int amt_cyclic_fill_device_f32(AMT_CYCLIC_SIG(float))
{
    return cyclic_fill_device("amt_cyclic_fill_device_f32", hip_stream, axes, members, AMT_CYCLIC_BOUNDS(float), u, u_1, v, v_1, t_1, muu, muv, msfuy, msfvx_inv);
}
extern "C" int amt_cyclic_fill_device_f64(AMT_CYCLIC_SIG(double))
{
    return cyclic_fill_device("amt_cyclic_fill_device_f64", hip_stream, axes, members, AMT_CYCLIC_BOUNDS(double), u, u_1, v, v_1, t_1, muu, muv, msfuy, msfvx_inv);
}
