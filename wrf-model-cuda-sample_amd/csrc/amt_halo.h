// amt_halo.h -- what crosses a patch edge, and the one kernel that moves it (not installed).  Everything that packs, unpacks,
// refreshes or poisons halo cells -- the exchange segments and column buffers of amt_grid.hip, the host-owned messages
// (DESIGN.md section 7.5), the cyclic refresh (amt_cyclic.hip, section 7.4), amt_domain_poison_halos -- reads THIS table and
// launches amt_halo.hip's kernel (the poison: a fill of its own over the same cells).  The one-shot host call (amt_oneshot.hip)
// reads the two row lists to know which arrays go up with a halo row.
#pragma once
#include "amt_internal.h"

// The sides in the order of the messages; AMT_SIDE_* (enum amt_sides) is 1 << index, and side ^ 1 is the opposite side.
enum { AMT_HALO_BELOW = 0, AMT_HALO_ABOVE = 1, AMT_HALO_LEFT = 2, AMT_HALO_RIGHT = 3, AMT_HALO_SIDES = 4 };
inline int amt_halo_side_index(int side_flag) { return __builtin_ctz((unsigned)side_flag); }
inline bool amt_halo_is_column(int side) { return side >= AMT_HALO_LEFT; }      // LEFT / RIGHT: a column; BELOW / ABOVE: a row

// The fields a patch RECEIVES INTO ITS HALO from each side (the stencil reads (i+-1, j) and (i, j+-1) only, no diagonals); what
// it SENDS towards a side is the receive list of the opposite side.  The order inside a list is the order of the fields inside
// a packed column buffer and inside a message: 3-D fields first.
struct AmtHaloFields {
    int n;
    int field[5];
};
constexpr AmtHaloFields kAmtHaloRecv[AMT_HALO_SIDES] = {
    {1, {AMT_F_T_1}},                                                      // row jts-1      module_small_step_em.f90:242
    {5, {AMT_F_V, AMT_F_V_1, AMT_F_T_1, AMT_F_MUV, AMT_F_MSFVX_INV}},      // row jte+1      :143-144, :241
    {1, {AMT_F_T_1}},                                                      // column its-1   :245
    {5, {AMT_F_U, AMT_F_U_1, AMT_F_T_1, AMT_F_MUU, AMT_F_MSFUY}},          // column ite+1   :145-146, :244
};
inline const AmtHaloFields &amt_halo_recv(int side) { return kAmtHaloRecv[side]; }
inline const AmtHaloFields &amt_halo_sent(int side) { return kAmtHaloRecv[side ^ 1]; }

inline bool amt_halo_receives(int side, int f)
{
    for (int q = 0; q < kAmtHaloRecv[side].n; ++q)
        if (kAmtHaloRecv[side].field[q] == f) return true;
    return false;
}

// memory levels of a field: kdim for a 3-D one, 1 for a 2-D one
inline long amt_halo_levels(int f, long kdim) { return amt_field_rank(f) == 3 ? kdim : 1; }
// how many fields of that rank the side receives
inline int amt_halo_count(int side, int rank)
{
    int n = 0;
    for (int q = 0; q < kAmtHaloRecv[side].n; ++q) n += amt_field_rank(kAmtHaloRecv[side].field[q]) == rank;
    return n;
}
// elements received from `side` per unit of edge length (per column of a row, per row of a column)
inline long amt_halo_elems(int side, long kdim) { return amt_halo_count(side, 3) * kdim + amt_halo_count(side, 2); }
// memory offset, in elements, of element (i, kms, j) of 3-D field f / (i, j) of 2-D field f in a patch of d's bounds
inline long amt_halo_at(const amt_domain &d, int f, int i, int j)
{
    const long idim = d.ime - d.ims + 1, kdim = d.kme - d.kms + 1;
    return (long)(j - d.jms) * amt_halo_levels(f, kdim) * idim + (i - d.ims);
}

// One launch moves up to AMT_HALO_MAX_JOBS jobs, for `members` member-stacked patches: job q copies `runs` runs of `len`
// elements, run r of member m from src + m * member_stride + r * src_stride to dst + m * member_stride + r * dst_stride
// (all in elements of dtype_bytes).  With idim = elements of a memory row of i:
//   pack (array -> dense message):     src_stride = idim, dst_stride = len       unpack: the reverse
//   cyclic refresh (array -> array):   both idim, member_stride = the field's elements per member
//   a row of a 3-D field:    runs = kdim (one per level),  len = its columns     (2-D: runs = 1)
//   a column of a 3-D field: runs = kdim * rows,           len = 1               (2-D: runs = rows; consecutive memory rows of i)
enum { AMT_HALO_MAX_JOBS = 12 };          // 5 + 1 row fields and 5 + 1 column fields
struct AmtHaloJob {
    const void *src;
    void *dst;
    long runs;
    int len;
    long src_stride, dst_stride, member_stride;
};
int amt_halo_launch(hipStream_t stream, int dtype_bytes, int members, const AmtHaloJob *jobs, int n);
