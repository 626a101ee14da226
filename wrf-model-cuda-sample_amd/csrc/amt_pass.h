// amt_pass.h -- what the streaming passes around the acoustic loop (amt_sumflux.hip, amt_stage.hip, amt_p_rho.hip; DESIGN.md
// section 7.10) share on the host.  No device code.  Included by amt_internal.h behind amt_domain; everything here is hidden.
#pragma once
#include <functional>
#pragma GCC visibility push(hidden)

// ---- the check: host arithmetic only; *empty: there is no cell to work on, the call enqueues nothing ---------------------
// One array of a call.  rank 3 and 2: one field's extents times the members; rank 1: kdim elements, shared by the members.
// An output may overlap no other array of the call, inputs may alias one another; an optional array may be NULL.
struct AmtPassArray { const void *p; int rank; bool output, optional; };
// where the passes differ: the levels kts..kte a tile needs to hold a cell, whether a tile without a mass column
// (its..min(ite, ide-1), jts..min(jte, jde-1)) holds none, and the texts of the overlap refusal
struct AmtPassRules { int min_levels; bool needs_mass_column; const char *output_overlaps_output, *output_overlaps_input; };
// Two calls, a pass checks its own scalar arguments between them.  _arrays: a NULL array that is not optional, then members >= 1
// (INVALID_ARG).  _box: empty memory extents (PRECONDITION), an output that overlaps (INVALID_ARG), kts == 1, kte == kde, the levels
// inside memory, the empty tile (*empty), the tile inside memory, members <= 65535 (PRECONDITION), the empty mass range (*empty).
int amt_pass_check_arrays(const char *who, int members, const AmtPassArray *arr, int narr);
int amt_pass_check_box(const char *who, const amt_domain &s, int members, const AmtPassArray *arr, int narr, const AmtPassRules &rules,
                       bool *empty);

// ---- the layout, into the six members every pass's job struct names the same: element (i, k, j) of member m of a 3-D array is
// at m * mstride3 + (j - jts) * jstride3 + (k - kts) * idim + (i - its) + first3, of a 2-D array at m * mstride2 +
// (j - jts) * idim + (i - its) + first2 ---------------------------------------------------------------------------------
template <typename Job>
inline void amt_pass_set_layout(const amt_domain &d, Job &job)
{
    const long idim = d.ime - d.ims + 1, kdim = d.kme - d.kms + 1, jdim = d.jme - d.jms + 1;
    job.idim = idim; job.jstride3 = kdim * idim; job.mstride3 = idim * kdim * jdim; job.mstride2 = idim * jdim;
    job.first3 = ((long)(d.jts - d.jms) * kdim + (d.kts - d.kms)) * idim + (d.its - d.ims);
    job.first2 = (long)(d.jts - d.jms) * idim + (d.its - d.ims);
}
// the columns of the mass range inside the tile: min(ite, ide-1) - its + 1 and its j twin; <= 0: none
void amt_pass_mass_lengths(const amt_domain &d, int *ni, int *nj);
// blocks of 256 threads for `items` work items: at least 1, at most 1024 (the kernels stride over the rest; amt_p_rho.hip counts waves)
unsigned amt_pass_blocks(long items);

// ---- from the check to the launch.  A pointer-level call may be the first HIP call of a process and reports a missing device
// itself -- behind the argument errors, which need none; it runs on the caller's current device -----------------------------
int amt_pass_current_device(int *device);
// rc, empty: what the pass's check answered.  launch(T()) enqueues the pass for the arrays' type T on d.stream, with the
// device current: the caller's for a pointer-level call, the handle's otherwise.
template <typename Launch>
inline int amt_pass_run(int rc, bool empty, const amt_domain &d, bool pointer_level, Launch launch)
{
    if (rc != AMT_OK || empty) return rc;
    int device = d.device;
    if (pointer_level && (rc = amt_pass_current_device(&device)) != AMT_OK) return rc;
    DeviceScope scope(device);
    return d.dtype_bytes == 8 ? launch(double()) : launch(float());
}

// ---- the arrays a setting keeps in its handle: the caller's or, when the caller gives none, the library's -------------------
struct AmtPassSetting {
    void **slot; bool *owned; int count;   // the `count` pointers in the amt_domain; owned: allocated by the library
    size_t bytes[9];                       // of array k, when the library allocates
    // "give all <three accumulators> or none", "<an accumulator> the library allocated, mixed with others", "the handle's
    // tile does not admit <the flux averages>", "no room for <three arrays> of %zu bytes"
    const char *all_of_them, *one_of_them, *pass, *room;
};
// _offer:   all `count` arrays or none (INVALID_ARG).  *given: 0 or count; *same: they are the library's own, handed back in their
//           order -- what that means is the pass's to say.
// _take:    one of the library's arrays among the caller's (INVALID_ARG; it would be freed under the caller); the caller's arrays
//           through check(arr), the pass's check on a copy of the handle that holds them; without arrays members <= 65535 and a
//           tile that admits the pass (PRECONDITION), then the allocation (AMT_ERR_ALLOC).  Then, unless `same`, the old arrays
//           are released and the new ones are the handle's.  A refusal changes nothing.
// _release: frees what the library allocated; the slot is empty afterwards.
int amt_pass_setting_offer(const char *who, const AmtPassSetting &s, void *const *arr, int *given, bool *same);
int amt_pass_setting_take(const char *who, const amt_domain *d, int members, const AmtPassSetting &s, void *const *arr, int given,
                          bool same, const std::function<int(void *const *)> &check);
void amt_pass_setting_release(const AmtPassSetting &s);

// ---- the 17 bounds that close the pointer-level exports' signatures, and the handle-less amt_domain those exports run on ----
#define AMT_BOUNDS_SIG                                                                                          \
    int ids, int ide, int jds, int jde, int kde, int ims, int ime, int jms, int jme, int kms, int kme,          \
    int its, int ite, int jts, int jte, int kts, int kte
#define AMT_BOUNDS_ARGS ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte
amt_domain amt_pass_domain(int dtype_bytes, void *hip_stream, AMT_BOUNDS_SIG);
#pragma GCC visibility pop
