/*
 * include/amt_advance_mu_t.h -- C-ABI of the MI355X (gfx950) advance_mu_t path.
 *
 * Drop-in boundary for WRF-ARW's acoustic-substep routine
 *   SUBROUTINE advance_mu_t(ww, ww_1, u, u_1, v, v_1, mu, mut, muave, muts, muu,
 *                           muv, mudf, t, t_1, t_ave, ft, mu_tend, rdx, rdy, dts,
 *                           epssm, dnw, fnm, fnp, rdnw, msfuy, msfvx_inv, msftx,
 *                           msfty, config_flags, ids,ide, jds,jde, kde, ims,ime,
 *                           jms,jme, kms,kme, its,ite, jts,jte, kts,kte)
 * (reference: module_small_step_em.f90:7-18; C/CUDA precedent for a flat C
 * signature: advance_mu_t.h:10-23, advance_mu_t_cu.h:3-17).
 *
 * Conventions shared by every entry point
 *  - Argument ORDER is the Fortran one.  config_flags is replaced by the three
 *    logicals the routine reads (module_small_step_em.f90:97-103; the C struct
 *    of advance_mu_t.h:3-8 carries the same three) as int 0/1, in the order
 *    periodic_x, specified, nested.
 *  - All 17 bounds are Fortran-style INCLUSIVE indices passed unchanged; there
 *    is no kds (the Fortran signature has none).  Arrays are i-fastest:
 *    element (i,k,j) of a 3-D array is at ((j-jms)*kdim + (k-kms))*idim + (i-ims),
 *    (i,j) of a 2-D array at (j-jms)*idim + (i-ims), (k) of a 1-D array at k-kms,
 *    with idim = ime-ims+1, kdim = kme-kms+1  (advance_mu_t.c:8-9,33-55).
 *  - Preconditions (anything else is undefined in the Fortran as well, see
 *    DESIGN.md): kts == 1, kte == kde, kms <= 1, kme >= kte, and the compute
 *    window plus its one-cell input halo (i-1, i+1, j-1, j+1) inside memory.
 *    Level count: a column's k chains live in LDS, which holds 320 levels in
 *    fp64 and 640 in fp32 (AMT_ERR_PRECONDITION beyond; WRF runs 30..150).
 *    SPEED CLIFF (a step since r06): the production kernel (AMT_VARIANT_MARCH) keeps four level-by-column
 *    buffers of a tile in the CU's 160 KB of LDS, which ends at 240 levels in fp64 and
 *    264 in fp32 (16-column tiles; a fifth level per lane does not fit).  Beyond that
 *    AMT_VARIANT_AUTO falls back to the column kernel, which re-reads its neighbours and evaluates dvdxi twice instead of
 *    keeping it (nothing in LDS): about 0.41 of the HBM roofline against 0.61-0.75 for the march kernel (until r06: 0.09, one
 *    wave per compute unit under a 150 KB LDS column); the first such call of a process says so
 *    on stderr (AMT_QUIET=1 suppresses it).
 *  - Return value: AMT_OK or an amt_status code; nothing ever calls exit()
 *    (the reference's wrapper prints and exit(1)s, advance_mu_t_no_async.cu:22-32,
 *    82-85).  amt_last_error() gives the text for the calling thread.
 *  - Outputs outside the compute window, and level k = kte, keep the caller's
 *    contents (the reference uploads its OUT arrays for the same reason,
 *    advance_mu_t_no_async.cu:259,270-272).  Section (12) advances the ring a
 *    specified / nested domain's window leaves out.
 *  - Calls on the same stream/handle are not re-entrant; different streams are
 *    independent.
 *
 * There is no CPU fallback anywhere behind this header: without a HIP device
 * every compute entry point returns AMT_ERR_NO_DEVICE / AMT_ERR_HIP.
 */
#ifndef AMT_ADVANCE_MU_T_H
#define AMT_ADVANCE_MU_T_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum amt_status {
    AMT_OK = 0,
    AMT_ERR_HIP = 1,           /* a HIP runtime call failed (text in amt_last_error) */
    AMT_ERR_PRECONDITION = 2,  /* bounds violate the preconditions above            */
    AMT_ERR_INVALID_ARG = 3,   /* null pointer, bad dtype / field id / variant      */
    AMT_ERR_NO_DEVICE = 4,     /* no gfx950 device visible                          */
    AMT_ERR_ALLOC = 5,         /* device or host allocation failed                  */
    AMT_ERR_COMM = 6,          /* RCCL could not be loaded or a collective call failed */
    AMT_ERR_NONFINITE = 7      /* the non-finite guard of section (10) found a NaN or Inf in ww, t or mu */
} amt_status;

/* Kernel variants (amt_set_variant / `variant` arguments).  AMT_VARIANT_AUTO picks
 * the fastest one that supports the given shape. */
enum amt_variant {
    AMT_VARIANT_AUTO = 0,
    AMT_VARIANT_COLUMN = 1,    /* one lane per (i,j) column, k-column staged in LDS */
    AMT_VARIANT_MARCH = 2      /* (i,k)-cell lanes marching in j, k-chains through LDS */
};
/* OR-ed into the `variant` argument of amt_advance_mu_t_device_*: kernels of ANOTHER stream are meant to run beside this
 * launch (a j-slab's interior rows while its halo exchange and edge rows go through a communication stream).  On its own a
 * launch may be planned as ONE round of workgroups that holds every compute unit until it ends; with this flag it is
 * planned in at least two rounds, so that the other stream's kernels get compute units at a round boundary.  Same bits. */
#define AMT_LAUNCH_BESIDE_OTHERS 0x100

const char *amt_version(void);
const char *amt_status_string(int status);
const char *amt_last_error(void);
int amt_device_count(void);               /* number of visible HIP devices, 0 if none */

/* ------------------------------------------------------------------------
 * (1) One-shot drop-ins: HOST arrays in, HOST arrays out.  Replaces the body of
 *     the Fortran routine (module_small_step_em.f90:7-252) and the CUDA host
 *     wrapper (advance_mu_t_no_async.cu:35-424): allocate, upload, launch,
 *     download, free -- on the current HIP device.  Of ww, t and t_ave only the
 *     cells the Fortran assigns (i_start..i_end, 1..kte-1, j_start..j_end) are
 *     written back; t_ave and the levels above 1 of ww are outputs only and are
 *     not uploaded.  Of the 2-D outputs, too, only the window's cells are written
 *     back: host threads that run tiles of one domain concurrently (OpenMP tiles,
 *     split in i or in j) never touch each other's cells.
 * ------------------------------------------------------------------------ */
int amt_advance_mu_t_f32(
    float *ww, const float *ww_1, const float *u, const float *u_1,
    const float *v, const float *v_1,
    float *mu, const float *mut, float *muave, float *muts,
    const float *muu, const float *muv,
    float *mudf, float *t, const float *t_1,
    float *t_ave, const float *ft, const float *mu_tend,
    float rdx, float rdy, float dts, float epssm,
    const float *dnw, const float *fnm, const float *fnp, const float *rdnw,
    const float *msfuy, const float *msfvx_inv,
    const float *msftx, const float *msfty,
    int periodic_x, int specified, int nested,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);

int amt_advance_mu_t_f64(
    double *ww, const double *ww_1, const double *u, const double *u_1,
    const double *v, const double *v_1,
    double *mu, const double *mut, double *muave, double *muts,
    const double *muu, const double *muv,
    double *mudf, double *t, const double *t_1,
    double *t_ave, const double *ft, const double *mu_tend,
    double rdx, double rdy, double dts, double epssm,
    const double *dnw, const double *fnm, const double *fnp, const double *rdnw,
    const double *msfuy, const double *msfvx_inv,
    const double *msftx, const double *msfty,
    int periodic_x, int specified, int nested,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);

/* Page-lock / release a host array (hipHostRegister).  The one-shot calls stream the window in
 * j chunks through an upload, a compute and a download stream so that both directions of the
 * host link and the kernels overlap.  With page-locked 3-D arrays (by these, or allocated pinned
 * by the caller as the reference driver does, advance_mu_t_driver.cu:97-167) every copy is
 * asynchronous; with pageable ones a second host thread issues the downloads and small arrays
 * pass through an internal page-locked staging buffer -- about the same speed for large
 * domains, ~2x slower than pinned for patch-sized ones.  Pin once, outside the time loop. */
int amt_host_pin(void *ptr, size_t bytes);
int amt_host_unpin(void *ptr);

/* One call, several devices.  The reference's host call IS its multi-GPU call: advance_mu_t_no_async.cu:108-162 splits j over
 * its `GPUs` devices inside one advance_mu_t(...), refills every device's halo rows from the host arrays (:135-160), launches and
 * gathers per device (:329-390).  amt_host_set_devices(n, ids) gives the calling host thread n DEVICE SLOTS (ids may name a device
 * more than once); from then on each one-shot call of that thread cuts its tile's rows jts..jte into n contiguous pieces (uneven
 * where they do not divide) and runs them at the same time, one per slot, each piece a tile of the same domain whose halo rows
 * come from the HOST arrays exactly as the reference's do -- no traffic between the devices, same bits as the one-device call.
 * The one-shot path is bound by the host link; a node has one link per device.  Every slot keeps its
 * own workspace, residency cache and deferred outputs on its device; the control calls below (amt_host_cache_*, _invalidate,
 * _defer, _fetch, _stale, _release) act on all slots.  n = 0 turns it off (what the slots' devices alone hold comes down first).
 * AMT_ONESHOT_DEVICES="0,1,2,3" or "all" in the environment does the same for every thread that never calls this (the Fortran
 * drop-in module is one CALL and has nowhere to put another).  amt_host_devices returns the number of slots of the calling thread
 * and their device ids. */
int amt_host_set_devices(int n, const int *device_ids);
int amt_host_devices(int *device_ids, int cap);

/* The one-shot calls keep their device workspace (three streams, six events, the buffer arena
 * when it is at most 1 GiB) per calling host thread between calls, instead of the reference
 * wrapper's allocate-and-free on every call (advance_mu_t_no_async.cu:178-244,392-423), which
 * at WRF patch sizes costs more than the call itself.  This frees the calling thread's
 * workspace now; it is freed anyway when the thread ends. */
int amt_host_release(void);

/* Residency cache of the one-shot calls (per calling host thread; off by default).  In WRF's acoustic loop
 * (solve_em) advance_mu_t is called number_of_small_timesteps times per Runge-Kutta stage with the SAME
 * ww_1, u_1, v_1, t_1 (the `_save` linearisation state) and ft (the tendency): five of the eight 3-D arrays a
 * call uploads.  With the cache enabled the calling thread keeps whole-window device copies of these five
 * between calls -- keyed on their host addresses and every extent -- and uploads one again only after
 * amt_host_invalidate(ptr) (NULL: all of them; call it when a new RK stage has rewritten them, and when an
 * array was freed and another one allocated at the same address: the key is the address, not the contents).  Since r04
 * the 2-D and 1-D inputs that are constant over the sub-steps as well (mut, muu, muv, mu_tend, the four map factors, dnw,
 * fnm, fnp, rdnw) are kept the same way.  u, v, t, mu and level 1 of ww, which change from sub-step to sub-step, and all
 * outputs cross the link on every call as before (unless deferred, below).  The reference re-uploads everything on every call
 * (advance_mu_t_no_async.cu:245-306).
 * amt_host_cache_check(1) is the debug mode: every call checksums the cached arrays on the host and fails with
 * AMT_ERR_PRECONDITION if one changed without an invalidate (it reads the whole arrays: slow).
 * amt_host_cache_enable(0) and amt_host_release() free the copies. */
int amt_host_cache_enable(int on);
int amt_host_cache_check(int on);
int amt_host_invalidate(const void *host_ptr);

/* Deferred outputs of the one-shot calls (per calling host thread; off by default): the practical form of a resident
 * small-step loop at the reference's own boundary (every call of advance_mu_t_no_async.cu brings all outputs down,
 * :366-390, and takes them up again with the next call, :245-306).  amt_host_defer(ptr, 1) marks one of the routine's
 * outputs -- ww, t, t_ave, mu, muave, muts, mudf, recognised by its host address in the calls that follow; NULL: all
 * seven -- as DEFERRED: it stays on the device after a call (a whole-window copy, like the cached inputs) and nothing of it
 * is written to the host array; the in/out ones (level 1 of ww, t, mu) are then also not uploaded by the next call --
 * the device copy is the truth.  amt_host_fetch(ptr) (NULL: every stale one) brings the window's cells down when the
 * caller -- the next routine of the acoustic loop, or the end of the loop -- really needs host values; amt_host_stale(ptr)
 * (NULL: any) says whether the device copy is newer than the host array.  amt_host_invalidate(ptr) says the HOST array
 * was rewritten and is the truth again (the next call uploads it).  With the residency cache on as well, a sub-step
 * uploads u, v and the 2-D / 1-D inputs only.  amt_host_defer(ptr, 0) fetches what is stale and makes the array an
 * ordinary output again; so do amt_host_release() and a call with other extents or other arrays (nothing the device
 * alone holds is ever dropped by the library; a thread that ENDS without amt_host_release() loses it).
 * In the debug mode (amt_host_cache_check(1)) the window's cells of a deferred host array are overwritten with NaN
 * canaries after every call, so that a consumer reading the stale array computes NaNs instead of silently using old
 * values, and a call that finds them changed without an invalidate fails with AMT_ERR_PRECONDITION.
 * After a call that FAILS once its kernels were enqueued, the device copies of the deferred outputs are undefined (t, mu and
 * level 1 of ww are advanced in place, chunk by chunk): amt_host_stale then returns -1 for them, amt_host_fetch and the next
 * call fail with AMT_ERR_PRECONDITION, and amt_host_invalidate(ptr) -- the host array as last fetched is the truth -- clears it. */
int amt_host_defer(const void *host_ptr, int on);
int amt_host_fetch(const void *host_ptr);
int amt_host_stale(const void *host_ptr);

/* ------------------------------------------------------------------------
 * (2) Device-resident drop-ins: the same call with every array pointer in
 *     DEVICE memory of the current device, enqueued on `hip_stream`
 *     (a hipStream_t; NULL = the default stream) and returning without
 *     synchronising.  This is the kernel-only boundary the reference times
 *     (advance_mu_t_no_async.cu:324-363) and what a resident small-step loop
 *     (solve_em) or a j-slab owner calls per sub-step; a slab owner passes the
 *     GLOBAL ids..jde and its LOCAL jms..jme / jts..jte, exactly as a WRF patch
 *     does.  `variant` is an amt_variant.
 * ------------------------------------------------------------------------ */
int amt_advance_mu_t_device_f32(
    void *hip_stream, int variant,
    float *ww, const float *ww_1, const float *u, const float *u_1,
    const float *v, const float *v_1,
    float *mu, const float *mut, float *muave, float *muts,
    const float *muu, const float *muv,
    float *mudf, float *t, const float *t_1,
    float *t_ave, const float *ft, const float *mu_tend,
    float rdx, float rdy, float dts, float epssm,
    const float *dnw, const float *fnm, const float *fnp, const float *rdnw,
    const float *msfuy, const float *msfvx_inv,
    const float *msftx, const float *msfty,
    int periodic_x, int specified, int nested,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);

int amt_advance_mu_t_device_f64(
    void *hip_stream, int variant,
    double *ww, const double *ww_1, const double *u, const double *u_1,
    const double *v, const double *v_1,
    double *mu, const double *mut, double *muave, double *muts,
    const double *muu, const double *muv,
    double *mudf, double *t, const double *t_1,
    double *t_ave, const double *ft, const double *mu_tend,
    double rdx, double rdy, double dts, double epssm,
    const double *dnw, const double *fnm, const double *fnp, const double *rdnw,
    const double *msfuy, const double *msfvx_inv,
    const double *msftx, const double *msfty,
    int periodic_x, int specified, int nested,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);

/* Compute window the routine will update for the given flags and bounds
 * (module_small_step_em.f90:91-106).  Pure host arithmetic, no device needed. */
int amt_compute_window(int periodic_x, int specified, int nested,
                       int ids, int ide, int jds, int jde,
                       int its, int ite, int jts, int jte, int kts, int kte,
                       int *i_start, int *i_end, int *j_start, int *j_end,
                       int *k_start, int *k_end);

/* ------------------------------------------------------------------------
 * (3) Resident domain handle: owns the 26 device arrays of one patch
 *     (memory extents ims:ime, kms:kme, jms:jme), a compute stream and the four
 *     scalars.  For C / Fortran hosts that keep ww, t, mu on the GPU across
 *     sub-steps; dtype_bytes is 4 (float) or 8 (double).  Field ids are
 *     enum amt_field of amt_synth.h (the Fortran argument order).
 * ------------------------------------------------------------------------ */
typedef struct amt_domain amt_domain;

int amt_domain_create(amt_domain **out, int dtype_bytes,
                      int periodic_x, int specified, int nested,
                      int ids, int ide, int jds, int jde, int kde,
                      int ims, int ime, int jms, int jme, int kms, int kme,
                      int its, int ite, int jts, int jte, int kts, int kte);
/* The same handle over device arrays the CALLER owns (a host model that already keeps its state
 * on the GPU, as WRF's arrays would be): fields[f] is the device pointer of field f (enum
 * amt_field, all AMT_F_COUNT of them, laid out as above); hip_stream is the hipStream_t the
 * handle's work is enqueued on, NULL = a stream of its own.  Nothing is copied; destroy frees
 * neither the arrays nor the caller's stream.  Device pointers -- here, in amt_ensemble_wrap and in
 * every amt_*_device_* call -- need the alignment of their element type only (4 or 8 bytes): arrays
 * packed back to back in one allocation, at whatever offsets their sizes add up to, are served
 * (tests/test_gpu_17c_packed_state.py). */
int amt_domain_wrap(amt_domain **out, int dtype_bytes,
                    int periodic_x, int specified, int nested,
                    int ids, int ide, int jds, int jde, int kde,
                    int ims, int ime, int jms, int jme, int kms, int kme,
                    int its, int ite, int jts, int jte, int kts, int kte,
                    void *const *fields, void *hip_stream);
int amt_domain_destroy(amt_domain *d);
int amt_domain_set_scalars(amt_domain *d, double rdx, double rdy, double dts, double epssm);
int amt_domain_set_variant(amt_domain *d, int variant);
/* whole-array copies in the (ims:ime[,kms:kme][,jms:jme]) layout; synchronous */
int amt_domain_upload(amt_domain *d, int field, const void *host);
int amt_domain_download(amt_domain *d, int field, void *host);
/* rows j_lo..j_hi (Fortran indices inside jms:jme) of a rank-3 or rank-2 field; `host` holds
 * exactly those rows (contiguous in this layout); synchronous */
int amt_domain_upload_rows(amt_domain *d, int field, int j_lo, int j_hi, const void *host);
int amt_domain_download_rows(amt_domain *d, int field, int j_lo, int j_hi, void *host);
/* fill every field from amt_synth.h; (gi0,gk0,gj0) = GLOBAL zero-based index of this
 * patch's element (ims,kms,jms); (gidim,gkdim,gjdim) = GLOBAL memory extents */
int amt_domain_fill_synthetic(amt_domain *d, uint64_t seed,
                              long gi0, long gk0, long gj0,
                              long gidim, long gkdim, long gjdim);
/* The same for the fields whose bit is set in field_mask (bit f = enum amt_field f) only; asynchronous on the domain's
 * stream.  With AMT_EXCHANGED_FIELDS and a seed that changes per sub-step this stands in for WRF's advance_uv, which
 * rewrites u and v before every advance_mu_t call (the operands of module_small_step_em.f90:143-146, :241-245): the rows
 * and columns a patch sends then differ from sweep to sweep, and only an exchange that delivers EVERY sweep gives the
 * bits of the unsplit run.  (AMT_EXCHANGED_FIELDS names enum amt_field: include amt_synth.h where it is expanded.) */
#define AMT_FIELD_BIT(f) (1ull << (f))
#define AMT_EXCHANGED_FIELDS                                                                                   \
    (AMT_FIELD_BIT(AMT_F_U) | AMT_FIELD_BIT(AMT_F_U_1) | AMT_FIELD_BIT(AMT_F_V) | AMT_FIELD_BIT(AMT_F_V_1) |   \
     AMT_FIELD_BIT(AMT_F_T_1) | AMT_FIELD_BIT(AMT_F_MUU) | AMT_FIELD_BIT(AMT_F_MUV) | AMT_FIELD_BIT(AMT_F_MSFUY) | \
     AMT_FIELD_BIT(AMT_F_MSFVX_INV))
int amt_domain_fill_fields(amt_domain *d, uint64_t field_mask, uint64_t seed,
                           long gi0, long gk0, long gj0,
                           long gidim, long gkdim, long gjdim);
/* Verification aid: overwrite with NaN exactly what the stencil reads from a neighbour on the given sides -- row jte+1 of
 * v, v_1, t_1, muv, msfvx_inv (AMT_SIDE_ABOVE), row jts-1 of t_1 (AMT_SIDE_BELOW), column ite+1 of u, u_1, t_1, muu, msfuy
 * (AMT_SIDE_RIGHT), column its-1 of t_1 (AMT_SIDE_LEFT); asynchronous on the domain's stream.  A sweep whose exchange
 * does not deliver then computes NaN in its boundary cells. */
enum amt_sides { AMT_SIDE_BELOW = 1, AMT_SIDE_ABOVE = 2, AMT_SIDE_LEFT = 4, AMT_SIDE_RIGHT = 8 };
int amt_domain_poison_halos(amt_domain *d, int sides);
/* enqueue n_sweeps calls of advance_mu_t over the patch's tile; asynchronous */
int amt_domain_step(amt_domain *d, int n_sweeps);
/* same, bracketed by HIP events on the domain's stream; returns after completion */
int amt_domain_step_timed(amt_domain *d, int n_sweeps, float *ms_total);
/* Placement tuning (speed only; +-3 % of a sweep hang on which physical pages the driver hands out):
 * allocates the handle's 26 arrays `tries` times, one set after the other (needs room for a second copy of the state;
 * stops early when there is none), copies the current contents over, times two sweeps of the handle's own kernel on each
 * set and keeps the fastest; every array holds afterwards what it held before the call.  ms_per_try (tries floats, or
 * NULL) receives the sweep time of each set (0 for sets that were not tried).  Device pointers obtained from
 * amt_domain_field_ptr before the call are no longer valid.  Not for wrapped domains (amt_domain_wrap). */
int amt_domain_tune_placement(amt_domain *domain, int tries, float *ms_per_try);
/* amt_domain_create does the same sampling by itself for states of 256 MiB and more (AMT_DOMAIN_PLACEMENT_TRIES allocations, default
 * 4; 0 or 1 = the first allocation as it comes; skipped where a second copy of the state does not fit): a host that creates its
 * handle once gets the sweep time bench.py prints.  COST, paid once at creation: up to TWICE the state plus a spacer of up to
 * 4 GiB resident for a moment, and 3 sweeps per allocation, timed with the AUTO kernel on the arrays as allocated (before
 * amt_domain_set_variant / the first upload: the placement of pages does not depend on either).  One process samples per device
 * at a time (advisory lock /tmp/amt_placement_<pci address>.lock); it is skipped altogether when the ranks of the launch
 * outnumber the visible devices (LOCAL_WORLD_SIZE, else WORLD_SIZE, > device count: ranks that share a device would sample beside
 * each other's sweeps and could starve each other's allocations).  Returns the number of allocations timed by the last sampling of this handle
 * (0: none) and their sweep times (ms; 0 for sets that were not tried). */
int amt_domain_placement(const amt_domain *domain, float *ms_per_try, int cap);
int amt_domain_sync(amt_domain *d);
void *amt_domain_field_ptr(amt_domain *d, int field);   /* device pointer, NULL on error */
void *amt_domain_stream(amt_domain *d);                 /* hipStream_t */

/* ------------------------------------------------------------------------
 * (4) Synthetic inputs (amt_synth.h) for a patch of extents idim x kdim x jdim
 *     whose element (0,0,0) is GLOBAL (gi0,gk0,gj0).  Rank-2 fields ignore the k
 *     arguments, rank-1 fields the i and j arguments.  The host and the device
 *     version produce identical bits.
 * ------------------------------------------------------------------------ */
int amt_synth_fill_host(int field, int dtype_bytes, void *dst, uint64_t seed,
                        long idim, long kdim, long jdim,
                        long gi0, long gk0, long gj0,
                        long gidim, long gkdim, long gjdim);
int amt_synth_fill_device(void *hip_stream, int field, int dtype_bytes, void *dst_device,
                          uint64_t seed,
                          long idim, long kdim, long jdim,
                          long gi0, long gk0, long gj0,
                          long gidim, long gkdim, long gjdim);

/* ------------------------------------------------------------------------
 * (5) j-slabs over several GPUs, one process per GPU: each rank owns rows jts..jte of the
 *     domain in a resident handle whose memory holds exactly one more row on either side
 *     (GLOBAL ids..jde, LOCAL jms = jts-1, jme = jte+1), as a WRF patch does.  Before a
 *     boundary row is computed the rank receives from the rank above row jte+1 of v, v_1, t_1,
 *     muv, msfvx_inv (module_small_step_em.f90:143-144,241) and from the rank below row jts-1
 *     of t_1 (:242): RCCL send/recv in one group on a communication stream, on which the two
 *     boundary rows then run, while the interior rows compute on the domain's stream.  Outputs
 *     need no exchange.  The reference splits j over its GPUs inside one process and refills
 *     the halos from the host on every call (advance_mu_t_no_async.cu:108-162).
 *     Two transports carry the rows.  RCCL (the default; loaded on first use with dlopen, AMT_RCCL_LIBRARY overrides the
 *     name): xGMI between the GPUs of a node; it needs one device per rank.  IPC (AMT_SLAB_TRANSPORT_IPC, or
 *     AMT_SLAB_TRANSPORT=ipc in the environment of a host that cannot pass the flag): no RCCL at all -- at creation the
 *     ranks trade hipIpcMemHandles of small staging buffers (copies of their boundary rows, refreshed by a kernel per sweep: the
 *     caller's arrays may be of any size and from any allocator) through a POSIX shared-memory block named after the unique id;
 *     per sweep the receiver waits for its neighbour's "rows final" number in that block (a one-wave kernel), pulls the rows
 *     with the copy engine (hipMemcpyAsync from the peer mapping: SDMA over xGMI between GPUs, no compute unit held while
 *     the wire is busy -- RCCL's send/recv kernel holds 31) and posts "pulled"; a rank's sweep ends when its neighbours have
 *     pulled its rows.  The ranks must be processes of one node; they may share ONE device (how the two-rank tests run on
 *     a one-GPU box).
 *     With overlap the IPC transport runs the HOST-WAITED schedule by default (AMT_IPC_HOST_WAIT=0: a waiting kernel instead): "rows
 *     final" is posted on the domain's stream in front of the interior, amt_slab_step waits on the calling host thread until the
 *     neighbours have posted theirs (so the call blocks for as long as a neighbour is behind -- per sub-step, like an MPI host),
 *     and the pull and the boundary rows run behind an interior that had the whole chip: nothing holds a compute unit while a
 *     neighbour is late (one rank of 8 in loopback: bare launch + 2.3 %, flat to 1.5 ms of lateness; profiles/r05_slab_ab.md).
 *     AMT_IPC_PULL=engine|kernel overrides how the rows are pulled (amt_slab_pull_mode; AMT_IPC_PULL_WGS: workgroups of the
 *     fused kernel, 4); AMT_IPC_TIMEOUT_S (120) bounds
 *     the host-side waits of the set-up, AMT_IPC_DEVICE_TIMEOUT_S (30) a device-side wait for a neighbour: it gives up,
 *     the sweep completes with invalid halo rows and amt_slab_sync returns AMT_ERR_COMM (nothing ever hangs the GPU).
 * ------------------------------------------------------------------------ */
#define AMT_UNIQUE_ID_BYTES 128              /* sizeof(ncclUniqueId) */
enum amt_slab_flags {
    AMT_SLAB_NO_OVERLAP = 1,                 /* exchange, then all rows, on one stream          */
    AMT_SLAB_LOOPBACK = 2,                   /* one-rank test mode: both neighbours are this rank */
    AMT_SLAB_TRANSPORT_IPC = 4,              /* peer copies between processes instead of RCCL     */
    /* Cyclic (periodic) domain, section (9): the decomposition is a torus in that direction.  With several ranks in it the edge
     * ranks are each other's neighbours and the wrap columns / rows travel as ordinary segments of the same exchange (both
     * transports, every schedule; counted by amt_*_halo_bytes); the edge ranks gather and scatter at their compute window's edge
     * (a last patch may end at ide-1 or at ide).  With ONE rank in it (a j-slab world with CYCLIC_X, a world of one) no transport
     * is involved: the refresh kernel of (9) runs on the domain's stream in front of every sweep.  Preconditions as in (9);
     * together with AMT_SLAB_LOOPBACK: AMT_ERR_INVALID_ARG. */
    AMT_SLAB_CYCLIC_X = 8,
    AMT_SLAB_CYCLIC_Y = 16,
    /* Section (11): the HOST moves the halos.  The library packs one contiguous message per side, the host carries the
     * messages with whatever it owns (MPI), the library unpacks.  unique_id may be NULL, creation is not collective, no RCCL
     * and no shared-memory block are involved, any number of such handles may live in one process and on one device; the
     * AMT_SLAB_TRANSPORT environment override does not apply.  Together with AMT_SLAB_LOOPBACK: AMT_ERR_INVALID_ARG.
     * AMT_SLAB_NO_OVERLAP and the cyclic flags work as with the other transports. */
    AMT_SLAB_TRANSPORT_EXTERNAL = 32,
    AMT_SLAB_EXTERNAL_HOST_BUFFERS = 64      /* with EXTERNAL: the messages lie in page-locked host memory */
};
typedef struct amt_slab amt_slab;

int amt_set_device(int device);              /* hipSetDevice for hosts without a HIP binding     */
/* rank 0: a fresh communicator id to hand to every rank: ncclGetUniqueId; where RCCL cannot be loaded, or with
 * AMT_SLAB_TRANSPORT=ipc in the environment, random bytes that name the launch for the IPC transport only */
int amt_comm_unique_id(void *id_out /* AMT_UNIQUE_ID_BYTES */);
/* The same through a file for hosts without MPI.  Rank 0 creates the id and publishes it as
 * `path` behind a header carrying `nonce`; every other rank waits (up to timeout_s) for a file
 * with ITS nonce, reads the id and acknowledges; rank 0 returns when all world-1 ranks have it and
 * removes the files.  `nonce` ties the file to one launch: a file left by another (crashed)
 * launch is never accepted, however fresh.  nonce = 0 means amt_comm_launch_nonce(). */
int amt_comm_rendezvous_file(const char *path, uint64_t nonce, int rank, int world,
                             double timeout_s, void *id_out);
/* a value all processes of one launch agree on and two launches do not: AMT_RENDEZVOUS_NONCE if
 * set, else the launcher (TORCHELASTIC_RUN_ID, parent pid + its start time) and MASTER_PORT */
uint64_t amt_comm_launch_nonce(void);
/* collective over the `world` ranks (ncclCommInitRank / the IPC set-up); the domain must outlive the slab */
int amt_slab_create(amt_slab **out, amt_domain *domain, int rank, int world,
                    const void *unique_id, int flags);
int amt_slab_destroy(amt_slab *slab);
int amt_slab_exchange(amt_slab *slab);       /* the halo exchange alone                           */
int amt_slab_step(amt_slab *slab, int n_sweeps);             /* asynchronous                      */
int amt_slab_step_timed(amt_slab *slab, int n_sweeps, float *ms_total);
int amt_slab_sync(amt_slab *slab);               /* AMT_ERR_COMM if a device-side wait for a neighbour gave up (IPC) */
const char *amt_slab_transport(const amt_slab *slab);        /* "rccl", "ipc", "external" (11), or "none" (no neighbour) */
/* how the IPC transport pulls: "copy engine" (between GPUs: hipMemcpyAsync per row) or "fused kernel" (ranks that share a device,
 * loopback: one kernel waits, pulls and posts -- a peer copy is a blit kernel there anyway); "" with RCCL */
const char *amt_slab_pull_mode(const amt_slab *slab);
/* Test hook: from now on every sweep's exchange starts `microseconds` late on the communication stream (a device-side
 * delay in front of the ncclSend/ncclRecv group), i.e. the neighbours' rows arrive that much late -- neighbour skew on
 * one GPU with the rank as its own neighbour (AMT_SLAB_LOOPBACK; profiles/slab_loopback.py --skew-us).  0 = off.  (The IPC
 * transport carries the delay inside its own waiting kernel: what waits is what would wait for a late neighbour.)
 * AMT_SLAB_SKEW_WGS=n in the environment gives the delay n workgroups that each hold a compute unit (31: what RCCL's
 * waiting send/recv kernel holds; default 1). */
int amt_slab_set_skew_us(amt_slab *slab, int microseconds);
long amt_slab_halo_bytes(const amt_slab *slab);              /* sent + received by this rank per sweep */
/* rank and size as the transport reports them: the communicator, or the ranks attached to the IPC block (0 of 1 without one) */
int amt_slab_comm_info(const amt_slab *slab, int *rank, int *world);
/* reporting aids for hosts without MPI: drain this rank's streams, then wait for every rank
 * (barrier) / replace *x by its maximum over the ranks.  The sweep itself has no collective. */
int amt_slab_barrier(amt_slab *slab);
int amt_slab_max(amt_slab *slab, double *x);

/* ------------------------------------------------------------------------
 * (5b) Patches in i AND j (domains whose j extent is too small for one slab per GPU): rank
 *      rj * pi + ri owns patch (ri, rj) of a pi x pj decomposition -- columns its..ite and rows jts..jte of the domain in a
 *      resident handle whose memory holds at least one more column and row on every side that has a neighbour (GLOBAL ids..jde,
 *      LOCAL ims <= its-1, ime >= ite+1, jms = jts-1, jme = jte+1).  Rows cross a boundary as in (5).  Across an i boundary the
 *      stencil reads column ite+1 of u, u_1, t_1, muu, msfuy (module_small_step_em.f90:145-146, :244) and column its-1 of t_1
 *      (:245): a column is kdim*jdim elements at stride idim, so one HIP kernel gathers the columns a patch sends into one
 *      contiguous buffer per direction, the buffers travel in the same exchange as the rows (same transports, same flags), and
 *      one kernel scatters what arrived into the halo columns.  No diagonal neighbours are needed.  Interior cells compute on
 *      the domain's stream beside the exchange; the boundary rows (over the patch's whole width: they own the corners) and the
 *      boundary columns (over the rows in between) follow it on the communication stream.  amt_slab_* is the pi = 1 case of the
 *      same stepper.  Flags are enum amt_slab_flags (AMT_SLAB_LOOPBACK: the rank is its own neighbour on all four sides).
 *      Cost on one patch (profiles/r05_grid_loopback.md): overlap +8 % at 2048 x 2048 columns, +20 % at 1024 x 1024 (three boundary
 *      launches per sweep); AMT_SLAB_NO_OVERLAP (halos, then ONE launch) +3 % and +7 % plus the neighbours' lateness.
 * ------------------------------------------------------------------------ */
typedef struct amt_grid amt_grid;
int amt_grid_create(amt_grid **out, amt_domain *domain, int ri, int rj, int pi, int pj,
                    const void *unique_id, int flags);               /* collective over the pi * pj ranks */
int amt_grid_destroy(amt_grid *grid);
int amt_grid_exchange(amt_grid *grid);                               /* pack, exchange, unpack alone      */
int amt_grid_step(amt_grid *grid, int n_sweeps);                     /* asynchronous                      */
int amt_grid_step_timed(amt_grid *grid, int n_sweeps, float *ms_total);
int amt_grid_sync(amt_grid *grid);
int amt_grid_set_skew_us(amt_grid *grid, int microseconds);          /* test hook, as amt_slab_set_skew_us */
long amt_grid_halo_bytes(const amt_grid *grid);                      /* sent + received by this rank per sweep */
const char *amt_grid_transport(const amt_grid *grid);
const char *amt_grid_pull_mode(const amt_grid *grid);
int amt_grid_comm_info(const amt_grid *grid, int *rank, int *world);
int amt_grid_barrier(amt_grid *grid);
int amt_grid_max(amt_grid *grid, double *x);

/* ------------------------------------------------------------------------
 * (6) Profiling aid: a plain streaming copy of nbytes (device to device) that moves
 *     bytes_per_lane = 4, 8 or 16 bytes per lane per access -- a KNOWN byte count in
 *     the kernels' own access width, used to calibrate rocprofv3's FETCH_SIZE /
 *     WRITE_SIZE on gfx950 (profiles/README.md).
 * ------------------------------------------------------------------------ */
int amt_calib_stream_copy(void *hip_stream, void *dst_device, const void *src_device,
                          size_t nbytes, int bytes_per_lane);
/* The box's own streaming ceilings, for attributing a measured sweep time to the machine or to the
 * kernel (bench.py: roofline.box_copy_GBps / box_read_GBps, measured in the same process): mode 0 copies
 * nbytes from src to dst (nbytes read + nbytes written), mode 1 only reads src (dst: 8 bytes that are never
 * written for finite data).  16 bytes per lane, tuned for gfx950; nbytes a multiple of 16.  Asynchronous:
 * time it with events on hip_stream. */
int amt_calib_stream_rate(void *hip_stream, void *dst_device, const void *src_device,
                          size_t nbytes, int mode);

/* ------------------------------------------------------------------------
 * (7) Tuning and test hooks of AMT_VARIANT_MARCH: force the wave shape
 *     (columns per lane, levels per lane, level groups per wave, extra DMA'd inputs, DMA or
 *     register flavour, rows per workgroup, 16- or 11-wave build; 0 / -1 = leave it to the launcher) for every later
 *     call of the process -- a shape that cannot run the given level count makes the call fail
 *     (AMT_VARIANT_AUTO then falls back to the column kernel).  amt_march_last_kernel names the
 *     kernel the calling thread's last launch plan chose (the column kernel included); amt_march_selectable lists the ones the
 *     launcher can choose unforced, one per line (returns the bytes needed).
 * ------------------------------------------------------------------------ */
int amt_march_force_shape(int vw, int kpt, int hl, int xd, int dma, int jrows, int max_waves);
const char *amt_march_last_kernel(void);
int amt_march_selectable(char *buf, int cap);
/* Rows per workgroup the launcher gives `ntile_i` column tiles of `nj` rows on `cus` compute units when a block's
 * unsigned 32-bit row offsets span at most `max_rows` rows, for a shape of `wbytes`-byte elements with `hl` level groups
 * per wave: the r <= max_rows that minimises rounds(r) * (r + 0.5), at most 64 for the fp64 shapes with level groups
 * (DESIGN.md section 4.2 "Launch plan", profiles/r04_rows.md).  Host arithmetic only; 0 when there is nothing to plan (no tile, row or CU). */
int amt_march_rows_for(long ntile_i, int nj, int cus, long max_rows, int wbytes, int hl);
/* Diagnosis: how workgroup numbers map to blocks.  0 (default): each XCD owns one contiguous run of blocks for the
 * whole launch; n > 0: every 8 n consecutive workgroup numbers cover 8 n consecutive blocks, n per XCD.  Which is
 * faster depends on where the arrays lie (profiles/r04_rows.md): not a tuning default. */
int amt_march_set_xchunk(int n);
/* How a launch made BESIDE another stream's kernels is planned (AMT_LAUNCH_BESIDE_OTHERS; a j-slab's interior).  A march workgroup
 * takes a compute unit whole (all its LDS and registers), so the other stream's kernels -- the halo exchange, the edge rows -- start
 * only where a workgroup ends, and every unit they take pushes interior workgroups into one more round.  `rounds`: least number of
 * rounds of workgroups (more, shorter rounds: more places to start, and a shorter extra round; half a row of prologue per block);
 * `reserve_cus`: compute units every round is planned to leave free (the other stream's kernels then start at once and push
 * nothing).  0, 0 = the defaults (AMT_MARCH_BESIDE_ROUNDS / AMT_MARCH_BESIDE_RESERVE in the environment, else 2 and 0).
 * Measured: profiles/r05_slab_ab.md. */
int amt_march_set_beside(int rounds, int reserve_cus);
/* Cache policy of the three once-read streams t, ft, ww_1 (same bits either way): -1 (default) by the
 * row length -- non-temporal loads (kernel amt_march_kernel) where rows are whole 128-byte lines, plain loads (kernel
 * amt_march_kernel_cached) where they are not (WRF's own unpadded ims:ime: neighbouring tiles then share the edge line of those
 * streams, and nt would drop it from L2: +3.5 % HBM reads, profiles/r06_rows4098_nt.md); 0 = always plain, 1 = always non-temporal.
 * AMT_MARCH_NT in the environment sets the same at load time. */
int amt_march_set_stream_policy(int policy);

/* ------------------------------------------------------------------------
 * (8) Ensembles: `members` patches of ONE shape -- same 17 bounds, same three flags, same four scalars rdx, rdy, dts, epssm,
 *     same four 1-D metric arrays dnw, fnm, fnp, rdnw, different state -- advanced by ONE launch per sweep.  A patch of a few
 *     hundred columns on a side cannot fill the chip on its own (128 x 128 columns: 256 blocks of one row, no reuse of the
 *     j faces); 20-50 such members planned together can (measured: profiles/ensemble_notes.md).
 *     LAYOUT: every 3-D and 2-D array has one more, slowest, dimension:
 *       3-D: element (i,k,j,m) at ((m*jdim + (j-jms))*kdim + (k-kms))*idim + (i-ims)
 *       2-D: element (i,j,m)   at  (m*jdim + (j-jms))*idim + (i-ims)               m = 0 .. members-1, jdim = jme-jms+1
 *     i.e. Fortran u(ims:ime, kms:kme, jms:jme, 1:members), numpy / torch shape (members, jdim, kdim, idim) and
 *     (members, jdim, idim).  Each member keeps its own halo rows jms..jts-1, jte+1..jme; nothing is shared between members
 *     and nothing of one member is ever read for another.  Outputs outside each member's compute window keep the caller's
 *     contents, as for a single patch.  Every member gets the bits the single-patch call gives that member alone.
 *     NOT provided: pointer tables, members of different shapes or scalars, placement sampling, slabs / grids over an
 *     ensemble (amt_slab_*, amt_grid_*), and a one-shot HOST-array ensemble call.
 * ------------------------------------------------------------------------ */
/* The device-resident drop-in (2) for an ensemble: the array pointers are the bases of the member-stacked device arrays, the
 * 1-D arrays and the scalars are the shared ones.  Asynchronous on hip_stream; same preconditions and status codes as
 * amt_advance_mu_t_device_*; members < 1 is AMT_ERR_INVALID_ARG. */
int amt_advance_mu_t_ensemble_device_f32(
    void *hip_stream, int variant, int members,
    float *ww, const float *ww_1, const float *u, const float *u_1,
    const float *v, const float *v_1,
    float *mu, const float *mut, float *muave, float *muts,
    const float *muu, const float *muv,
    float *mudf, float *t, const float *t_1,
    float *t_ave, const float *ft, const float *mu_tend,
    float rdx, float rdy, float dts, float epssm,
    const float *dnw, const float *fnm, const float *fnp, const float *rdnw,
    const float *msfuy, const float *msfvx_inv,
    const float *msftx, const float *msfty,
    int periodic_x, int specified, int nested,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);

int amt_advance_mu_t_ensemble_device_f64(
    void *hip_stream, int variant, int members,
    double *ww, const double *ww_1, const double *u, const double *u_1,
    const double *v, const double *v_1,
    double *mu, const double *mut, double *muave, double *muts,
    const double *muu, const double *muv,
    double *mudf, double *t, const double *t_1,
    double *t_ave, const double *ft, const double *mu_tend,
    double rdx, double rdy, double dts, double epssm,
    const double *dnw, const double *fnm, const double *fnp, const double *rdnw,
    const double *msfuy, const double *msfvx_inv,
    const double *msftx, const double *msfty,
    int periodic_x, int specified, int nested,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);

/* Resident ensemble handle, the counterpart of amt_domain (3): owns (create) or adopts (wrap: fields[f] = base of the stacked
 * device array of field f, all AMT_F_COUNT of them; hip_stream NULL = a stream of its own; nothing is copied, destroy frees
 * nothing of the caller's) the member-stacked arrays, a stream and the scalars.  The four 1-D fields hold kdim elements. */
typedef struct amt_ensemble amt_ensemble;
int amt_ensemble_create(amt_ensemble **out, int members, int dtype_bytes,
                        int periodic_x, int specified, int nested,
                        int ids, int ide, int jds, int jde, int kde,
                        int ims, int ime, int jms, int jme, int kms, int kme,
                        int its, int ite, int jts, int jte, int kts, int kte);
int amt_ensemble_wrap(amt_ensemble **out, int members, int dtype_bytes,
                      int periodic_x, int specified, int nested,
                      int ids, int ide, int jds, int jde, int kde,
                      int ims, int ime, int jms, int jme, int kms, int kme,
                      int its, int ite, int jts, int jte, int kts, int kte,
                      void *const *fields, void *hip_stream);
int amt_ensemble_destroy(amt_ensemble *e);
int amt_ensemble_set_scalars(amt_ensemble *e, double rdx, double rdy, double dts, double epssm);
int amt_ensemble_set_variant(amt_ensemble *e, int variant);
int amt_ensemble_members(const amt_ensemble *e);                   /* 0 for NULL */
/* ONE member (0-based) of a field; `host` holds that member in the single-patch layout of (3): the member's halo rows
 * included, no other member touched.  A 1-D field is shared: `member` only has to name a member.  Synchronous. */
int amt_ensemble_upload_member(amt_ensemble *e, int field, int member, const void *host);
int amt_ensemble_download_member(amt_ensemble *e, int field, int member, void *host);
/* member m is filled as amt_domain_fill_synthetic(seed + m, ...) fills a single patch; asynchronous on the handle's stream */
int amt_ensemble_fill_synthetic(amt_ensemble *e, uint64_t seed,
                                long gi0, long gk0, long gj0,
                                long gidim, long gkdim, long gjdim);
int amt_ensemble_step(amt_ensemble *e, int n_sweeps);              /* n_sweeps launches, each over all members; asynchronous */
int amt_ensemble_step_timed(amt_ensemble *e, int n_sweeps, float *ms_total);
int amt_ensemble_sync(amt_ensemble *e);
void *amt_ensemble_field_ptr(amt_ensemble *e, int field);          /* base of the stacked device array, NULL on error */
void *amt_ensemble_stream(amt_ensemble *e);                        /* hipStream_t */
/* amt_march_rows_for for an ensemble: `members` x `ntile_i` tile columns of `nj` rows each in one launch; a block never
 * leaves its member (the result is at most nj) and `max_rows` bounds the 32-bit offsets of ONE block.  members = 1 gives
 * exactly amt_march_rows_for; 0 when there is nothing to plan.  amt_march_last_kernel of an ensemble launch ends in
 * "jrows=R members=M jblocks=B" (B row blocks per member). */
int amt_march_rows_for_members(long ntile_i, int members, int nj, int cus, long max_rows, int wbytes, int hl);

/* ------------------------------------------------------------------------
 * (9) Cyclic (periodic) lateral boundaries, refreshed on the device.  The routine reads one cell past its compute window
 *     (i_start..i_end, j_start..j_end of amt_compute_window): column i_end+1 of u, u_1, t_1, muu, msfuy and column i_start-1
 *     of t_1 (module_small_step_em.f90:145-146, :244-245), row j_end+1 of v, v_1, t_1, muv, msfvx_inv and row j_start-1 of t_1
 *     (:143-144, :241-242).  periodic_x only widens the loop bounds (:97-102); in WRF the periodic-boundary exchange fills
 *     those cells before every call.  For a patch that holds the whole period of a direction, these calls do:
 *       AMT_CYCLIC_X, period ide - ids: column ide receives column ids of u, u_1, t_1, muu, msfuy; column ids-1 receives
 *                     column ide-1 of t_1; rows j_start..j_end, every memory level kms..kme
 *       AMT_CYCLIC_Y, period jde - jds: row jde receives row jds of v, v_1, t_1, muv, msfvx_inv; row jds-1 receives row
 *                     jde-1 of t_1; columns i_start..i_end, every memory level
 *     Corner cells are not written (the routine reads no diagonals), nothing outside the named cells changes, and the
 *     elements move as bits (NaN payloads survive).  One launch does a whole refresh, for every member of an ensemble.
 *     AMT_ERR_PRECONDITION: cyclic x with a clipped i window (it needs periodic_x || !(specified || nested)); cyclic y with
 *     specified or nested; a window that does not span the period (the window decides, not ite / jte: a last patch may end at
 *     ide-1 or at ide); memory extents that do not hold the destination cells.  axes = 0 refreshes nothing.
 *     A domain split over ranks wraps through AMT_SLAB_CYCLIC_X / AMT_SLAB_CYCLIC_Y of (5) instead.
 * ------------------------------------------------------------------------ */
enum amt_cyclic_axes { AMT_CYCLIC_X = 1, AMT_CYCLIC_Y = 2 };
/* pointer level, for callers of amt_advance_mu_t_device_* (members = 1) or amt_advance_mu_t_ensemble_device_* who keep
 * their own arrays; asynchronous on hip_stream (NULL = the default stream).  Only the arrays of the chosen axes are touched
 * (x: u, u_1, t_1, muu, msfuy; y: v, v_1, t_1, muv, msfvx_inv); the others may be NULL. */
int amt_cyclic_fill_device_f32(
    void *hip_stream, int axes, int members,
    float *u, float *u_1, float *v, float *v_1, float *t_1,
    float *muu, float *muv, float *msfuy, float *msfvx_inv,
    int periodic_x, int specified, int nested,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);
int amt_cyclic_fill_device_f64(
    void *hip_stream, int axes, int members,
    double *u, double *u_1, double *v, double *v_1, double *t_1,
    double *muu, double *muv, double *msfuy, double *msfvx_inv,
    int periodic_x, int specified, int nested,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);
/* one refresh now; asynchronous on the handle's stream (wrapped handles: the caller's stream) */
int amt_domain_cyclic_fill(amt_domain *d, int axes);
/* 0 = off (the default); otherwise every sweep of amt_domain_step / amt_domain_step_timed is preceded by a refresh on the
 * same stream.  A combination the handle's flags and extents do not admit is refused here and changes nothing. */
int amt_domain_set_cyclic(amt_domain *d, int axes);
int amt_domain_cyclic(const amt_domain *d);                        /* the axes set; 0 for NULL */
/* the same for an ensemble: all members in one launch */
int amt_ensemble_cyclic_fill(amt_ensemble *e, int axes);
int amt_ensemble_set_cyclic(amt_ensemble *e, int axes);
int amt_ensemble_cyclic(const amt_ensemble *e);

/* ------------------------------------------------------------------------
 * (10) Looking at resident state without downloading it: statistics of a field, a bit comparison of two fields, and a guard
 *      that watches ww, t and mu for NaN / Inf while the handle steps.  Each is ONE read of the field on the device.
 *      BOX: Fortran-inclusive i0..i1, k0..k1, j0..j1 inside the memory extents ims:ime, kms:kme, jms:jme of a rank-3 field
 *      (rank 2: the k arguments are ignored); with `members` > 1 the arrays are member-stacked as in (8) and every member gets
 *      a record of its own over the same box.  Cells outside the box never influence a result (halo cells may hold NaN) and
 *      nothing outside the array is read.  OFFSETS are element offsets from the MEMBER's base in the layout of (3).
 *      DETERMINISM: a member's record is a function of that member's box contents and the box shape alone -- not of the
 *      address, the stream, the run, or of what is stacked beside it (fixed partition, partials folded in index order, no
 *      floating-point atomics): `sum` has the same bits every time.
 *      Argument errors (a box outside the extents or empty, rank not 2 or 3, members < 1, a NULL pointer, a rank-1 field, an
 *      unknown region) are AMT_ERR_INVALID_ARG and are reported before any device call; `out` is then untouched.
 * ------------------------------------------------------------------------ */
typedef struct amt_field_stats {
    int64_t count;            /* elements in the box */
    int64_t n_nan, n_inf;
    int64_t first_nonfinite;  /* smallest element offset from the MEMBER's base of a NaN/Inf in the box, -1: none */
    double  min, max, max_abs;/* over the finite elements; +inf, -inf, 0 when there is none */
    double  sum;              /* of the finite elements, each converted to double exactly, added in double */
} amt_field_stats;

typedef struct amt_field_diff {
    int64_t count;
    int64_t n_diff;           /* elements whose BIT PATTERNS differ (-0.0 vs +0.0 differs; equal NaN payloads do not) */
    int64_t first_diff;       /* smallest offset from the member's base, -1: none */
    double  max_abs_diff;     /* max |a-b| over pairs with both finite, in double; 0 when there is none */
} amt_field_diff;

typedef struct amt_guard_report {
    int64_t sweeps_checked;   /* sweeps after which the guard looked, since it was armed */
    int64_t sweep;            /* sweep of the first finding, 1-based since arming; 0 = none (the fields below are then 0) */
    int32_t field;            /* enum amt_field: AMT_F_WW, AMT_F_T or AMT_F_MU */
    int32_t member;           /* 0 for a domain */
    int64_t offset;           /* of the first non-finite element, from the member's base */
    int64_t n_nonfinite;      /* NaN + Inf of that field and member at that sweep */
} amt_guard_report;

/* pointer level, beside amt_advance_mu_t_device_*: enqueued on hip_stream (NULL = the default stream), waits for that stream
 * and fills out[0 .. members-1] in HOST memory.  The workspace is kept per calling host thread. */
int amt_stats_device_f32(void *hip_stream, const float *a, int rank, int members,
                         int ims, int ime, int jms, int jme, int kms, int kme,
                         int i0, int i1, int k0, int k1, int j0, int j1, amt_field_stats *out);
int amt_stats_device_f64(void *hip_stream, const double *a, int rank, int members,
                         int ims, int ime, int jms, int jme, int kms, int kme,
                         int i0, int i1, int k0, int k1, int j0, int j1, amt_field_stats *out);
int amt_compare_device_f32(void *hip_stream, const float *a, const float *b, int rank, int members,
                           int ims, int ime, int jms, int jme, int kms, int kme,
                           int i0, int i1, int k0, int k1, int j0, int j1, amt_field_diff *out);
int amt_compare_device_f64(void *hip_stream, const double *a, const double *b, int rank, int members,
                           int ims, int ime, int jms, int jme, int kms, int kme,
                           int i0, int i1, int k0, int k1, int j0, int j1, amt_field_diff *out);

/* handle level.  AMT_REGION_WINDOW: i_start..i_end, j_start..j_end of amt_compute_window, levels k_start..k_end for a rank-3
 * field; AMT_REGION_MEMORY: the whole extents.  Synchronous: the work runs on the handle's stream behind whatever is enqueued
 * there.  The compare calls take two handles of the same dtype, bounds and member count on one device; the work is enqueued
 * on a's stream after b's stream has been waited for.  An ensemble fills `members` records. */
enum amt_region { AMT_REGION_WINDOW = 0, AMT_REGION_MEMORY = 1 };
int amt_domain_field_stats(amt_domain *d, int field, int region, amt_field_stats *out);
int amt_ensemble_field_stats(amt_ensemble *e, int field, int region, amt_field_stats *out);
int amt_domain_compare(amt_domain *a, amt_domain *b, int field, int region, amt_field_diff *out);
int amt_ensemble_compare(amt_ensemble *a, amt_ensemble *b, int field, int region, amt_field_diff *out);

/* Non-finite guard.  every = 0: off (the default; the step path enqueues exactly what it does without this section) and
 * any finding is cleared.  every = n >= 1: armed, any finding cleared; after every n-th sweep enqueued by *_step /
 * *_step_timed since arming, one statistics launch each for ww, t and mu over AMT_REGION_WINDOW runs on the handle's stream
 * (wrapped handles: the caller's), with no host wait and no allocation.  The FIRST finding -- earliest checked sweep, then
 * lowest member, then ww before t before mu, then smallest offset -- is sticky: the kernel writes it into a page-locked
 * host record.  With a finding present *_sync and *_step_timed return AMT_ERR_NONFINITE; *_step returns it WITHOUT enqueuing
 * anything when the finding is already visible at the call (it never waits); amt_last_error() names the sweep, the field,
 * the member and (i,k,j).  *_guard_report waits for the stream and fills the record (all zero with the guard off). */
int amt_domain_set_guard(amt_domain *d, int every);
int amt_ensemble_set_guard(amt_ensemble *e, int every);
int amt_domain_guard_report(amt_domain *d, amt_guard_report *out);
int amt_ensemble_guard_report(amt_ensemble *e, amt_guard_report *out);

/* ------------------------------------------------------------------------
 * (11) Host-owned halo exchange (AMT_SLAB_TRANSPORT_EXTERNAL of (5)): for a host that has its own communicator and halo
 *      layer (MPI, GPU-aware or not).  The library does not link or detect MPI.  Per side that has a neighbour the handle
 *      owns ONE send and ONE receive buffer (base 256-byte aligned; device memory, or page-locked host memory with
 *      AMT_SLAB_EXTERNAL_HOST_BUFFERS); one kernel launch packs all sends, one unpacks all receives.
 *      CONTENT, fixed: a peer that is not this library can produce it.  ilo..ihi, jlo..jhi: the patch's first / last column
 *      and row -- its..ite, jts..jte, in a cyclic direction the compute window's edges (a last patch may end at ide-1 or at
 *      ide); ni = ihi-ilo+1, nj = jhi-jlo+1; levels are every memory level kms..kme; elements travel as bits.
 *        send towards BELOW = the neighbour's recv from ABOVE: row jlo of v, v_1, t_1 (each: i fastest over ilo..ihi, then
 *                             k), then row jlo of muv, msfvx_inv (i over ilo..ihi)                   (3 kdim + 2) ni elements
 *        send towards ABOVE = recv from BELOW:                 row jhi of t_1                                  kdim ni
 *        send towards LEFT  = recv from RIGHT: column ilo of u, u_1, t_1 (each: k fastest, then j over jlo..jhi), then
 *                             column ilo of muu, msfuy (j over jlo..jhi)                             (3 kdim + 2) nj
 *        send towards RIGHT = recv from LEFT:                  column ihi of t_1                               kdim nj
 *      Received data lands in row jhi+1 / jlo-1 and column ihi+1 / ilo-1, columns ilo..ihi / rows jlo..jhi only: the cells
 *      outside (the corners) are never written -- the stencil reads no diagonal.  send_bytes of a rank towards a side equals
 *      recv_bytes of its neighbour from the opposite side.
 *      SWEEP: amt_grid_step_begin -> [amt_grid_halo_wait] -> amt_grid_step_end; any other order (end without begin, begin
 *      twice, a second wait, pack / unpack inside an open sweep) is AMT_ERR_INVALID_ARG before any device call, and so are
 *      amt_grid_step, _step_timed, _exchange, _max and _barrier on such a handle.
 *        begin  (asynchronous) on the domain's stream: the self-wrap refresh of a cyclic direction with one rank, the pack,
 *               the event "packed", then the interior cells (planned on their own: the whole chip).
 *        wait   (host) returns when "packed" of this sweep has happened -- the send buffers are readable -- and the unpack
 *               of the previous sweep has run -- the receive buffers are writable.  The interior keeps running meanwhile.
 *        end    (asynchronous) on the communication stream behind "packed": the unpack, the boundary rows and columns, the
 *               join into the domain's stream.
 *      With AMT_SLAB_NO_OVERLAP begin is refresh, pack, "packed"; end is the unpack and the whole patch as one launch on the
 *      domain's stream.  A patch without any neighbour: begin is the plain launch, wait and end enqueue nothing, no message.
 *      CONTRACT: the host completes its sends and its receives of sweep n between amt_grid_halo_wait and amt_grid_step_end
 *      of sweep n (with a stream-ordered transport it may skip the wait and order its copies itself).
 *      amt_grid_halo_pack / _unpack are the two halves of amt_grid_exchange without any compute, both asynchronous on the
 *      domain's stream: pack, amt_grid_sync, move the messages, unpack.
 * ------------------------------------------------------------------------ */
typedef struct amt_halo_message {
    int side;            /* AMT_SIDE_BELOW / ABOVE / LEFT / RIGHT (enum amt_sides) */
    int peer;            /* rank rj*pi+ri of the neighbour; with two ranks in a cyclic direction two sides name one peer: tag by side */
    void *send;  size_t send_bytes;
    void *recv;  size_t recv_bytes;
    int on_host;         /* 1: page-locked host memory (AMT_SLAB_EXTERNAL_HOST_BUFFERS) */
} amt_halo_message;
/* the messages of a handle, in the order BELOW, ABOVE, LEFT, RIGHT; *n = their number (0..4), also when it exceeds cap
 * (then AMT_ERR_INVALID_ARG and nothing is written); out may be NULL with cap = 0 */
int amt_grid_halo_messages(amt_grid *grid, amt_halo_message *out, int cap, int *n);
int amt_slab_halo_messages(amt_slab *slab, amt_halo_message *out, int cap, int *n);
/* The same list from the shape alone -- host arithmetic, no device, no handle: side, peer, send_bytes, recv_bytes; the
 * pointers are NULL.  flags: enum amt_slab_flags (EXTERNAL is implied); the precondition errors are those of creation. */
int amt_halo_plan(int dtype_bytes, int periodic_x, int specified, int nested,
                  int ids, int ide, int jds, int jde, int kde,
                  int ims, int ime, int jms, int jme, int kms, int kme,
                  int its, int ite, int jts, int jte, int kts, int kte,
                  int ri, int rj, int pi, int pj, int flags,
                  amt_halo_message *out, int cap, int *n);
int amt_grid_step_begin(amt_grid *grid);     /* asynchronous */
int amt_grid_halo_wait(amt_grid *grid);      /* host wait: send buffers readable AND recv buffers writable */
int amt_grid_step_end(amt_grid *grid);       /* asynchronous; the host's receives of this sweep are complete */
int amt_grid_halo_pack(amt_grid *grid);
int amt_grid_halo_unpack(amt_grid *grid);
int amt_slab_step_begin(amt_slab *slab);
int amt_slab_halo_wait(amt_slab *slab);
int amt_slab_step_end(amt_slab *slab);
int amt_slab_halo_pack(amt_slab *slab);
int amt_slab_halo_unpack(amt_slab *slab);

/* ------------------------------------------------------------------------
 * (12) Specified and nested lateral boundaries: the boundary-zone update on the device.  With `specified` or `nested` the
 *      routine clips its compute window by one cell at every domain edge (module_small_step_em.f90:97-106; with periodic_x
 *      in j only) and leaves t, mu and muts of that ring as the caller passed them.  In WRF's acoustic loop the ring is not
 *      constant: after every advance_mu_t call three spec_bdyupdate calls of zone width 1 advance it with the boundary
 *      tendencies.  These calls do the same.  With ihi = min(ite, ide-1), jhi = min(jte, jde-1), the BOUNDARY ZONE of a tile
 *      is every cell (i, j), its <= i <= ihi, jts <= j <= jhi, that is not in the window of amt_compute_window; in it, each
 *      cell exactly once,
 *        t(i,k,j)  = t(i,k,j)  + dts * ft(i,k,j)        k = kts .. kte-1
 *        mu(i,j)   = mu(i,j)   + dts * mu_tend(i,j)
 *        muts(i,j) = muts(i,j) + dts * mu_tend(i,j)
 *      each assignment two roundings in the arrays' type (product, then sum; no fused multiply-add; for fp32 dts is rounded
 *      to float first, as the sweep does).  Bit-unchanged: everything outside the zone (NaN payloads included), level kte of
 *      t, the zone's cells of ww, t_ave, muave and mudf, every input.  The sweep neither reads nor writes the zone's cells of
 *      t, mu and muts (it reads t_1 across the edge), so the update commutes with it; it is enqueued behind it, where WRF has it.
 *      periodic_x with specified: rows only, over the tile's whole width.  A tile that touches no domain edge: nothing to
 *      do, AMT_OK, nothing enqueued.  A corner tile: the corner cell belongs to the row strip and is updated once.  A domain
 *      so small that the window is empty (ide-ids < 3 or jde-jds < 3): the whole tile.  One launch does a whole update, for
 *      every member of an ensemble.
 *      AMT_ERR_PRECONDITION: neither specified nor nested (no zone to own); a tile outside memory; more than 65535 members
 *      (one launch carries the member in a grid dimension).  AMT_ERR_INVALID_ARG:
 *      members < 1, a NULL array.  All are reported before any device call, with or without a device.
 *      NOT provided: the one-shot host-array calls of (1).  A host that owns the arrays owns the ring as well and does its
 *      own boundary update.
 * ------------------------------------------------------------------------ */
/* pointer level, beside amt_advance_mu_t_device_* (members = 1) or amt_advance_mu_t_ensemble_device_* (member-stacked
 * arrays); asynchronous on hip_stream (NULL = the default stream) */
int amt_spec_bdy_update_device_f32(
    void *hip_stream, int members,
    float *t, const float *ft, float *mu, float *muts, const float *mu_tend, float dts,
    int periodic_x, int specified, int nested,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);
int amt_spec_bdy_update_device_f64(
    void *hip_stream, int members,
    double *t, const double *ft, double *mu, double *muts, const double *mu_tend, double dts,
    int periodic_x, int specified, int nested,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);
/* one update now, with the handle's dts (amt_domain_set_scalars); asynchronous on the handle's stream (wrapped handles: the
 * caller's stream) */
int amt_domain_spec_bdy_update(amt_domain *d);
/* on = 0: off (the default; the step paths enqueue exactly what they do without this section).  Otherwise every sweep of
 * amt_domain_step / amt_domain_step_timed is followed by one update on the same stream.  A handle keeps the setting under
 * amt_slab_* and amt_grid_*: every sweep of amt_slab_step / amt_grid_step / *_step_timed and of amt_slab_step_end /
 * amt_grid_step_end (a patch without a neighbour included) is followed by the update of that rank's own tile, on the domain's
 * stream where the sweep's work has joined it -- every schedule, AMT_SLAB_NO_OVERLAP included.  Nothing is exchanged for it
 * (the zone holds outputs only) and a rank whose patch touches no domain edge enqueues nothing.  A combination the handle
 * does not admit is refused here and changes nothing. */
int amt_domain_set_spec_bdy(amt_domain *d, int on);
int amt_domain_spec_bdy(const amt_domain *d);                      /* the setting; 0 for NULL */
/* the same for an ensemble: all members in one launch */
int amt_ensemble_spec_bdy_update(amt_ensemble *e);
int amt_ensemble_set_spec_bdy(amt_ensemble *e, int on);
int amt_ensemble_spec_bdy(const amt_ensemble *e);

/* ------------------------------------------------------------------------
 * (13) Ensemble mean, variance and envelope of a member-stacked field, on the device: what an ensemble host asks at every
 *      output time, without downloading `members` x the field.  INPUT: a BOX exactly as in (10) -- Fortran-inclusive i0..i1,
 *      k0..k1, j0..j1 inside the extents ims:ime, kms:kme, jms:jme of a rank-3 or rank-2 field (rank 2 ignores k) -- of the
 *      array `a`, member-stacked as in (8) with members = M >= 1: member m's base is a + m * idim*kdim*jdim (kdim = 1 for
 *      rank 2).  OUTPUTS: mean, var, lo, hi, each an array of ONE member's extents and of a's type, each may be NULL ("not
 *      wanted"), at least one must be given.  For every cell c of the box, in member order, with x_m = a_m[c]:
 *        mean  s = double(x_0); for m = 1..M-1: s = s + double(x_m);  mean_d = s / double(M);  mean[c] = T(mean_d), rounded
 *              to nearest even.  With M = 1 the mean is x_0 itself, -0.0 included.
 *        var   q = 0.0; for m = 0..M-1: d = double(x_m) - mean_d; q = q + d*d;  var_d = q / double(max(M-1, 1));
 *              var[c] = T(var_d): the unbiased sample variance; a single finite member gives +0.0.  d*d is a product, then a
 *              sum (no fused multiply-add).  There is no square root here: the caller takes it.
 *        lo    a NaN if any x_m is NaN (its payload is not part of the contract); otherwise the FIRST member, in member
 *              order, that attains the minimum: lo = x_0; if (x_m < lo) lo = x_m -- so the sign of a zero is that member's.
 *        hi    the same with >.
 *      +-Inf follow IEEE through these expressions (+Inf and -Inf in one cell: a NaN mean).  Every cell outside the box, in
 *      every output array, keeps its bits; no cell of `a` outside the box is read (halo cells may hold NaN), nothing outside
 *      the arrays is read or written.  The order is per cell and sequential over the members: a result is a function of the
 *      box contents alone -- not of addresses, alignment, stream, run or launch geometry (no atomics, no workspace).
 *      AMT_ERR_INVALID_ARG, reported before any device call, with or without a device, the outputs untouched: a NULL `a`;
 *      all four outputs NULL; members < 1; a rank that is not 2 or 3 (a rank-1 field at handle level); an unknown region;
 *      a box that is empty or outside the extents; an output whose address range (one member's extents) overlaps a's
 *      (members x that) or another output's.
 * ------------------------------------------------------------------------ */
/* pointer level, beside amt_stats_device_*: asynchronous on hip_stream (NULL = the default stream); writes DEVICE arrays,
 * needs no workspace and allocates nothing */
int amt_moments_device_f32(void *hip_stream, const float *a, int rank, int members,
                           int ims, int ime, int jms, int jme, int kms, int kme,
                           int i0, int i1, int k0, int k1, int j0, int j1,
                           float *mean, float *var, float *lo, float *hi);
int amt_moments_device_f64(void *hip_stream, const double *a, int rank, int members,
                           int ims, int ime, int jms, int jme, int kms, int kme,
                           int i0, int i1, int k0, int k1, int j0, int j1,
                           double *mean, double *var, double *lo, double *hi);
/* handle level: field `field` (rank 2 or 3, amt_field_rank) of the ensemble over AMT_REGION_WINDOW or AMT_REGION_MEMORY, with
 * the meaning amt_ensemble_field_stats gives them.  Asynchronous on the ensemble's stream (wrapped handles: the caller's),
 * behind whatever is enqueued there; amt_ensemble_sync waits for it.  The outputs are caller-owned device arrays of one
 * member's extents and the handle's type -- for instance amt_domain_field_ptr of an amt_domain of the same shape, which
 * amt_domain_field_stats, amt_domain_compare and amt_domain_download then understand. */
int amt_ensemble_moments(amt_ensemble *e, int field, int region, void *mean, void *var, void *lo, void *hi);

/* ------------------------------------------------------------------------
 * (14) The acoustic loop's flux averages ru_m, rv_m, ww_m (WRF's sumflux), on the device.  In solve_em every acoustic
 *      sub-step runs advance_mu_t, its three spec_bdyupdate calls (12) and then sumflux, which adds the sub-step's u, v and
 *      ww into three accumulators and, on the last sub-step, turns the sums into the time-averaged mass fluxes that scalar
 *      advection uses.  Every operand is one of the resident arrays (WRF passes ww1 = ww_1, u_save = u_1, v_save = v_1);
 *      only the accumulators are new: three arrays of a 3-D field's extents, member-stacked as in (8).
 *      Indices are Fortran-inclusive and global, on a tile its..ite, jts..jte with kts == 1 and kte == kde; T is the arrays'
 *      type, n = n_small_steps >= 1 and 1 <= iteration <= n.  Every operation is rounded once in T, there is no fused
 *      multiply-add, expressions associate left to right as written.  RANGES in which a field accumulates:
 *        ru_m  adds u    i = its..ite              k = kts..kte-1   j = jts..min(jte, jde-1)
 *        rv_m  adds v    i = its..min(ite, ide-1)  k = kts..kte-1   j = jts..jte
 *        ww_m  adds ww   i = its..min(ite, ide-1)  k = kts..kte     j = jts..min(jte, jde-1)
 *      For a cell of its field's range, x the added field's value there:
 *        s = (iteration == 1) ? T(0) + x : acc + x      at iteration 1 the old contents of acc are NOT read (they may be NaN);
 *                                                       T(0) + x makes -0.0 into +0.0, as the Fortran's zero-then-add does
 *        iteration <  n:  acc = s
 *        iteration == n:  q = s / T(n) (n converted to T, IEEE divide), and
 *                           ru_m = q + (muu(i,j) * u_1(i,k,j)) / msfuy(i,j)
 *                           rv_m = q + (muv(i,j) * v_1(i,k,j)) * msfvx_inv(i,j)
 *                           ww_m = q + ww_1(i,k,j)
 *      (n == 1 does both in the one call).  At iteration 1 every cell of the tile box its..ite, kts..kte, jts..jte OUTSIDE a
 *      field's range becomes +0.0 in that accumulator (WRF zeroes the whole tile); at any other iteration those cells keep
 *      their bits.  Always bit-unchanged, NaN payloads included: everything outside the tile box, every memory level outside
 *      kts..kte, every input.  No cell of an input outside the field's range is read (halos may hold NaN), nothing outside
 *      the arrays is touched.  The result is a function of the operands' contents alone -- not of addresses, alignment,
 *      stream or launch geometry (no atomics, no workspace).  Inputs may alias one another; an accumulator may not overlap
 *      any other array of the call.  One launch does a whole accumulation, for every member of an ensemble.
 *      Reported before any device call, with or without a device, the accumulators untouched:
 *      AMT_ERR_INVALID_ARG: a NULL array; members < 1; n < 1; iteration outside 1..n; an accumulator that overlaps another
 *      array.  AMT_ERR_PRECONDITION: the tile outside memory; kts != 1; kte != kde; kme < kte; more than 65535 members.
 *      NOT provided: the one-shot host-array calls of (1).  A host that owns the arrays accumulates on its own side.
 * ------------------------------------------------------------------------ */
/* pointer level, beside amt_advance_mu_t_device_* (members = 1) or amt_advance_mu_t_ensemble_device_*; asynchronous on
 * hip_stream (NULL = the default stream) */
int amt_sumflux_device_f32(
    void *hip_stream, int members, float *ru_m, float *rv_m, float *ww_m,
    const float *u, const float *v, const float *ww, const float *u_1, const float *v_1, const float *ww_1,
    const float *muu, const float *muv, const float *msfuy, const float *msfvx_inv,
    int iteration, int n_small_steps,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);
int amt_sumflux_device_f64(
    void *hip_stream, int members, double *ru_m, double *rv_m, double *ww_m,
    const double *u, const double *v, const double *ww, const double *u_1, const double *v_1, const double *ww_1,
    const double *muu, const double *muv, const double *msfuy, const double *msfvx_inv,
    int iteration, int n_small_steps,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);
/* n_small_steps = 0: off (the default; the step paths enqueue exactly what they do without this section) and what the
 * library allocated is freed.  n >= 1 with ru_m, rv_m, ww_m all NULL: the library allocates the three accumulators, each of
 * one 3-D field's extents (times the members of an ensemble); all three given: the caller's device arrays are used and never
 * freed; a mix is AMT_ERR_INVALID_ARG.  (The library's own three, as amt_domain_sumflux_ptr returns them, may be handed back to
 * set n anew: they stay the library's.)  The iteration counter is reset to 1.  Then every sweep of amt_domain_step /
 * amt_domain_step_timed is followed by one accumulation on the same stream, behind the boundary-zone update of (12) and in
 * front of the guard's checks of (10); the counter runs 1..n and wraps back to 1.  A handle keeps the setting under
 * amt_slab_* and amt_grid_*: the accumulation of that rank's own tile is enqueued where the boundary-zone update of (12) is,
 * in every schedule and in amt_*_step_end; nothing is exchanged for it.  amt_domain_tune_placement neither accumulates nor
 * advances the counter.  A refusal changes nothing. */
int amt_domain_set_sumflux(amt_domain *d, int n_small_steps, void *ru_m, void *rv_m, void *ww_m);
/* one accumulation now, as iteration `next_iteration`, asynchronous on the handle's stream; advances the counter */
int amt_domain_sumflux_accumulate(amt_domain *d);
int amt_domain_sumflux_state(const amt_domain *d, int *n, int *next_iteration);   /* n = 0: off; either may be NULL */
void *amt_domain_sumflux_ptr(amt_domain *d, int which);           /* 0 ru_m, 1 rv_m, 2 ww_m; NULL while off */
/* the same for an ensemble: all members in one launch, member-stacked accumulators */
int amt_ensemble_set_sumflux(amt_ensemble *e, int n_small_steps, void *ru_m, void *rv_m, void *ww_m);
int amt_ensemble_sumflux_accumulate(amt_ensemble *e);
int amt_ensemble_sumflux_state(const amt_ensemble *e, int *n, int *next_iteration);
void *amt_ensemble_sumflux_ptr(amt_ensemble *e, int which);

/* ------------------------------------------------------------------------
 * (15) The bracket of a Runge-Kutta stage: small_step_prep and small_step_finish, on the device.  In solve_em every
 *      Runge-Kutta stage opens its acoustic loop with small_step_prep, which turns the full fields into the perturbation form
 *      advance_mu_t works on, and closes it with small_step_finish, which turns them back.  With these two calls
 *      prep -> n x (sweep -> zone update (12) -> accumulation (14)) -> finish runs without a host round trip.  The reference has
 *      no source for the two routines: the definition below is this library's contract, modelled on WRF's routines and
 *      restricted to the arrays the library owns.  WRF's names: t = t_2, t_1 = t_save, ww_1 = ww1, mu = mu_2.  Arrays that
 *      are not AMT_F_* fields: t_old (3-D; WRF's t_1: theta at the time level the RK step starts from), mu_old (2-D; WRF's
 *      mu_1), mu_save (2-D), mub (2-D; base-state column mass, a pure input), h_diabatic (3-D; read by finish only, may be
 *      NULL); `members` >= 1 patches are member-stacked as in (8).
 *      Indices are Fortran-inclusive and global, on a tile its..ite, jts..jte with kts == 1 and kte == kde;
 *      ihi = min(ite, ide-1), jhi = min(jte, jde-1); T is the arrays' type.  Every operation is rounded once in T, there is
 *      no fused multiply-add, expressions associate exactly as written.  An assignment without arithmetic is a bit copy: NaN
 *      payloads, signalling NaNs and -0.0 are kept.
 *      PREP(rk_step), rk_step >= 1.  For every column i = its..ihi, j = jts..jhi, m = mu(i,j) as it was before the call:
 *        rk_step == 1:  mu_old = m;  muts = mub + m;  mu_save = m;  mu = m - m;  mudf = +0.0
 *                       (m - m is computed, not a stored zero: -0.0 gives +0.0, a NaN or +-Inf gives a NaN)
 *        rk_step  > 1:  muts = mub + mu_old;  mu_save = m;  mu = mu_old - m;  mudf is not touched and may be NULL
 *        cells k = kts..kte-1, x = t(i,k,j) before the call, s the NEW muts(i,j):
 *                       at rk_step == 1  t_old = x (its old contents are not read and may be NaN);
 *                       t_1 = x;  t = (s * t_old) - (mut * x)        two products, then one subtraction
 *        cells k = kts..kte:  ww_1 = ww
 *      FINISH(n, dts, h_diabatic), n = n_small_steps >= 1.  Over the same columns:
 *        cells k = kts..kte-1:  t = ((t - ((dts * T(n)) * mut) * h_diabatic) + (t_1 * mut)) / muts      with h_diabatic,
 *                               t = (t + (t_1 * mut)) / muts                                            without;
 *                               an IEEE divide; for fp32 dts is rounded to float first, as the sweep does
 *        cells k = kts..kte:    ww = ww + ww_1
 *        columns:               mu = mu + mu_save
 *      Always bit-unchanged, NaN payloads included: everything outside its..ihi x jts..jhi (column ide and row jde of a tile
 *      that reaches them too), level kte of t, t_1 and t_old, every memory level outside kts..kte, every input.  No input
 *      cell outside these ranges is read (halos may hold NaN), nothing outside the arrays is touched.  No atomics, no
 *      workspace: the result is a function of the operands' contents alone.  Inputs may alias one another; an output
 *      overlaps no other array of the call.  Prep is two launches in stream order (the 3-D pass reads the old mu, the 2-D
 *      pass overwrites it), finish is one.
 *      Reported before any device call, with or without a device, the arrays untouched:
 *      AMT_ERR_INVALID_ARG: a NULL array other than h_diabatic, and mudf at rk_step > 1; members < 1; rk_step < 1; n < 1; an
 *      output that overlaps another array.  AMT_ERR_PRECONDITION: the tile outside memory; kts != 1; kte != kde; kme < kte;
 *      more than 65535 members.
 *      NOT provided: the one-shot host-array calls of (1); u, v, w, ph and muus, muvs (they belong to advance_uv / advance_w);
 *      the cells of t_1 OUTSIDE the tile that the sweep reads at i+-1, j+-1 (a host fills them as it does today: the cyclic
 *      refresh (9), the steppers' halo exchange, which carries t_1, or its own boundary code); any coupling to the counter
 *      of (14).
 * ------------------------------------------------------------------------ */
/* pointer level; asynchronous on hip_stream (NULL = the default stream) */
int amt_stage_prep_device_f32(
    void *hip_stream, int members, float *t, float *t_1, float *t_old, const float *ww, float *ww_1,
    float *mu, float *mu_old, float *mu_save, float *muts, float *mudf, const float *mut, const float *mub, int rk_step,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);
int amt_stage_prep_device_f64(
    void *hip_stream, int members, double *t, double *t_1, double *t_old, const double *ww, double *ww_1,
    double *mu, double *mu_old, double *mu_save, double *muts, double *mudf, const double *mut, const double *mub, int rk_step,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);
int amt_stage_finish_device_f32(
    void *hip_stream, int members, float *t, const float *t_1, float *ww, const float *ww_1,
    float *mu, const float *mu_save, const float *muts, const float *mut, float dts, int n_small_steps, const float *h_diabatic,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);
int amt_stage_finish_device_f64(
    void *hip_stream, int members, double *t, const double *t_1, double *ww, const double *ww_1,
    double *mu, const double *mu_save, const double *muts, const double *mut, double dts, int n_small_steps, const double *h_diabatic,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);
/* on = 0: off (the default) and what the library allocated is freed; the handle's destroy frees it too.  on != 0 with t_old,
 * mu_old, mu_save, mub all NULL: the library allocates the four arrays (t_old of a 3-D field's extents, the others of a 2-D
 * field's, times the members of an ensemble; the host then fills mub once through amt_domain_stage_ptr); all four given: the
 * caller's device arrays are used and never freed; a mix is AMT_ERR_INVALID_ARG.  (The library's own four, as
 * amt_domain_stage_ptr returns them, may be handed back: nothing changes.)  A refusal changes nothing.  The setting is no
 * per-sweep setting: amt_domain_step and amt_domain_tune_placement enqueue what they do without it.  A handle keeps it under
 * amt_slab_* and amt_grid_*: prep and finish work on the rank's own tile, are issued on the domain handle between the stepper's
 * step calls and are ordered by the domain's stream; nothing is exchanged for them. */
int amt_domain_set_stage(amt_domain *d, int on, void *t_old, void *mu_old, void *mu_save, void *mub);
void *amt_domain_stage_ptr(amt_domain *d, int which);             /* 0 t_old, 1 mu_old, 2 mu_save, 3 mub; NULL while off */
/* prep in front of a stage's acoustic loop, finish (with the handle's dts; h_diabatic a caller-owned device array or NULL)
 * behind it: asynchronous on the handle's stream (the caller's for a wrapped handle); AMT_ERR_PRECONDITION while off */
int amt_domain_stage_prep(amt_domain *d, int rk_step);
int amt_domain_stage_finish(amt_domain *d, int n_small_steps, const void *h_diabatic);
/* the same for an ensemble: all members in one launch, member-stacked arrays */
int amt_ensemble_set_stage(amt_ensemble *e, int on, void *t_old, void *mu_old, void *mu_save, void *mub);
void *amt_ensemble_stage_ptr(amt_ensemble *e, int which);
int amt_ensemble_stage_prep(amt_ensemble *e, int rk_step);
int amt_ensemble_stage_finish(amt_ensemble *e, int n_small_steps, const void *h_diabatic);

/* ------------------------------------------------------------------------
 * (16) The pressure diagnosis that closes an acoustic sub-step: calc_p_rho, on the device.  In solve_em calc_p_rho follows
 *      small_step_prep (with step = 0) and every advance_mu_t of the acoustic loop (step != 0): from t, mu and muts it diagnoses
 *      the inverse density al and the pressure p that the next advance_uv reads, and in its hydrostatic branch integrates the
 *      geopotential ph up the column.  With it prep (15) -> calc_p_rho(0) -> n x (sweep -> zone update (12) -> accumulation (14)
 *      -> calc_p_rho) -> finish runs without a host round trip.  The reference has no source for the routine: the definition
 *      below is this library's contract, modelled on WRF's routine (without the hybrid coordinate's c1h, c2h) and restricted to
 *      the arrays the library owns.  WRF's names: t = t_2, t_old = t_1 (the array of (15)), mu = mu_2.  3-D arrays that are
 *      not AMT_F_* fields: al, p, pm1 (outputs), ph (on w levels kts..kte; an input in mode 1, an output above kts in mode 2),
 *      alt, c2a (pure inputs).  1-D arrays over kms..kme: rdnw (a handle uses its own metric), znu, dnw.  `members` >= 1
 *      patches are member-stacked as in (8); the 1-D arrays are shared by the members.
 *      Indices are Fortran-inclusive and global, on a tile its..ite, jts..jte with kts == 1 and kte == kde;
 *      ihi = min(ite, ide-1), jhi = min(jte, jde-1); columns i = its..ihi, j = jts..jhi, cells k = kts..kte-1; T is the arrays'
 *      type.  Every operation is rounded once in T, there is no fused multiply-add, divides are IEEE divides (no reciprocal
 *      approximation), expressions associate exactly as written; for fp32 t0 and smdiv are rounded to float first.
 *      Every cell computes   q = (alt * (t - (mu * t_old))) / (muts * (t0 + t_old))
 *      MODE 1, non-hydrostatic:  al = (T(-1) / muts) * ((alt * mu) + (rdnw(k) * (ph(k+1) - ph(k))))
 *                                p  = c2a * (q - al)                                            ph is not written
 *      MODE 2, hydrostatic, k ascending:
 *                                p  = mu * znu(k)
 *                                al = q - (p / c2a)
 *                                ph(k+1) = ph(k) - (dnw(k) * ((muts * al) + (mu * alt)))
 *                                ph(k) is the value just written for k > kts; ph(kts) is read and never written
 *      DIVERGENCE DAMPING, both modes, on the p just computed (x):
 *        step == 0:  p = x;  pm1 = x                       (the old pm1 is not read and may hold NaN)
 *        step != 0:  p = x + (smdiv * (x - pm1));  pm1 = x
 *        in mode 2 al and ph use the undamped x.
 *      Always bit-unchanged, NaN payloads included: everything outside the columns (column ide and row jde of a tile that
 *      reaches them too), level kte of al, p, pm1, every memory level outside kts..kte, every input.  No input cell outside
 *      the ranges is read (halos may hold NaN), nothing outside the arrays is touched.  No atomics, no workspace.  Inputs may
 *      alias one another; an output overlaps no other array of the call.  One launch.
 *      Reported before any device call, with or without a device, the arrays untouched:
 *      AMT_ERR_INVALID_ARG: a NULL array; members < 1; a mode other than 1 or 2; step < 0; an output that overlaps another
 *      array.  AMT_ERR_PRECONDITION: the tile outside memory; kts != 1; kte != kde; kme < kte; more than 65535 members.
 *      NOT provided: the one-shot host-array calls of (1); advance_uv and advance_w; WRF's hybrid-coordinate (c1h, c2h) form;
 *      filling or exchanging the halo cells of p, al, ph that advance_uv will read at i-1, j-1.
 * ------------------------------------------------------------------------ */
/* pointer level; asynchronous on hip_stream (NULL = the default stream) */
int amt_p_rho_device_f32(
    void *hip_stream, int members, int mode, int step, float *al, float *p, float *ph, float *pm1,
    const float *alt, const float *c2a, const float *t, const float *t_old, const float *mu, const float *muts,
    const float *rdnw, const float *znu, const float *dnw, float t0, float smdiv,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);
int amt_p_rho_device_f64(
    void *hip_stream, int members, int mode, int step, double *al, double *p, double *ph, double *pm1,
    const double *alt, const double *c2a, const double *t, const double *t_old, const double *mu, const double *muts,
    const double *rdnw, const double *znu, const double *dnw, double t0, double smdiv,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);
/* mode = 0: off (the default) and what the library allocated is freed; the handle's destroy frees it too.  mode = 1 or 2 with
 * al, p, ph, pm1, alt, c2a, znu, dnw all NULL: the library allocates the eight arrays (the six 3-D ones of a 3-D field's extents
 * times the members of an ensemble, znu and dnw of kme-kms+1 elements; the host then fills alt, c2a, ph, znu, dnw through
 * amt_domain_p_rho_ptr); all eight given: the caller's device arrays are used and never freed; a mix is AMT_ERR_INVALID_ARG.
 * (The library's own eight, as amt_domain_p_rho_ptr returns them, may be handed back: mode, per_sweep, t0 and smdiv are set
 * anew.)  The setting needs the stage setting of (15) on, whose t_old it reads: AMT_ERR_PRECONDITION otherwise, also from
 * amt_domain_p_rho after amt_domain_set_stage(d, 0, ...).  A refusal changes nothing.
 * per_sweep != 0: every sweep of amt_domain_step / amt_domain_step_timed is followed by one diagnosis with step != 0, behind
 * the boundary-zone update (12) and the flux accumulation (14) and in front of the guard's checks (10), where WRF has it.  Under
 * amt_slab_* and amt_grid_* it is enqueued exactly where the accumulation of the rank's own tile is, for every schedule and
 * for *_step_end; nothing is exchanged.  amt_domain_tune_placement's timed sweeps are not followed by it. */
int amt_domain_set_p_rho(amt_domain *d, int mode, int per_sweep, double t0, double smdiv,
                         void *al, void *p, void *ph, void *pm1, void *alt, void *c2a, void *znu, void *dnw);
void *amt_domain_p_rho_ptr(amt_domain *d, int which);   /* 0 al, 1 p, 2 ph, 3 pm1, 4 alt, 5 c2a, 6 znu, 7 dnw; NULL while off */
/* one diagnosis now, asynchronous on the handle's stream (the caller's for a wrapped handle): the step = 0 call behind
 * amt_domain_stage_prep, or any other; AMT_ERR_PRECONDITION while off */
int amt_domain_p_rho(amt_domain *d, int step);
/* the same for an ensemble: all members in one launch, member-stacked 3-D arrays, shared znu and dnw */
int amt_ensemble_set_p_rho(amt_ensemble *e, int mode, int per_sweep, double t0, double smdiv,
                           void *al, void *p, void *ph, void *pm1, void *alt, void *c2a, void *znu, void *dnw);
void *amt_ensemble_p_rho_ptr(amt_ensemble *e, int which);
int amt_ensemble_p_rho(amt_ensemble *e, int step);

/* ------------------------------------------------------------------------
 * (17) The momentum update that opens an acoustic sub-step: advance_uv, on the device.  In solve_em
 *      advance_uv precedes every advance_mu_t of the acoustic loop: from the p, al, ph that calc_p_rho (16) has left and the mu,
 *      mudf of the last sweep it advances u and v by the horizontal pressure gradient and the divergence damping.  The
 *      reference has no source for the routine: the definition below is this library's contract, modelled on WRF's routine,
 *      without the hybrid coordinate (c1h, c2h), top_lid and open / symmetric boundaries.
 *      Indices are Fortran-inclusive and global, on a tile its..ite, jts..jte with kts == 1 and kte == kde; T is the arrays'
 *      type.  Every operation is rounded once in T, there is no fused multiply-add, divides are IEEE divides, expressions
 *      associate exactly as written; for fp32 every scalar is rounded to float first; dx = T(1)/rdx, dy = T(1)/rdy.
 *      Outputs, in place: u, v.  3-D inputs: ru_tend, rv_tend, p, pb, ph (w levels kts..kte), php, alt, al, cqu, cqv.  2-D
 *      inputs: mu, muu, muv, mudf, msfux, msfuy, msfvx, msfvx_inv, msfvy.  1-D inputs over kms..kme, shared by the members:
 *      fnm, fnp, rdnw.  `members` >= 1 patches are member-stacked as in (8).  The flags are amt_compute_window's.
 *      RANGES, with clip = specified || nested:
 *        columns, clip && !periodic_x:  i_start = max(its, ids+1), i_end = min(ite, ide-2), i_endu = min(ite, ide-1)
 *        columns, otherwise:            i_start = its, i_endu = ite, i_end = min(ite, ide-1)
 *        rows, clip:                    j_start = max(jts, jds+1), j_end = min(jte, jde-2), j_endv = min(jte, jde-1)
 *        rows, otherwise:               j_start = jts, j_endv = jte, j_end = min(jte, jde-1)
 *        levels:                        k = kts..kte-1
 *      U PART, j = j_start..j_end, i = i_start..i_endu:
 *        mr   = msfux(i,j) / msfuy(i,j)
 *        c    = ((mr * T(0.5)) * rdx) * muu(i,j)
 *        g    = (((ph(i,k+1,j) - ph(i-1,k+1,j)) + (ph(i,k,j) - ph(i-1,k,j)))
 *                + ((alt(i,k,j) + alt(i-1,k,j)) * (p(i,k,j) - p(i-1,k,j))))
 *                + ((al(i,k,j) + al(i-1,k,j)) * (pb(i,k,j) - pb(i-1,k,j)))
 *        dpxy = c * g
 *        non_hydrostatic only:
 *          s(k)     = p(i,k,j) + p(i-1,k,j)
 *          dpn(kts) = T(0.5) * (((cf1*s(1)) + (cf2*s(2))) + (cf3*s(3)))
 *          dpn(k)   = T(0.5) * ((fnm(k)*s(k)) + (fnp(k)*s(k-1)))          k = kts+1..kte-1
 *          dpn(kte) = T(0)
 *          dpxy = dpxy + (((mr * rdx) * (php(i,k,j) - php(i-1,k,j)))
 *                         * ((rdnw(k) * (dpn(k+1) - dpn(k))) - (T(0.5) * (mu(i-1,j) + mu(i,j)))))
 *        mdx  = (((-emdiv) * dx) * (mudf(i,j) - mudf(i-1,j))) / msfuy(i,j)
 *        u    = ((u + (dts * ru_tend)) - ((dts * cqu) * dpxy)) + mdx
 *      V PART, j = j_start..j_endv, i = i_start..i_end: the same text with (i, j-1) for (i-1, j), mr = msfvy(i,j) / msfvx(i,j),
 *        rdy for rdx, muv for muu, cqv for cqu, rv_tend for ru_tend and
 *        mdy = (((-emdiv) * dy) * (mudf(i,j) - mudf(i,j-1))) * msfvx_inv(i,j)
 *      Always bit-unchanged, NaN payloads included: every cell of u, v outside its range, every memory level outside
 *      kts..kte-1, every input.  No input cell outside those the formulas name is read: php, mu, fnm, fnp, rdnw not at all
 *      when non_hydrostatic == 0.  The cells named include the mass cells at i_start-1, at j_start-1 and at column ide / row
 *      jde where i_endu / j_endv reach them: they must lie in memory and the caller supplies their values, as WRF's boundary
 *      code and halo exchange do.  No atomics, no workspace.  Inputs may alias one another; u and v overlap no other array.
 *      One launch.
 *      Reported before any device call, with or without a device, the arrays untouched, in this order: AMT_ERR_INVALID_ARG: a
 *      NULL array; members < 1.  AMT_ERR_PRECONDITION: empty memory extents.  AMT_ERR_INVALID_ARG: u or v overlaps another
 *      array.  AMT_ERR_PRECONDITION: kts != 1; kte != kde; kme < kte; the tile outside memory; more than 65535 members;
 *      non_hydrostatic with kde < 4; the cells read at i_start-1, j_start-1, i_endu, j_endv outside ims..ime, jms..jme.
 *      Empty (AMT_OK, nothing enqueued): the empty tile, kte == kts, both parts without a cell.
 *      NOT provided: the one-shot host-array calls of (1); advance_w; the stage bracket for u, v; the spec_bdyupdate
 *      of u, v on the ring; top_lid; open / symmetric boundaries; the hybrid coordinate; any exchange between ranks.
 * ------------------------------------------------------------------------ */
/* pointer level; asynchronous on hip_stream (NULL = the default stream) */
int amt_advance_uv_device_f32(
    void *hip_stream, int members, int non_hydrostatic, float *u, float *v, const float *ru_tend, const float *rv_tend,
    const float *p, const float *pb, const float *ph, const float *php, const float *alt, const float *al,
    const float *mu, const float *muu, const float *muv, const float *mudf, const float *cqu, const float *cqv,
    const float *msfux, const float *msfuy, const float *msfvx, const float *msfvx_inv, const float *msfvy,
    const float *fnm, const float *fnp, const float *rdnw,
    float rdx, float rdy, float dts, float cf1, float cf2, float cf3, float emdiv,
    int periodic_x, int specified, int nested,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);
int amt_advance_uv_device_f64(
    void *hip_stream, int members, int non_hydrostatic, double *u, double *v, const double *ru_tend, const double *rv_tend,
    const double *p, const double *pb, const double *ph, const double *php, const double *alt, const double *al,
    const double *mu, const double *muu, const double *muv, const double *mudf, const double *cqu, const double *cqv,
    const double *msfux, const double *msfuy, const double *msfvx, const double *msfvx_inv, const double *msfvy,
    const double *fnm, const double *fnp, const double *rdnw,
    double rdx, double rdy, double dts, double cf1, double cf2, double cf3, double emdiv,
    int periodic_x, int specified, int nested,
    int ids, int ide, int jds, int jde, int kde,
    int ims, int ime, int jms, int jme, int kms, int kme,
    int its, int ite, int jts, int jte, int kts, int kte);
/* on = 0: off (the default) and what the library allocated is freed; the handle's destroy frees it too.  on != 0 with ru_tend,
 * rv_tend, pb, php, cqu, cqv, msfux, msfvx, msfvy all NULL: the library allocates the nine arrays (the six 3-D ones of a 3-D
 * field's extents, the three map factors of a 2-D field's, times the members of an ensemble; the host fills them through
 * amt_domain_uv_ptr); all nine given: the caller's device arrays are used and never freed; a mix is AMT_ERR_INVALID_ARG.  (The
 * library's own nine may be handed back: per_sweep and the scalars are set anew.)  The setting needs the pressure diagnosis
 * (16) on: it reads that setting's al, p, ph, alt, and non_hydrostatic is mode 1; AMT_ERR_PRECONDITION otherwise, also from
 * amt_domain_uv after amt_domain_set_p_rho(d, 0, ...).  u, v, mu, muu, muv, mudf, msfuy, msfvx_inv, fnm, fnp, rdnw are the
 * handle's fields, rdx, rdy, dts its scalars.  A refusal changes nothing.
 * per_sweep != 0: every sweep of amt_domain_step / amt_domain_step_timed is preceded by one update, in front of the cyclic
 * refresh of (9).  amt_domain_tune_placement's timed sweeps are not preceded by it.  Under amt_slab_* and amt_grid_* the step
 * calls (step, step_timed, step_begin, step_end) return AMT_ERR_PRECONDITION with a text before they enqueue anything: the
 * halo exchange of p, al, ph, mu, mudf is not provided.
 * A handle with cyclic axes (amt_domain_set_cyclic) refreshes, on the same stream in front of every update, the wrap cells of
 * p, al, ph, alt, pb, php, mu, mudf: column ide <- ids and ids-1 <- ide-1 over the rows of the u part, row jde <- jds and
 * jds-1 <- jde-1 over the columns of the v part, every memory level, elements moved as bits. */
int amt_domain_set_uv(amt_domain *d, int on, int per_sweep, double emdiv, double cf1, double cf2, double cf3,
                      void *ru_tend, void *rv_tend, void *pb, void *php, void *cqu, void *cqv,
                      void *msfux, void *msfvx, void *msfvy);
void *amt_domain_uv_ptr(amt_domain *d, int which);   /* 0 ru_tend, 1 rv_tend, 2 pb, 3 php, 4 cqu, 5 cqv, 6 msfux, 7 msfvx, 8 msfvy; NULL while off */
/* one update now, asynchronous on the handle's stream (the caller's for a wrapped handle); AMT_ERR_PRECONDITION while off */
int amt_domain_uv(amt_domain *d);
/* the same for an ensemble: all members in one launch, member-stacked arrays */
int amt_ensemble_set_uv(amt_ensemble *e, int on, int per_sweep, double emdiv, double cf1, double cf2, double cf3,
                        void *ru_tend, void *rv_tend, void *pb, void *php, void *cqu, void *cqv,
                        void *msfux, void *msfvx, void *msfvy);
void *amt_ensemble_uv_ptr(amt_ensemble *e, int which);
int amt_ensemble_uv(amt_ensemble *e);

#ifdef __cplusplus
}
#endif

#endif /* AMT_ADVANCE_MU_T_H */
