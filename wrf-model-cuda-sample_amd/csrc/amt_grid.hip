// amt_grid.hip -- advance_mu_t on patch (ri, rj) of a pi x pj decomposition in i AND j, one process per GPU: amt_grid_*
// (include/amt_advance_mu_t.h section 5b), and -- as its pi = 1 case -- the j-slab stepper amt_slab_*
// (section 5; the reference splits j over its GPUs inside one process with host-sourced halos,
// advance_mu_t_no_async.cu:108-162).
//
// What crosses a patch boundary is amt_halo.h's table (the stencil reads (i+-1, j) and (i, j+-1) only: no diagonal neighbours).
// A j row of the (i,k,j) layout is one contiguous run and travels in place.  A column is kdim*jdim elements at stride idim:
// one launch of the mover (amt_halo.hip) gathers the columns a patch sends into two contiguous buffers (one per direction), the
// buffers travel like rows, one launch scatters what arrived into the halo columns.  The exchange engine of amt_comm.h carries
// both.
#include "amt_comm.h"
#include "amt_halo.h"
#include <vector>

struct amt_grid {
    amt_domain *dom = nullptr;
    int ri = 0, rj = 0, pi = 1, pj = 1, rank = 0, world = 1;
    int left = -1, right = -1, below = -1, above = -1;      // neighbour ranks, -1 = none
    bool overlap = true;
    AmtExchange *xchg = nullptr;
    hipStream_t comm_stream = nullptr;
    hipStream_t col_stream[2] = {nullptr, nullptr};         // the two boundary columns run beside the boundary rows
    hipEvent_t halos_in = nullptr, col_done[2] = {nullptr, nullptr};
    hipEvent_t inputs_final = nullptr, edges_done = nullptr, t0 = nullptr, t1 = nullptr;
    // Cyclic boundaries (AMT_SLAB_CYCLIC_X / _Y).  wrap_*: the direction has several ranks and the edge
    // ranks are each other's neighbours (the wrap columns / rows travel as ordinary segments); self_wrap: amt_cyclic_axes of
    // the directions with ONE rank, refreshed by amt_halo_kernel on the domain's stream in front of every sweep.
    bool wrap_x = false, wrap_y = false;
    int self_wrap = 0;
    int skew_us = 0;                                        // test hook: the neighbours' rows arrive this late
    unsigned long long packs = 0;                           // exchanges begun (what AMT_TEST_FAULT skip_pack / skip_unpack count)
    // packed columns: what goes to the left / right neighbour, what came from the right / left one
    void *to_left = nullptr, *to_right = nullptr, *from_right = nullptr, *from_left = nullptr;
    // Host-owned exchange (AMT_SLAB_TRANSPORT_EXTERNAL; header section 11): no AmtExchange; one send and
    // one receive message per side with a neighbour (order BELOW, ABOVE, LEFT, RIGHT), all carved out of ONE allocation at
    // 256-byte steps; phase: 0 = no sweep open, 1 = begun, 2 = begun and waited for.
    bool external = false, host_buffers = false;
    int phase = 0;
    int n_msg = 0;
    amt_halo_message msg[4] = {};
    void *msg_block = nullptr;
    hipEvent_t packed = nullptr, unpacked = nullptr;
};
struct amt_slab {
    amt_grid g;
};

namespace {
// First / last column and row a patch sends and the halo cells it receives into.  Without a cyclic flag: its, ite, jts, jte as
// ever.  With one, the compute window's edges (amt_compute_window) instead: the last patch of a periodic direction may end at
// ide-1 or at ide (jde-1 or jde), and what its neighbour across the domain edge reads is column ide-1 / row jde-1, what it
// receives goes to column ide / row jde.  Interior patches' windows are their tiles (the flags' preconditions rule clipping out).
struct EdgeCells { int ilo, ihi, jlo, jhi; };
EdgeCells edge_cells(const amt_grid *g)
{
    const amt_domain *d = g->dom;
    EdgeCells e{d->its, d->ite, d->jts, d->jte};
    const AmtWindow w = amt_window(d->periodic_x, d->specified, d->nested, d->ids, d->ide, d->jds, d->jde, d->its, d->ite, d->jts, d->jte, d->kts, d->kte);
    if (g->wrap_x || (g->self_wrap & AMT_CYCLIC_X)) { e.ilo = w.i_start; e.ihi = w.i_end; }
    if (g->wrap_y || (g->self_wrap & AMT_CYCLIC_Y)) { e.jlo = w.j_start; e.jhi = w.j_end; }
    return e;
}

// Appends the jobs between the arrays and ONE dense run of memory `packed` (a column buffer, a message): for every field of
// `list`, one behind the other, `per_level` runs per memory level of `len` elements each, from element (i, kms, j) on.
//   a row:  per_level = 1, len = its columns;    columns: per_level = their rows, len = 1
struct HaloJobs {
    AmtHaloJob job[AMT_HALO_MAX_JOBS];
    int n = 0;
};
void halo_jobs(HaloJobs &out, const amt_domain *d, const AmtHaloFields &list, int i, int j, long per_level, int len, void *packed, bool scatter)
{
    const long idim = d->ime - d->ims + 1, kdim = d->kme - d->kms + 1;
    const size_t es = (size_t)d->dtype_bytes;
    char *p = static_cast<char *>(packed);
    for (int q = 0; q < list.n; ++q) {
        const int f = list.field[q];
        char *a = static_cast<char *>(d->field[f]) + (size_t)amt_halo_at(*d, f, i, j) * es;
        const long runs = amt_halo_levels(f, kdim) * per_level;
        out.job[out.n++] = scatter ? AmtHaloJob{p, a, runs, len, len, idim, 0} : AmtHaloJob{a, p, runs, len, idim, len, 0};
        p += (size_t)(runs * len) * es;
    }
}

// bytes of the packed whole memory columns (every level, every memory row) received from `side`
size_t column_bytes(const amt_domain *d, int side)
{
    return (size_t)amt_halo_elems(side, d->kme - d->kms + 1) * (size_t)(d->jme - d->jms + 1) * (size_t)d->dtype_bytes;
}

// One launch gathers the columns the patch sends into to_left / to_right (scatter = false) or scatters from_right / from_left
// into its halo columns (true).
int grid_columns(amt_grid *g, hipStream_t stream, bool scatter)
{
    amt_domain *d = g->dom;
    const EdgeCells ec = edge_cells(g);
    const long jdim = d->jme - d->jms + 1;
    HaloJobs jobs;
    if (scatter) {
        if (g->right >= 0) halo_jobs(jobs, d, amt_halo_recv(AMT_HALO_RIGHT), ec.ihi + 1, d->jms, jdim, 1, g->from_right, true);
        if (g->left >= 0) halo_jobs(jobs, d, amt_halo_recv(AMT_HALO_LEFT), ec.ilo - 1, d->jms, jdim, 1, g->from_left, true);
    } else {
        if (g->left >= 0) halo_jobs(jobs, d, amt_halo_sent(AMT_HALO_LEFT), ec.ilo, d->jms, jdim, 1, g->to_left, false);
        if (g->right >= 0) halo_jobs(jobs, d, amt_halo_sent(AMT_HALO_RIGHT), ec.ihi, d->jms, jdim, 1, g->to_right, false);
    }
    return amt_halo_launch(stream, d->dtype_bytes, 1, jobs.job, jobs.n);
}
int grid_pack(amt_grid *g, hipStream_t s)
{
    if (amt_test_fault("skip_pack", ++g->packs)) return AMT_OK;
    return grid_columns(g, s, false);
}
int grid_unpack(amt_grid *g, hipStream_t s)
{
    if (amt_test_fault("skip_unpack", g->packs)) return AMT_OK;
    return grid_columns(g, s, true);
}

// Test hook (amt_*_set_skew_us, RCCL transport): holds the communication stream for `ticks` of the 100 MHz real-time counter, so
// that the exchange behind it starts -- and the neighbours' rows arrive -- that much late.  AMT_SLAB_SKEW_WGS=n (default 1) gives
// the delay the footprint of RCCL's waiting send/recv kernel: n workgroups of 256 threads, each with enough LDS to have a compute
// unit to itself.  (The IPC transport carries the delay inside its own waiting kernel.)
__global__ void amt_grid_delay_kernel(unsigned long long ticks)
{
    extern __shared__ unsigned char amt_delay_lds[];
    if (threadIdx.x == 0) amt_delay_lds[0] = 0;
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

template <typename T>
int grid_tile(amt_grid *g, hipStream_t stream, int its, int ite, int jts, int jte, bool beside_the_exchange = false, bool thin_column = false)
{
    if (jte < jts || ite < its) return AMT_OK;
    AmtArgs<T> a;
    amt_domain_args<T>(g->dom, a);
    a.its = its; a.ite = ite; a.jts = jts; a.jte = jte;
    // A boundary COLUMN is one column wide: the march kernel streams a whole tile for it; the column kernel -- one lane per
    // column, the same bits -- would touch one line per element instead.
    // Measured: the column kernel is the SLOWER one here (2048^2 patch: +18 % against +8.6 % per sweep, one active lane per
    // workgroup walking its levels in sequence): off unless AMT_GRID_THIN_COLUMNS=1.
    static const bool thin_env = [] { const char *e = getenv("AMT_GRID_THIN_COLUMNS"); return e && *e && atoi(e) != 0; }();
    if (thin_column && thin_env && g->dom->variant == AMT_VARIANT_AUTO) return amt_device_call<T>(stream, AMT_VARIANT_COLUMN, a);
    // A launch that is ONE round of workgroups (the launcher's choice for a patch on its own) holds every compute unit
    // until it ends; beside the exchange the interior is planned as amt_march_set_beside says (profiles/r05_slab_ab.md).
    return beside_the_exchange ? amt_device_call_shared<T>(stream, g->dom->variant, a) : amt_device_call<T>(stream, g->dom->variant, a);
}

// Specified / nested boundaries (amt_domain_set_spec_bdy): the boundary-zone update of this rank's own
// tile, on the domain's stream where the sweep's work has joined it.  The zone holds outputs only: nothing is exchanged for it,
// and a patch that touches no domain edge enqueues nothing.
// With amt_domain_set_sumflux the flux accumulation of this rank's own tile follows at the same place:
// its operands are this rank's u, v and the ww the sweep has just written, nothing is exchanged for it either.
// With amt_domain_set_p_rho(per_sweep) the pressure diagnosis of this rank's own tile follows the
// accumulation: it reads the t, mu and muts the sweep has just written in the tile's own columns, nothing is exchanged.
// The part of a resident handle's sweep sequence behind the sweep (amt_domain.hip), without the guard check: these steppers do
// not run the non-finite guard.
int grid_bdy(amt_grid *g, const char *who) { return amt_handle_behind_sweep(who, g->dom, 1); }

// the cells that read a neighbour's data, after the halos are in: boundary rows over the patch's whole width (they own the
// corners), boundary columns over the rows in between; every tile is clipped on its own by the routine's window rule
template <typename T>
int grid_edges(amt_grid *g, hipStream_t edge_stream, bool lo, bool hi, bool lf, bool rt, bool unclipped, int in_jlo, int in_jhi)
{
    amt_domain *d = g->dom;
    const EdgeCells ec = edge_cells(g);
    const int ilo = ec.ilo, ihi = ec.ihi, jlo = ec.jlo, jhi = ec.jhi;
    int rc = AMT_OK;
    // The boundary columns are independent of the rows and of each other: they go to streams of their own (three small
    // launches, the chip has room for all of them at once) behind the event "halos are in", and join the edge stream.
    const bool fork = (lf || rt) && g->col_stream[0] && edge_stream == g->comm_stream;
    if (fork) AMT_HIP(hipEventRecord(g->halos_in, edge_stream));
    int used = 0;
    auto column = [&](int c) -> int {
        hipStream_t st = fork ? g->col_stream[used] : edge_stream;
        if (fork) AMT_HIP(hipStreamWaitEvent(st, g->halos_in, 0));
        const int rc2 = grid_tile<T>(g, st, c, c, in_jlo, in_jhi, false, true);
        if (fork) (void)hipEventRecord(g->col_done[used++], st);
        return rc2;
    };
    if (lf) rc = column(ilo < ihi ? ilo : ihi);
    if (rc == AMT_OK && rt && (ihi > ilo || !lf)) rc = column(ihi);
    if (rc == AMT_OK) {
        if (lo && hi && jhi > jlo && unclipped) {                       // both rows in one launch
            AmtArgs<T> a;
            amt_domain_args<T>(d, a);
            a.jts = jlo; a.jte = jhi;
            rc = amt_device_call_edges<T>(edge_stream, d->variant, a);
        } else {                                                        // one-row tiles
            if (lo) rc = grid_tile<T>(g, edge_stream, ilo, ihi, jlo, jlo < jhi ? jlo : jhi);
            if (rc == AMT_OK && hi && (jhi > jlo || !lo)) rc = grid_tile<T>(g, edge_stream, ilo, ihi, jhi, jhi);
        }
    }
    for (int q = 0; q < used; ++q) (void)hipStreamWaitEvent(edge_stream, g->col_done[q], 0);      // always joined, also after an error
    return rc;
}

template <typename T>
int grid_step_t(amt_grid *g, int n_sweeps)
{
    amt_domain *d = g->dom;
    const EdgeCells ec = edge_cells(g);
    const int ilo = ec.ilo, ihi = ec.ihi, jlo = ec.jlo, jhi = ec.jhi;
    const bool lo = g->below >= 0, hi = g->above >= 0, lf = g->left >= 0, rt = g->right >= 0;
    // the rows the routine really updates in this patch (module_small_step_em.f90:91-106): with specified / nested boundaries
    // the first / last row of an outermost patch is clipped away.  Every tile below is clipped on its own by the same rule;
    // only the one-launch path for both boundary rows computes rows j_start and j_end of the CLIPPED window, so it is taken only
    // when nothing is clipped (always, for a patch with a neighbour on that side -- except in loopback, where the rank is its
    // own neighbour on a patch that touches the domain edge).
    const AmtWindow wclip = amt_window(d->periodic_x, d->specified, d->nested, d->ids, d->ide, d->jds, d->jde,
                                       ilo, ihi, jlo, jhi, d->kts, d->kte);
    const bool unclipped = wclip.j_start == jlo && wclip.j_end == jhi;
    // a failure between the fork (inputs_final) and the join (edges_done) must not leave the streams apart
    auto join = [&]() {
        (void)hipEventRecord(g->edges_done, g->comm_stream);
        (void)hipStreamWaitEvent(d->stream, g->edges_done, 0);
    };
    const bool none = !lo && !hi && !lf && !rt;
    // cells that read a neighbour's data: rows jlo / jhi, columns ilo / ihi; the rest is interior
    const int in_jlo = jlo + (lo ? 1 : 0), in_jhi = jhi - (hi ? 1 : 0);
    const int in_ilo = ilo + (lf ? 1 : 0), in_ihi = ihi - (rt ? 1 : 0);
    const bool ipc = amt_exchange_transport(g->xchg) == AMT_XCHG_IPC && amt_exchange_active(g->xchg);
    static const bool host_wait_env = [] { const char *e = getenv("AMT_IPC_HOST_WAIT"); return !(e && *e && atoi(e) == 0); }();
    static const int order_env = [] { const char *e = getenv("AMT_SLAB_EXCHANGE_FIRST"); return e && *e ? atoi(e) : -1; }();
    auto delay_for_the_test_hook = [&](hipStream_t stream) {
        if (g->skew_us <= 0 || amt_exchange_owns_skew(g->xchg)) return;
        static const int wgs = [] { const char *e = getenv("AMT_SLAB_SKEW_WGS"); const int n = e ? atoi(e) : 1; return n > 1 ? n : 1; }();
        if (wgs > 1) {
            static const bool granted = hipFuncSetAttribute(reinterpret_cast<const void *>(amt_grid_delay_kernel),
                                                            hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) == hipSuccess;
            hipLaunchKernelGGL(amt_grid_delay_kernel, dim3(wgs), dim3(256), granted ? 96 * 1024 : 48 * 1024, stream, (unsigned long long)g->skew_us * 100ull);
        } else {
            hipLaunchKernelGGL(amt_grid_delay_kernel, dim3(1), dim3(1), 16, stream, (unsigned long long)g->skew_us * 100ull);
        }
    };
    for (int sweep = 0; sweep < n_sweeps; ++sweep) {
        // a device-side wait of an EARLIER sweep that gave up (IPC transport: a neighbour that never posted or never pulled):
        // that sweep's halo rows were not valid, so nothing is built on top of it -- the step fails here, not only in *_sync
        int rc = amt_exchange_check(g->xchg);
        if (rc) return rc;
        // a cyclic direction with ONE rank: the patch is its own neighbour there, no transport -- the refresh kernel on the
        // domain's stream in front of everything else of the sweep (the inputs are final here); that direction adds no
        // boundary columns or rows to the edge launches
        if (g->self_wrap) {
            rc = amt_cyclic_refresh_domain("amt_grid_step", d, g->self_wrap, 1);
            if (rc) return rc;
        }
        if (none) {                                                        // a world of one: the plain launch
            rc = grid_tile<T>(g, d->stream, ilo, ihi, jlo, jhi);
            if (rc == AMT_OK) rc = grid_bdy(g, "amt_grid_step");
            if (rc) return rc;
            continue;
        }
        if (!g->overlap) {
            // (1) NO OVERLAP: the halos first, then the WHOLE patch as one launch (nothing to split when nothing runs beside)
            rc = grid_pack(g, d->stream);
            if (rc == AMT_OK) delay_for_the_test_hook(d->stream);
            if (rc == AMT_OK) rc = amt_exchange_enqueue(g->xchg, d->stream, true);
            if (rc == AMT_OK) rc = grid_unpack(g, d->stream);
            if (rc == AMT_OK) rc = grid_tile<T>(g, d->stream, ilo, ihi, jlo, jhi);
            if (rc == AMT_OK) rc = amt_exchange_enqueue_release(g->xchg, d->stream);
            if (rc == AMT_OK) rc = grid_bdy(g, "amt_grid_step");
            if (rc) return rc;
            continue;
        }
        if (ipc && host_wait_env) {
            // (2) HOST-WAITED (IPC transport, default; AMT_IPC_HOST_WAIT=0 for (3)).  A march workgroup takes a compute unit whole,
            // so nothing can run BESIDE the interior (profiles/r05_slab_ab.md): here nothing of the exchange holds a unit while
            // the interior runs, the interior is planned on its own -- one round where it can be one, full efficiency -- and the
            // neighbours' lateness hides behind ALL of it:
            //   domain stream: [gather columns] -> refresh the staging copies -> post "rows final n" (one wave) -> interior
            //   host:          poll the mailbox until every neighbour has posted n (the call returns after that: per sub-step,
            //                  as a host that exchanges by MPI would wait)
            //   comm stream:   pull (copy engine between GPUs; one kernel on a shared device) -> post "pulled n" -> [scatter
            //                  columns] -> boundary rows / columns -> wait until the neighbours have pulled -> join
            // The boundary tiles get their compute units when the interior's workgroups end: they run right behind it.
            rc = grid_pack(g, d->stream);
            if (rc == AMT_OK) rc = amt_exchange_enqueue_post(g->xchg, d->stream);
            if (rc) return rc;
            if (hipEventRecord(g->inputs_final, d->stream) != hipSuccess || hipStreamWaitEvent(g->comm_stream, g->inputs_final, 0) != hipSuccess)
                return amt_fail(AMT_ERR_HIP, "amt_grid_step: cannot fork the communication stream: %s", hipGetErrorString(hipGetLastError()));
            rc = grid_tile<T>(g, d->stream, in_ilo, in_ihi, in_jlo, in_jhi);       // on its own: the launcher's best plan
            if (rc == AMT_OK) rc = amt_exchange_host_wait(g->xchg);
            if (rc == AMT_OK) rc = amt_exchange_enqueue_pull(g->xchg, g->comm_stream);
            if (rc == AMT_OK) rc = grid_unpack(g, g->comm_stream);
            if (rc == AMT_OK) rc = grid_edges<T>(g, g->comm_stream, lo, hi, lf, rt, unclipped, in_jlo, in_jhi);
            if (rc == AMT_OK) rc = amt_exchange_enqueue_release(g->xchg, g->comm_stream);
            join();                                                        // also after an error: the streams never stay apart
            if (rc == AMT_OK) rc = grid_bdy(g, "amt_grid_step");           // behind the join: on the domain's stream
            if (rc) return rc;
            continue;
        }
        // (3) DEVICE-WAITED (RCCL; IPC with AMT_IPC_HOST_WAIT=0): the exchange on the communication stream, the interior BESIDE it
        // on the domain's stream, planned by amt_march_set_beside (rounds, reserved units).  Whatever the communication stream
        // launches once the interior is out starts only where an interior workgroup ends; the IPC transport's waiting kernel
        // therefore goes out FIRST (it has its units from the start of the sweep), RCCL's send/recv kernel -- which holds its
        // units for as long as it waits -- after the interior (AMT_SLAB_EXCHANGE_FIRST=0|1 overrides either).
        const bool exchange_first = order_env >= 0 ? order_env != 0 : ipc;
        if (hipEventRecord(g->inputs_final, d->stream) != hipSuccess || hipStreamWaitEvent(g->comm_stream, g->inputs_final, 0) != hipSuccess)
            return amt_fail(AMT_ERR_HIP, "amt_grid_step: cannot fork the communication stream: %s", hipGetErrorString(hipGetLastError()));
        if (!exchange_first) rc = grid_tile<T>(g, d->stream, in_ilo, in_ihi, in_jlo, in_jhi, true);
        if (rc == AMT_OK) delay_for_the_test_hook(g->comm_stream);
        if (rc == AMT_OK) rc = grid_pack(g, g->comm_stream);               // the columns this patch sends, gathered
        if (rc == AMT_OK) rc = amt_exchange_enqueue(g->xchg, g->comm_stream);
        if (rc == AMT_OK && exchange_first) rc = grid_tile<T>(g, d->stream, in_ilo, in_ihi, in_jlo, in_jhi, true);
        if (rc == AMT_OK) rc = grid_unpack(g, g->comm_stream);             // the columns that arrived, scattered into the halo
        if (rc == AMT_OK) rc = grid_edges<T>(g, g->comm_stream, lo, hi, lf, rt, unclipped, in_jlo, in_jhi);
        // the sweep ends when the neighbours have this sweep's rows (RCCL: the sends of the group have completed; IPC: they
        // have pulled them)
        if (rc == AMT_OK) rc = amt_exchange_enqueue_release(g->xchg, g->comm_stream);
        join();
        if (rc == AMT_OK) rc = grid_bdy(g, "amt_grid_step");
        if (rc) return rc;
    }
    return AMT_OK;
}

void grid_teardown(amt_grid *g)
{
    DeviceScope scope(g->dom ? g->dom->device : 0);
    if (g->comm_stream) (void)hipStreamSynchronize(g->comm_stream);
    (void)amt_exchange_destroy(g->xchg);
    g->xchg = nullptr;
    for (hipStream_t st : {g->col_stream[0], g->col_stream[1]})
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    for (hipEvent_t e : {g->inputs_final, g->edges_done, g->t0, g->t1, g->halos_in, g->col_done[0], g->col_done[1], g->packed, g->unpacked})
        if (e) (void)hipEventDestroy(e);
    if (g->comm_stream) (void)hipStreamDestroy(g->comm_stream);
    for (void *q : {g->to_left, g->to_right, g->from_right, g->from_left})
        if (q) (void)hipFree(q);
    if (g->msg_block) (void)(g->host_buffers ? hipHostFree(g->msg_block) : hipFree(g->msg_block));
    g->msg_block = nullptr;
}

// Who the neighbours are and whether the shape admits the flags: host arithmetic only, nothing of the device is touched (what
// amt_grid_create and the planner amt_halo_plan share).  loop_i / loop_j: one-rank test mode -- the rank is its own neighbour
// across i / across j.  id_given: the caller has a communicator id (a host-owned exchange needs none).
int grid_topology(amt_grid *g, amt_domain *dom, int ri, int rj, int pi, int pj, bool id_given, int flags, bool loop_i, bool loop_j)
{
    if (!dom || pi < 1 || pj < 1 || ri < 0 || ri >= pi || rj < 0 || rj >= pj) return amt_fail(AMT_ERR_INVALID_ARG, "bad patch index");
    const int world = pi * pj, rank = rj * pi + ri;
    const bool external = (flags & AMT_SLAB_TRANSPORT_EXTERNAL) != 0;
    if (external && (loop_i || loop_j || (flags & AMT_SLAB_LOOPBACK)))
        return amt_fail(AMT_ERR_INVALID_ARG, "AMT_SLAB_LOOPBACK cannot be combined with AMT_SLAB_TRANSPORT_EXTERNAL: the host is the transport");
    if (external && (flags & AMT_SLAB_TRANSPORT_IPC))
        return amt_fail(AMT_ERR_INVALID_ARG, "AMT_SLAB_TRANSPORT_IPC and AMT_SLAB_TRANSPORT_EXTERNAL name two transports");
    if (!external && (flags & AMT_SLAB_EXTERNAL_HOST_BUFFERS))
        return amt_fail(AMT_ERR_INVALID_ARG, "AMT_SLAB_EXTERNAL_HOST_BUFFERS is an option of AMT_SLAB_TRANSPORT_EXTERNAL");
    if ((loop_i || loop_j) && world != 1) return amt_fail(AMT_ERR_INVALID_ARG, "loopback is a one-rank test mode");
    const bool comm_needed = !external && (world > 1 || loop_i || loop_j);
    if (comm_needed && !id_given) return amt_fail(AMT_ERR_INVALID_ARG, "a communicator needs the unique id");
    g->external = external;
    g->host_buffers = external && (flags & AMT_SLAB_EXTERNAL_HOST_BUFFERS) != 0;
    g->dom = dom; g->ri = ri; g->rj = rj; g->pi = pi; g->pj = pj; g->rank = rank; g->world = world;
    g->overlap = !(flags & AMT_SLAB_NO_OVERLAP);
    const bool cyc_x = (flags & AMT_SLAB_CYCLIC_X) != 0, cyc_y = (flags & AMT_SLAB_CYCLIC_Y) != 0;
    if ((cyc_x || cyc_y) && (loop_i || loop_j || (flags & AMT_SLAB_LOOPBACK)))
        return amt_fail(AMT_ERR_INVALID_ARG, "AMT_SLAB_LOOPBACK cannot be combined with AMT_SLAB_CYCLIC_X / AMT_SLAB_CYCLIC_Y");
    if (cyc_x && !dom->periodic_x && (dom->specified || dom->nested))
        return amt_fail(AMT_ERR_PRECONDITION, "AMT_SLAB_CYCLIC_X needs an unclipped i window: periodic_x, or neither specified nor nested");
    if (cyc_y && (dom->specified || dom->nested))
        return amt_fail(AMT_ERR_PRECONDITION, "AMT_SLAB_CYCLIC_Y needs an unclipped j window: neither specified nor nested");
    // Torus: with several ranks in a cyclic direction the edge ranks are each other's neighbours.  With exactly TWO, both
    // neighbours are the same peer and there are two sets of segments per pair; the engine pairs the k-th segment sent to a
    // peer with the k-th received from it, and the lists below keep that order: towards below / left first, then towards
    // above / right, on the sending side; from above / right first, then from below / left, on the receiving side (what I
    // send "below" is what my peer receives "from above").
    g->wrap_x = cyc_x && pi > 1;
    g->wrap_y = cyc_y && pj > 1;
    g->self_wrap = (cyc_x && pi == 1 ? AMT_CYCLIC_X : 0) | (cyc_y && pj == 1 ? AMT_CYCLIC_Y : 0);
    g->left = loop_i ? rank : ri > 0 ? rank - 1 : g->wrap_x ? rank + (pi - 1) : -1;
    g->right = loop_i ? rank : ri < pi - 1 ? rank + 1 : g->wrap_x ? rank - (pi - 1) : -1;
    g->below = loop_j ? rank : rj > 0 ? rank - pi : g->wrap_y ? rank + pi * (pj - 1) : -1;
    g->above = loop_j ? rank : rj < pj - 1 ? rank + pi : g->wrap_y ? rank - pi * (pj - 1) : -1;
    if (g->self_wrap) {
        const int rc = amt_cyclic_check_domain("amt_grid_create", dom, g->self_wrap, 1);
        if (rc) return rc;
    }
    const EdgeCells ec = edge_cells(g);
    if ((g->below >= 0 || g->above >= 0) && (ec.jlo - 1 < dom->jms || ec.jhi + 1 > dom->jme))
        return amt_fail(AMT_ERR_PRECONDITION, "a patch holds one halo row below jts and above jte");
    if ((g->left >= 0 || g->right >= 0) && (ec.ilo - 1 < dom->ims || ec.ihi + 1 > dom->ime))
        return amt_fail(AMT_ERR_PRECONDITION, "a patch holds one halo column left of its and right of ite");
    return AMT_OK;
}

// ---------------------------------------------------------------------------
// The host-owned exchange (AMT_SLAB_TRANSPORT_EXTERNAL; header section 11)
// ---------------------------------------------------------------------------
// side, peer and the byte counts of the messages of g (order BELOW, ABOVE, LEFT, RIGHT); pointers NULL.  Host arithmetic.
int halo_plan(const amt_grid *g, amt_halo_message out[4])
{
    const amt_domain *d = g->dom;
    const EdgeCells ec = edge_cells(g);
    const long kdim = d->kme - d->kms + 1;
    const size_t ni = ec.ihi >= ec.ilo ? ec.ihi - ec.ilo + 1 : 0, nj = ec.jhi >= ec.jlo ? ec.jhi - ec.jlo + 1 : 0;
    const int peer[AMT_HALO_SIDES] = {g->below, g->above, g->left, g->right};
    int n = 0;
    for (int side = 0; side < AMT_HALO_SIDES; ++side) {
        if (peer[side] < 0) continue;
        const size_t edge_bytes = (amt_halo_is_column(side) ? nj : ni) * (size_t)d->dtype_bytes;
        out[n++] = amt_halo_message{1 << side, peer[side], nullptr, (size_t)amt_halo_elems(side ^ 1, kdim) * edge_bytes, nullptr,
                                    (size_t)amt_halo_elems(side, kdim) * edge_bytes, g->host_buffers ? 1 : 0};
    }
    return n;
}

int external_buffers(amt_grid *g)
{
    g->n_msg = halo_plan(g, g->msg);
    auto step = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
    size_t total = 0;
    for (int m = 0; m < g->n_msg; ++m) total += step(g->msg[m].send_bytes) + step(g->msg[m].recv_bytes);
    if (total == 0) return AMT_OK;
    // hipMalloc and hipHostMalloc return bases aligned far beyond 256 bytes
    const hipError_t e = g->host_buffers ? hipHostMalloc(&g->msg_block, total, hipHostMallocDefault) : hipMalloc(&g->msg_block, total);
    if (e != hipSuccess) {
        g->msg_block = nullptr;
        return amt_fail(e == hipErrorOutOfMemory ? AMT_ERR_ALLOC : AMT_ERR_HIP, "amt_grid_create: the halo messages (%zu bytes): %s", total, hipGetErrorString(e));
    }
    char *at = static_cast<char *>(g->msg_block);
    for (int m = 0; m < g->n_msg; ++m) {
        g->msg[m].send = at; at += step(g->msg[m].send_bytes);
        g->msg[m].recv = at; at += step(g->msg[m].recv_bytes);
    }
    return AMT_OK;
}

// One launch for everything the patch sends (scatter = false: rows jlo / jhi and columns ilo / ihi into the send messages) or
// for everything that arrived (true: the receive messages into rows jhi+1 / jlo-1 and columns ihi+1 / ilo-1).
int external_move(amt_grid *g, hipStream_t stream, bool scatter)
{
    amt_domain *d = g->dom;
    const EdgeCells ec = edge_cells(g);
    const long ni = ec.ihi - ec.ilo + 1, nj = ec.jhi - ec.jlo + 1;
    if (ni < 1 || nj < 1) return AMT_OK;
    // per side: the edge cell the patch sends, the halo cell it receives into
    const int sent[AMT_HALO_SIDES] = {ec.jlo, ec.jhi, ec.ilo, ec.ihi}, halo[AMT_HALO_SIDES] = {ec.jlo - 1, ec.jhi + 1, ec.ilo - 1, ec.ihi + 1};
    HaloJobs jobs;
    for (int k = 0; k < g->n_msg; ++k) {
        const amt_halo_message &m = g->msg[k];
        const int side = amt_halo_side_index(m.side), cell = scatter ? halo[side] : sent[side];
        const AmtHaloFields &list = scatter ? amt_halo_recv(side) : amt_halo_sent(side);
        void *msg = scatter ? m.recv : m.send;
        if (amt_halo_is_column(side)) halo_jobs(jobs, d, list, cell, ec.jlo, nj, 1, msg, scatter);
        else halo_jobs(jobs, d, list, ec.ilo, cell, 1, (int)ni, msg, scatter);
    }
    return amt_halo_launch(stream, d->dtype_bytes, 1, jobs.job, jobs.n);
}

int external_only(const amt_grid *g, const char *who)
{
    if (g->external) return AMT_OK;
    return amt_fail(AMT_ERR_INVALID_ARG, "%s needs a handle made with AMT_SLAB_TRANSPORT_EXTERNAL", who);
}

int not_for_external(const amt_grid *g, const char *who)
{
    if (!g->external) return AMT_OK;
    return amt_fail(AMT_ERR_INVALID_ARG, "%s: the host moves this handle's halos (AMT_SLAB_TRANSPORT_EXTERNAL): call amt_grid_step_begin / "
                    "amt_grid_halo_wait / amt_grid_step_end (amt_slab_*) per sweep, or amt_grid_halo_pack / amt_grid_halo_unpack", who);
}

// refresh (a cyclic direction with one rank), pack, "packed" -- on the domain's stream, where the inputs are final
int external_pack(amt_grid *g, const char *who)
{
    amt_domain *d = g->dom;
    int rc = g->self_wrap ? amt_cyclic_refresh_domain(who, d, g->self_wrap, 1) : AMT_OK;
    if (rc == AMT_OK) rc = external_move(g, d->stream, false);
    if (rc) return rc;
    AMT_HIP(hipEventRecord(g->packed, d->stream));
    return AMT_OK;
}

template <typename T>
int external_begin_t(amt_grid *g)
{
    amt_domain *d = g->dom;
    const EdgeCells ec = edge_cells(g);
    const bool lo = g->below >= 0, hi = g->above >= 0, lf = g->left >= 0, rt = g->right >= 0;
    if (g->n_msg == 0) {                                                   // no neighbour at all: the plain launch
        const int rc = g->self_wrap ? amt_cyclic_refresh_domain("amt_grid_step_begin", d, g->self_wrap, 1) : AMT_OK;
        return rc ? rc : grid_tile<T>(g, d->stream, ec.ilo, ec.ihi, ec.jlo, ec.jhi);
    }
    const int rc = external_pack(g, "amt_grid_step_begin");
    if (rc || !g->overlap) return rc;
    // the interior on its own, the launcher's best plan: nothing of the exchange holds a compute unit beside it
    return grid_tile<T>(g, d->stream, ec.ilo + (lf ? 1 : 0), ec.ihi - (rt ? 1 : 0), ec.jlo + (lo ? 1 : 0), ec.jhi - (hi ? 1 : 0));
}

template <typename T>
int external_end_t(amt_grid *g)
{
    amt_domain *d = g->dom;
    if (g->n_msg == 0) return grid_bdy(g, "amt_grid_step_end");           // begin was the plain launch
    const EdgeCells ec = edge_cells(g);
    const bool lo = g->below >= 0, hi = g->above >= 0, lf = g->left >= 0, rt = g->right >= 0;
    if (!g->overlap) {
        int rc = external_move(g, d->stream, true);
        if (rc) return rc;
        AMT_HIP(hipEventRecord(g->unpacked, d->stream));
        rc = grid_tile<T>(g, d->stream, ec.ilo, ec.ihi, ec.jlo, ec.jhi);
        return rc ? rc : grid_bdy(g, "amt_grid_step_end");
    }
    const AmtWindow wclip = amt_window(d->periodic_x, d->specified, d->nested, d->ids, d->ide, d->jds, d->jde,
                                       ec.ilo, ec.ihi, ec.jlo, ec.jhi, d->kts, d->kte);
    const bool unclipped = wclip.j_start == ec.jlo && wclip.j_end == ec.jhi;
    AMT_HIP(hipStreamWaitEvent(g->comm_stream, g->packed, 0));
    int rc = external_move(g, g->comm_stream, true);
    if (rc == AMT_OK && hipEventRecord(g->unpacked, g->comm_stream) != hipSuccess)
        rc = amt_fail(AMT_ERR_HIP, "amt_grid_step_end: cannot record the unpack: %s", hipGetErrorString(hipGetLastError()));
    if (rc == AMT_OK) rc = grid_edges<T>(g, g->comm_stream, lo, hi, lf, rt, unclipped, ec.jlo + (lo ? 1 : 0), ec.jhi - (hi ? 1 : 0));
    (void)hipEventRecord(g->edges_done, g->comm_stream);                   // also after an error: the streams never stay apart
    (void)hipStreamWaitEvent(d->stream, g->edges_done, 0);
    return rc ? rc : grid_bdy(g, "amt_grid_step_end");                    // behind the join: on the domain's stream
}

// advance_uv in front of every sweep needs the halo cells of p, al, ph, mu, mudf of the neighbours: that exchange is not
// provided, so a stepper refuses to step a handle with the per-sweep setting on, before it enqueues anything
int uv_refused(const amt_grid *g, const char *who)
{
    return g->dom->uv_per_sweep ? amt_fail(AMT_ERR_PRECONDITION, "%s: advance_uv in front of every sweep (amt_domain_set_uv, per_sweep) is not "
                                           "provided under a stepper: the halo exchange of p, al, ph, mu, mudf is missing", who) : AMT_OK;
}

int external_begin(amt_grid *g)
{
    int rc = external_only(g, "amt_grid_step_begin");
    if (rc) return rc;
    if ((rc = uv_refused(g, "amt_grid_step_begin")) != AMT_OK) return rc;
    if (g->phase != 0) return amt_fail(AMT_ERR_INVALID_ARG, "amt_grid_step_begin: the previous sweep is still open (amt_grid_step_end closes it)");
    DeviceScope scope(g->dom->device);
    rc = g->dom->dtype_bytes == 8 ? external_begin_t<double>(g) : external_begin_t<float>(g);
    if (rc == AMT_OK) g->phase = 1;
    return rc;
}

int external_wait(amt_grid *g)
{
    int rc = external_only(g, "amt_grid_halo_wait");
    if (rc) return rc;
    if (g->phase != 1) return amt_fail(AMT_ERR_INVALID_ARG, "amt_grid_halo_wait: once per sweep, between amt_grid_step_begin and amt_grid_step_end");
    g->phase = 2;
    if (g->n_msg == 0) return AMT_OK;
    DeviceScope scope(g->dom->device);
    AMT_HIP(hipEventSynchronize(g->packed));        // this sweep's send messages are complete
    AMT_HIP(hipEventSynchronize(g->unpacked));      // the previous sweep's receive messages have been read (at once before the first)
    return AMT_OK;
}

int external_end(amt_grid *g)
{
    int rc = external_only(g, "amt_grid_step_end");
    if (rc) return rc;
    if ((rc = uv_refused(g, "amt_grid_step_end")) != AMT_OK) return rc;
    if (g->phase == 0) return amt_fail(AMT_ERR_INVALID_ARG, "amt_grid_step_end without amt_grid_step_begin");
    DeviceScope scope(g->dom->device);
    g->phase = 0;
    return g->dom->dtype_bytes == 8 ? external_end_t<double>(g) : external_end_t<float>(g);
}

int external_pack_only(amt_grid *g, bool unpack)
{
    const char *who = unpack ? "amt_grid_halo_unpack" : "amt_grid_halo_pack";
    int rc = external_only(g, who);
    if (rc) return rc;
    if (g->phase != 0) return amt_fail(AMT_ERR_INVALID_ARG, "%s inside an open sweep (amt_grid_step_begin packs, amt_grid_step_end unpacks)", who);
    if (g->n_msg == 0 && !g->self_wrap) return AMT_OK;
    DeviceScope scope(g->dom->device);
    if (!unpack) return external_pack(g, who);
    rc = external_move(g, g->dom->stream, true);
    if (rc) return rc;
    AMT_HIP(hipEventRecord(g->unpacked, g->dom->stream));
    return AMT_OK;
}

int external_messages(amt_grid *g, amt_halo_message *out, int cap, int *n)
{
    if (!n || cap < 0 || (cap > 0 && !out)) return amt_fail(AMT_ERR_INVALID_ARG, "amt_grid_halo_messages: bad argument");
    const int rc = external_only(g, "amt_grid_halo_messages");
    if (rc) return rc;
    *n = g->n_msg;
    if (g->n_msg > cap) return amt_fail(AMT_ERR_INVALID_ARG, "amt_grid_halo_messages: %d messages, room for %d", g->n_msg, cap);
    for (int m = 0; m < g->n_msg; ++m) out[m] = g->msg[m];
    return AMT_OK;
}

int grid_setup(amt_grid *g, amt_domain *dom, int ri, int rj, int pi, int pj, const void *unique_id, int flags, bool loop_i, bool loop_j)
{
    int rc = grid_topology(g, dom, ri, rj, pi, pj, unique_id != nullptr, flags, loop_i, loop_j);
    if (rc) return rc;
    const int rank = g->rank, world = g->world;
    const EdgeCells ec = edge_cells(g);
    int transport = (flags & AMT_SLAB_TRANSPORT_IPC) ? AMT_XCHG_IPC : AMT_XCHG_RCCL;
    if (const char *e = g->external ? nullptr : getenv("AMT_SLAB_TRANSPORT")) {                  // hosts that cannot pass the flag (the Fortran drivers)
        if (!strcmp(e, "ipc")) transport = AMT_XCHG_IPC;
        else if (!strcmp(e, "rccl")) transport = AMT_XCHG_RCCL;
        else if (*e) return amt_fail(AMT_ERR_INVALID_ARG, "AMT_SLAB_TRANSPORT must be rccl or ipc, not '%s'", e);
    }
    DeviceScope scope(dom->device);
    // the communication stream outranks the domain's: where a compute unit is free, the exchange and the edge tiles get it
    int prio_low = 0, prio_high = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);
    hipError_t e = hipStreamCreateWithPriority(&g->comm_stream, hipStreamNonBlocking, prio_high);
    for (hipEvent_t *ev : {&g->inputs_final, &g->edges_done})
        if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    for (hipEvent_t *ev : {&g->t0, &g->t1})
        if (e == hipSuccess) e = hipEventCreate(ev);
    if (g->left >= 0 || g->right >= 0) {
        for (hipStream_t *st : {&g->col_stream[0], &g->col_stream[1]})
            if (e == hipSuccess) e = hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio_high);
        for (hipEvent_t *ev : {&g->halos_in, &g->col_done[0], &g->col_done[1]})
            if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    }
    if (g->external) {
        // the host is the transport: its messages instead of the column buffers and the exchange engine
        for (hipEvent_t *ev : {&g->packed, &g->unpacked})
            if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
        if (e != hipSuccess) return amt_fail(AMT_ERR_HIP, "amt_grid_create: %s", hipGetErrorString(e));
        return external_buffers(g);
    }
    const size_t from_right = column_bytes(dom, AMT_HALO_RIGHT), from_left = column_bytes(dom, AMT_HALO_LEFT);
    if (e == hipSuccess && g->left >= 0) e = hipMalloc(&g->to_left, from_right);         // what my left neighbour receives from its right
    if (e == hipSuccess && g->right >= 0) e = hipMalloc(&g->from_right, from_right);
    if (e == hipSuccess && g->right >= 0) e = hipMalloc(&g->to_right, from_left);
    if (e == hipSuccess && g->left >= 0) e = hipMalloc(&g->from_left, from_left);
    if (e != hipSuccess) return amt_fail(e == hipErrorOutOfMemory ? AMT_ERR_ALLOC : AMT_ERR_HIP, "amt_grid_create: %s", hipGetErrorString(e));
    // the segments of one exchange.  Per pair of ranks the order of the sends is the order of the receives on the other side.
    const size_t es = (size_t)dom->dtype_bytes, idim = dom->ime - dom->ims + 1, kdim = dom->kme - dom->kms + 1;
    std::vector<AmtSeg> sends, recvs;
    auto rows = [&](std::vector<AmtSeg> &segs, const AmtHaloFields &list, int j, int peer) {       // whole memory rows j, in place
        for (int q = 0; q < list.n; ++q) {
            const int f = list.field[q];
            segs.push_back(AmtSeg{static_cast<char *>(dom->field[f]) + (size_t)amt_halo_at(*dom, f, dom->ims, j) * es,
                                  (size_t)amt_halo_levels(f, kdim) * idim * es, peer});
        }
    };
    if (g->below >= 0) rows(sends, amt_halo_sent(AMT_HALO_BELOW), ec.jlo, g->below);
    if (g->above >= 0) rows(sends, amt_halo_sent(AMT_HALO_ABOVE), ec.jhi, g->above);
    if (g->left >= 0) sends.push_back(AmtSeg{g->to_left, from_right, g->left});
    if (g->right >= 0) sends.push_back(AmtSeg{g->to_right, from_left, g->right});
    if (g->above >= 0) rows(recvs, amt_halo_recv(AMT_HALO_ABOVE), ec.jhi + 1, g->above);
    if (g->below >= 0) rows(recvs, amt_halo_recv(AMT_HALO_BELOW), ec.jlo - 1, g->below);
    if (g->right >= 0) recvs.push_back(AmtSeg{g->from_right, from_right, g->right});
    if (g->left >= 0) recvs.push_back(AmtSeg{g->from_left, from_left, g->left});
    return amt_exchange_create(&g->xchg, transport, rank, world, unique_id, dom->device, sends.data(), (int)sends.size(),
                               recvs.data(), (int)recvs.size(), loop_i || loop_j);
}

int grid_exchange_only(amt_grid *g)
{
    if (const int no = not_for_external(g, "amt_grid_exchange")) return no;
    DeviceScope scope(g->dom->device);
    AMT_HIP(hipEventRecord(g->inputs_final, g->dom->stream));
    AMT_HIP(hipStreamWaitEvent(g->comm_stream, g->inputs_final, 0));
    int rc = g->self_wrap ? amt_cyclic_refresh_domain("amt_grid_exchange", g->dom, g->self_wrap, 1) : AMT_OK;   // on the domain's stream
    if (rc == AMT_OK) rc = grid_pack(g, g->comm_stream);
    if (rc == AMT_OK) rc = amt_exchange_enqueue(g->xchg, g->comm_stream, true);
    if (rc == AMT_OK) rc = grid_unpack(g, g->comm_stream);
    if (rc == AMT_OK) rc = amt_exchange_enqueue_release(g->xchg, g->comm_stream);
    if (rc) return rc;
    AMT_HIP(hipEventRecord(g->edges_done, g->comm_stream));
    AMT_HIP(hipStreamWaitEvent(g->dom->stream, g->edges_done, 0));
    return AMT_OK;
}

int grid_step(amt_grid *g, int n_sweeps)
{
    if (const int no = not_for_external(g, "amt_grid_step")) return no;
    if (const int no = uv_refused(g, "amt_grid_step")) return no;
    DeviceScope scope(g->dom->device);
    return g->dom->dtype_bytes == 8 ? grid_step_t<double>(g, n_sweeps) : grid_step_t<float>(g, n_sweeps);
}

int grid_step_timed(amt_grid *g, int n_sweeps, float *ms_total)
{
    if (const int no = not_for_external(g, "amt_grid_step_timed")) return no;
    if (const int no = uv_refused(g, "amt_grid_step_timed")) return no;
    DeviceScope scope(g->dom->device);
    AMT_HIP(hipEventRecord(g->t0, g->dom->stream));
    int rc = grid_step(g, n_sweeps);
    if (rc) return rc;
    AMT_HIP(hipEventRecord(g->t1, g->dom->stream));
    AMT_HIP(hipEventSynchronize(g->t1));
    float ms = 0.f;
    AMT_HIP(hipEventElapsedTime(&ms, g->t0, g->t1));
    if (ms_total) *ms_total = ms;
    return amt_exchange_check(g->xchg);          // the timed sweeps are complete: report a wait that gave up inside them
}

int grid_sync(amt_grid *g)
{
    DeviceScope scope(g->dom->device);
    AMT_HIP(hipStreamSynchronize(g->comm_stream));
    AMT_HIP(hipStreamSynchronize(g->dom->stream));
    return amt_exchange_check(g->xchg);          // a device-side wait that gave up (IPC) is reported here
}

long grid_halo_bytes(const amt_grid *g)
{
    size_t sent = 0, received = 0;
    amt_exchange_bytes(g->xchg, &sent, &received);
    for (int m = 0; m < g->n_msg; ++m) { sent += g->msg[m].send_bytes; received += g->msg[m].recv_bytes; }      // host-owned exchange
    return (long)(sent + received);
}

const char *grid_transport(const amt_grid *g)
{
    if (g->external) return g->n_msg ? "external" : "none";
    if (!amt_exchange_active(g->xchg)) return "none";
    return amt_exchange_transport(g->xchg) == AMT_XCHG_IPC ? "ipc" : "rccl";
}

// max over the ranks of *x (in place); also a barrier: every rank's streams are drained first and nobody returns before all
// have contributed.  For reporting only (the max-over-ranks sweep time of a host without MPI) -- the sweep itself uses no
// collective.
int grid_max(amt_grid *g, double *x)
{
    if (g->external) return amt_fail(AMT_ERR_INVALID_ARG, "amt_grid_max / amt_grid_barrier: the host owns this handle's communicator (AMT_SLAB_TRANSPORT_EXTERNAL)");
    DeviceScope scope(g->dom->device);
    AMT_HIP(hipStreamSynchronize(g->dom->stream));
    AMT_HIP(hipStreamSynchronize(g->comm_stream));
    return amt_exchange_max(g->xchg, x, g->comm_stream);
}

template <typename H>
int create_handle(H **out, amt_domain *dom, int ri, int rj, int pi, int pj, const void *unique_id, int flags, bool loop_i, bool loop_j, amt_grid *(*grid_of)(H *))
{
    if (!out) return amt_fail(AMT_ERR_INVALID_ARG, "null out pointer");
    *out = nullptr;
    H *h = new (std::nothrow) H;
    if (!h) return amt_fail(AMT_ERR_ALLOC, "host allocation failed");
    const int rc = grid_setup(grid_of(h), dom, ri, rj, pi, pj, unique_id, flags, loop_i, loop_j);
    if (rc) {
        const std::string keep = amt_last_error();       // the teardown must not lose the diagnosis
        if (grid_of(h)->dom) grid_teardown(grid_of(h));
        delete h;
        return amt_fail(rc, "%s", keep.c_str());
    }
    *out = h;
    return AMT_OK;
}
amt_grid *self(amt_grid *g) { return g; }
amt_grid *inner(amt_slab *s) { return &s->g; }
}  // namespace

// ---------------------------------------------------------------------------
// amt_grid_*: patch (ri, rj) of pi x pj; rank = rj * pi + ri
// ---------------------------------------------------------------------------
extern "C" int amt_grid_create(amt_grid **out, amt_domain *dom, int ri, int rj, int pi, int pj, const void *unique_id, int flags)
{
    const bool loop = (flags & AMT_SLAB_LOOPBACK) != 0;
    return create_handle<amt_grid>(out, dom, ri, rj, pi, pj, unique_id, flags, loop, loop, self);
}
extern "C" int amt_grid_destroy(amt_grid *g)
{
    if (!g) return AMT_OK;
    grid_teardown(g);
    delete g;
    return AMT_OK;
}
extern "C" int amt_grid_exchange(amt_grid *g) { return g ? grid_exchange_only(g) : amt_fail(AMT_ERR_INVALID_ARG, "null grid"); }
extern "C" int amt_grid_step(amt_grid *g, int n) { return g && n >= 0 ? grid_step(g, n) : amt_fail(AMT_ERR_INVALID_ARG, "bad step argument"); }
extern "C" int amt_grid_step_timed(amt_grid *g, int n, float *ms) { return g && n >= 0 ? grid_step_timed(g, n, ms) : amt_fail(AMT_ERR_INVALID_ARG, "bad step argument"); }
extern "C" int amt_grid_sync(amt_grid *g) { return g ? grid_sync(g) : amt_fail(AMT_ERR_INVALID_ARG, "null grid"); }
extern "C" long amt_grid_halo_bytes(const amt_grid *g) { return g ? grid_halo_bytes(g) : 0; }
extern "C" const char *amt_grid_transport(const amt_grid *g) { return g ? grid_transport(g) : "none"; }
extern "C" int amt_grid_comm_info(const amt_grid *g, int *rank, int *world) { return g ? amt_exchange_info(g->xchg, rank, world) : amt_fail(AMT_ERR_INVALID_ARG, "null grid"); }
extern "C" int amt_grid_max(amt_grid *g, double *x) { return g && x ? grid_max(g, x) : amt_fail(AMT_ERR_INVALID_ARG, "bad reduction argument"); }
extern "C" int amt_grid_barrier(amt_grid *g) { double zero = 0.0; return amt_grid_max(g, &zero); }
extern "C" int amt_grid_set_skew_us(amt_grid *g, int microseconds)
{
    if (!g || microseconds < 0) return amt_fail(AMT_ERR_INVALID_ARG, "bad skew argument");
    g->skew_us = microseconds;
    amt_exchange_set_skew_us(g->xchg, microseconds);      // the IPC transport carries it inside its waiting kernel
    return AMT_OK;
}

extern "C" int amt_grid_halo_messages(amt_grid *g, amt_halo_message *out, int cap, int *n) { return g ? external_messages(g, out, cap, n) : amt_fail(AMT_ERR_INVALID_ARG, "null grid"); }
extern "C" int amt_grid_step_begin(amt_grid *g) { return g ? external_begin(g) : amt_fail(AMT_ERR_INVALID_ARG, "null grid"); }
extern "C" int amt_grid_halo_wait(amt_grid *g) { return g ? external_wait(g) : amt_fail(AMT_ERR_INVALID_ARG, "null grid"); }
extern "C" int amt_grid_step_end(amt_grid *g) { return g ? external_end(g) : amt_fail(AMT_ERR_INVALID_ARG, "null grid"); }
extern "C" int amt_grid_halo_pack(amt_grid *g) { return g ? external_pack_only(g, false) : amt_fail(AMT_ERR_INVALID_ARG, "null grid"); }
extern "C" int amt_grid_halo_unpack(amt_grid *g) { return g ? external_pack_only(g, true) : amt_fail(AMT_ERR_INVALID_ARG, "null grid"); }

// The planner: the message list of patch (ri, rj) of pi x pj from the shape alone.  Nothing of the device is touched.
extern "C" int amt_halo_plan(AMT_SHAPE_SIG, int ri, int rj, int pi, int pj, int flags, amt_halo_message *out, int cap, int *n)
{
    if (!n || cap < 0 || (cap > 0 && !out)) return amt_fail(AMT_ERR_INVALID_ARG, "amt_halo_plan: bad argument");
    if (dtype_bytes != 4 && dtype_bytes != 8) return amt_fail(AMT_ERR_INVALID_ARG, "amt_halo_plan: dtype_bytes is 4 or 8");
    if (ime < ims || jme < jms || kme < kms) return amt_fail(AMT_ERR_PRECONDITION, "amt_halo_plan: empty memory extents");
    amt_domain d;
    amt_domain_set_shape(&d, AMT_SHAPE_ARGS);
    amt_grid g;
    const int rc = grid_topology(&g, &d, ri, rj, pi, pj, true, flags | AMT_SLAB_TRANSPORT_EXTERNAL, false, false);
    if (rc) return rc;
    amt_halo_message msg[4];
    *n = halo_plan(&g, msg);
    if (*n > cap) return amt_fail(AMT_ERR_INVALID_ARG, "amt_halo_plan: %d messages, room for %d", *n, cap);
    for (int m = 0; m < *n; ++m) out[m] = msg[m];
    return AMT_OK;
}

// ---------------------------------------------------------------------------
// amt_slab_*: the pi = 1 case (rank = rj, world = pj); loopback loops j only
// ---------------------------------------------------------------------------
extern "C" int amt_slab_create(amt_slab **out, amt_domain *dom, int rank, int world, const void *unique_id, int flags)
{
    if (world < 1 || rank < 0 || rank >= world) return amt_fail(AMT_ERR_INVALID_ARG, "bad slab argument");
    const bool loop = (flags & AMT_SLAB_LOOPBACK) != 0;
    if (loop && world != 1) return amt_fail(AMT_ERR_INVALID_ARG, "AMT_SLAB_LOOPBACK is a one-rank test mode");
    return create_handle<amt_slab>(out, dom, 0, rank, 1, world, unique_id, flags, false, loop, inner);
}
extern "C" int amt_slab_destroy(amt_slab *s)
{
    if (!s) return AMT_OK;
    grid_teardown(&s->g);
    delete s;
    return AMT_OK;
}
extern "C" int amt_slab_halo_messages(amt_slab *s, amt_halo_message *out, int cap, int *n) { return s ? external_messages(&s->g, out, cap, n) : amt_fail(AMT_ERR_INVALID_ARG, "null slab"); }
extern "C" int amt_slab_step_begin(amt_slab *s) { return s ? external_begin(&s->g) : amt_fail(AMT_ERR_INVALID_ARG, "null slab"); }
extern "C" int amt_slab_halo_wait(amt_slab *s) { return s ? external_wait(&s->g) : amt_fail(AMT_ERR_INVALID_ARG, "null slab"); }
extern "C" int amt_slab_step_end(amt_slab *s) { return s ? external_end(&s->g) : amt_fail(AMT_ERR_INVALID_ARG, "null slab"); }
extern "C" int amt_slab_halo_pack(amt_slab *s) { return s ? external_pack_only(&s->g, false) : amt_fail(AMT_ERR_INVALID_ARG, "null slab"); }
extern "C" int amt_slab_halo_unpack(amt_slab *s) { return s ? external_pack_only(&s->g, true) : amt_fail(AMT_ERR_INVALID_ARG, "null slab"); }
extern "C" int amt_slab_exchange(amt_slab *s) { return s ? grid_exchange_only(&s->g) : amt_fail(AMT_ERR_INVALID_ARG, "null slab"); }
extern "C" int amt_slab_step(amt_slab *s, int n) { return s && n >= 0 ? grid_step(&s->g, n) : amt_fail(AMT_ERR_INVALID_ARG, "bad step argument"); }
extern "C" int amt_slab_step_timed(amt_slab *s, int n, float *ms) { return s && n >= 0 ? grid_step_timed(&s->g, n, ms) : amt_fail(AMT_ERR_INVALID_ARG, "bad step argument"); }
extern "C" int amt_slab_sync(amt_slab *s) { return s ? grid_sync(&s->g) : amt_fail(AMT_ERR_INVALID_ARG, "null slab"); }
extern "C" long amt_slab_halo_bytes(const amt_slab *s) { return s ? grid_halo_bytes(&s->g) : 0; }
extern "C" const char *amt_slab_transport(const amt_slab *s) { return s ? grid_transport(&s->g) : "none"; }
extern "C" const char *amt_slab_pull_mode(const amt_slab *s) { return s ? amt_exchange_pull_mode(s->g.xchg) : ""; }
extern "C" const char *amt_grid_pull_mode(const amt_grid *g) { return g ? amt_exchange_pull_mode(g->xchg) : ""; }
extern "C" int amt_slab_comm_info(const amt_slab *s, int *rank, int *world) { return s ? amt_exchange_info(s->g.xchg, rank, world) : amt_fail(AMT_ERR_INVALID_ARG, "null slab"); }
extern "C" int amt_slab_max(amt_slab *s, double *x) { return s && x ? grid_max(&s->g, x) : amt_fail(AMT_ERR_INVALID_ARG, "bad reduction argument"); }
extern "C" int amt_slab_barrier(amt_slab *s) { double zero = 0.0; return amt_slab_max(s, &zero); }
extern "C" int amt_slab_set_skew_us(amt_slab *s, int microseconds)
{
    if (!s) return amt_fail(AMT_ERR_INVALID_ARG, "bad skew argument");
    return amt_grid_set_skew_us(&s->g, microseconds);
}
