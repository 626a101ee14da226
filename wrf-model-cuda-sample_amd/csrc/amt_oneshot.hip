// amt_oneshot.hip -- the one-shot host drop-in amt_advance_mu_t_f32/_f64: host arrays in, host
// arrays out (the job of the reference's CUDA wrapper, advance_mu_t_no_async.cu:178-423: alloc,
// H2D, launch, D2H, free), streamed.
#include "amt_halo.h"
#include "amt_oneshot_plan.h"
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>
#include <sys/syscall.h>
#include <unistd.h>

namespace {
// The arrays a thread may keep on the device between calls (HostWorkspace::Kept): first the cached inputs, then the
// deferrable outputs -- exactly the fields the routine assigns (amt_internal.h's table).  Rank and name of an entry are its field's.
constexpr int kKeepField[] = {AMT_F_WW_1, AMT_F_U_1, AMT_F_V_1, AMT_F_T_1, AMT_F_FT, AMT_F_MUT, AMT_F_MUU, AMT_F_MUV, AMT_F_MU_TEND,
                              AMT_F_MSFUY, AMT_F_MSFVX_INV, AMT_F_MSFTX, AMT_F_MSFTY, AMT_F_DNW, AMT_F_FNM, AMT_F_FNP, AMT_F_RDNW,
                              /* deferred: */ AMT_F_WW, AMT_F_T, AMT_F_T_AVE, AMT_F_MU, AMT_F_MUAVE, AMT_F_MUTS, AMT_F_MUDF};
constexpr int NKEEP = sizeof kKeepField / sizeof *kKeepField;
constexpr int NCACHE = 17;                                    // the first NCACHE entries are the cached inputs
constexpr bool amt_keep_table_ok()
{
    int nout = 0, nwrong = 0;
    for (int f = 0; f < AMT_F_COUNT; ++f) nout += kAmtField[f].out;
    for (int r = 0; r < NKEEP; ++r) nwrong += kAmtField[kKeepField[r]].out != (r >= NCACHE);
    return nwrong == 0 && NKEEP - NCACHE == nout;
}
static_assert(amt_keep_table_ok(), "kKeepField: NCACHE read-only inputs, then every field the routine assigns");
inline int amt_keep_rank(int r) { return amt_field_rank(kKeepField[r]); }
inline const char *amt_keep_name(int r) { return amt_field_name(kKeepField[r]); }

// The window's cells of an array with memory rows of idim elements (and kdim levels): columns i0 .. i0+ni-1, levels k1 .. k1+nk-1.
struct WindowCells {
    size_t es = 0;                                            // element size
    long idim = 0, kdim = 0, i0 = 0, ni = 0, k1 = 0, nk = 0;
};
// nj rows of those cells of a rank-3 or rank-2 array, device to host: row `drow` of the device array lands in row `hrow` of the host array
hipError_t amt_window_down(const WindowCells &g, int rank, void *host, size_t hrow, const void *dev, size_t drow, size_t nj, hipStream_t st)
{
    const size_t pitch = (size_t)g.idim * g.es;
    if (rank == 2)
        return hipMemcpy2DAsync(static_cast<char *>(host) + hrow * pitch + (size_t)g.i0 * g.es, pitch,
                                static_cast<const char *>(dev) + drow * pitch + (size_t)g.i0 * g.es, pitch, (size_t)g.ni * g.es, nj,
                                hipMemcpyDeviceToHost, st);
    hipMemcpy3DParms cp;
    memset(&cp, 0, sizeof cp);
    cp.srcPtr = make_hipPitchedPtr(const_cast<void *>(dev), pitch, (size_t)g.idim, (size_t)g.kdim);
    cp.dstPtr = make_hipPitchedPtr(host, pitch, (size_t)g.idim, (size_t)g.kdim);
    cp.srcPos = make_hipPos((size_t)g.i0 * g.es, (size_t)g.k1, drow);
    cp.dstPos = make_hipPos((size_t)g.i0 * g.es, (size_t)g.k1, hrow);
    cp.extent = make_hipExtent((size_t)g.ni * g.es, (size_t)g.nk, nj);
    cp.kind = hipMemcpyDeviceToHost;
    return hipMemcpy3DAsync(&cp, st);
}

// What a one-shot call needs on the device besides the data: three streams, six events and a
// buffer arena.  Creating and destroying them costs ~10 ms per call -- more than the whole call
// at WRF patch sizes -- so each host thread keeps its own set between calls (per thread: WRF
// calls advance_mu_t from OpenMP tile threads).  amt_host_release() frees the calling thread's.
struct HostWorkspace {
    int device = -1;
    hipStream_t up = nullptr, comp = nullptr, down = nullptr;
    hipEvent_t uploaded[2] = {}, computed[2] = {}, drained[2] = {};
    char *arena = nullptr;
    size_t arena_size = 0;
    char *stage = nullptr;                                   // page-locked host staging (packed calls)
    size_t stage_size = 0;
    static constexpr size_t keep_limit = (size_t)1 << 30;   // larger arenas are not kept between calls

    // Arrays that stay on the device between calls of this thread, as whole-window copies keyed on the host
    // pointers and every extent:
    //  * residency cache (amt_host_cache_enable): the inputs that are constant over the acoustic sub-steps of a
    //    Runge-Kutta stage -- the five 3-D ones ww_1, u_1, v_1, t_1, ft, and (r04) the eight 2-D and four 1-D ones
    //    mut, muu, muv, mu_tend, msfuy, msfvx_inv, msftx, msfty, dnw, fnm, fnp, rdnw -- go up again only after
    //    amt_host_invalidate;
    //  * deferred outputs (amt_host_defer): ww, t, t_ave, mu, muave, muts, mudf stay on the device after the call;
    //    the device copy is the truth until amt_host_fetch brings the window's cells down (or amt_host_invalidate
    //    says the host array was rewritten and is the truth again); the in/out ones (level 1 of ww, t, mu) go up
    //    only while the device copy is not valid.
    struct Kept {
        bool enabled = false, check = false;                  // cache on; checksum / canary debug mode
        bool defer_all = false;
        const void *defer_ptr[16] = {};
        int ndefer = 0;
        char *buf[NKEEP] = {};
        size_t bytes[NKEEP] = {};
        bool active[NKEEP] = {};                              // kept by the calls of the current key
        bool valid[NKEEP] = {};                               // the device copy is current
        bool stale[NKEEP] = {};                               // deferred: the device copy is NEWER than the host array
        bool poisoned[NKEEP] = {};                            // deferred in/out: a FAILED call may have advanced part of the device copy
        uint64_t sum[NKEEP] = {};                             // check mode: checksum of what was uploaded / of the canary
        const void *host[NKEEP] = {};
        int key[16] = {};                                     // element size, extents, window, device
        // geometry of the window the copies cover (amt_host_fetch works from it)
        WindowCells cells;
        long j_start = 0, j_end = 0, jms = 0;
        bool deferred(const void *ptr) const
        {
            if (defer_all) return true;
            for (int q = 0; q < ndefer; ++q)
                if (defer_ptr[q] == ptr) return true;
            return false;
        }
        bool any_stale() const
        {
            for (int r = 0; r < NKEEP; ++r)
                if (stale[r]) return true;
            return false;
        }
        void drop()
        {
            for (int r = 0; r < NKEEP; ++r) {
                if (buf[r]) (void)hipFree(buf[r]);
                buf[r] = nullptr; bytes[r] = 0; active[r] = valid[r] = stale[r] = poisoned[r] = false; host[r] = nullptr; sum[r] = 0;
            }
        }
    } res;

    void release()
    {
        if (device < 0) return;
        int prev = -1;
        const bool sw = hipGetDevice(&prev) == hipSuccess && prev != device && hipSetDevice(device) == hipSuccess;
        for (hipStream_t st : {up, comp, down})
            if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
        for (int s = 0; s < 2; ++s)
            for (hipEvent_t e : {uploaded[s], computed[s], drained[s]})
                if (e) (void)hipEventDestroy(e);
        if (arena) (void)hipFree(arena);
        if (stage) (void)hipHostFree(stage);
        Kept keep = res;                                     // the thread's settings outlive its buffers
        res.drop();
        if (sw) (void)hipSetDevice(prev);
        *this = HostWorkspace();
        res.enabled = keep.enabled; res.check = keep.check; res.defer_all = keep.defer_all; res.ndefer = keep.ndefer;
        memcpy(res.defer_ptr, keep.defer_ptr, sizeof res.defer_ptr);
    }
    // A worker thread's workspace is freed when the thread ends.  The main thread's destructor
    // runs at process exit only, possibly from a signal path with a HIP call on the stack: leave
    // that one to the operating system.
    ~HostWorkspace()
    {
        if ((long)syscall(SYS_gettid) != (long)getpid()) release();
    }

    hipError_t prepare(int dev, size_t bytes)
    {
        if (device != dev) {
            release();
            device = dev;
            hipError_t e = hipSuccess;
            for (hipStream_t *st : {&up, &comp, &down})
                if (e == hipSuccess) e = hipStreamCreateWithFlags(st, hipStreamNonBlocking);
            for (int s = 0; s < 2; ++s)
                for (hipEvent_t *ev : {&uploaded[s], &computed[s], &drained[s]})
                    if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
            if (e != hipSuccess) { release(); return e; }
        }
        if (bytes > arena_size) {
            if (arena) (void)hipFree(arena);
            arena = nullptr;
            arena_size = 0;
            hipError_t e = hipMalloc((void **)&arena, bytes);
            if (e != hipSuccess) { (void)hipGetLastError(); arena = nullptr; return e; }
            arena_size = bytes;
        }
        return hipSuccess;
    }
    hipError_t stage_reserve(size_t bytes)
    {
        if (bytes <= stage_size) return hipSuccess;
        if (stage) (void)hipHostFree(stage);
        stage = nullptr;
        stage_size = 0;
        hipError_t e = hipHostMalloc((void **)&stage, bytes, hipHostMallocDefault);
        if (e != hipSuccess) { (void)hipGetLastError(); stage = nullptr; return e; }
        stage_size = bytes;
        return hipSuccess;
    }
    // end of a call: nothing may still be in flight towards the caller's arrays
    void finish()
    {
        for (hipStream_t st : {up, comp, down})
            if (st) (void)hipStreamSynchronize(st);
        if (arena_size > keep_limit) {
            (void)hipFree(arena);
            arena = nullptr;
            arena_size = 0;
        }
    }
};
thread_local HostWorkspace tl_workspace;
thread_local long tl_oneshot_calls = 0;                       // one-shot calls of this thread, either precision (test hook below)
struct WorkspaceScope {
    HostWorkspace &ws;
    ~WorkspaceScope() { ws.finish(); }
};
}  // namespace

// 64-bit checksum of a byte range (check mode only: it reads the whole range; byte-wise loads of the head and tail,
// memcpy-based word loads in between: the range need not be 8-byte aligned)
static uint64_t amt_host_sum(const void *p, size_t bytes)
{
    const unsigned char *q = static_cast<const unsigned char *>(p);
    uint64_t a = 0x9e3779b97f4a7c15ull, b = 0;
    size_t i = 0;
    for (; i + 8 <= bytes; i += 8) {
        uint64_t w;
        memcpy(&w, q + i, 8);
        a = (a ^ w) * 0x100000001b3ull;
        b += w + (a >> 29);
    }
    for (; i < bytes; ++i) a = (a ^ q[i]) * 0x100000001b3ull;
    return a ^ (b << 1);
}

namespace {
// The window's cells of kept field r as a list of (host address, device address, bytes) runs is never built: the
// strided copies below walk it.  dir > 0: device -> host (fetch); the canary and the checksum walk the host side.
const uint64_t kCanary64 = 0x7ff8dead0badc0deull;             // a quiet NaN in fp64
const uint32_t kCanary32 = 0x7fc0dead;                        // a quiet NaN in fp32

// bring the window's cells of kept field r down to its host array (the strided copies of a normal call's download)
hipError_t amt_keep_fetch(HostWorkspace &ws, int r)
{
    HostWorkspace::Kept &k = ws.res;
    if (!k.buf[r] || !k.stale[r]) return hipSuccess;
    void *host = const_cast<void *>(k.host[r]);
    const size_t nj = (size_t)(k.j_end - k.j_start + 1), hrow = (size_t)(k.j_start - k.jms);
    if (amt_keep_rank(r) == 3 && k.cells.nk <= 0) { k.stale[r] = false; return hipSuccess; }
    hipError_t e = amt_window_down(k.cells, amt_keep_rank(r), host, hrow, k.buf[r], 1, nj, ws.down);
    if (e == hipSuccess) e = hipStreamSynchronize(ws.down);
    if (e == hipSuccess) k.stale[r] = false;
    return e;
}

// check mode: the window's cells of a deferred host array are overwritten with NaN canaries after the call (a consumer
// that reads the stale host array computes NaNs instead of silently using old values) -- or, with fill = false, checked
// to still hold them (a host write without amt_host_invalidate would otherwise be lost)
bool amt_keep_canary(HostWorkspace::Kept &k, int r, bool fill)
{
    char *host = static_cast<char *>(const_cast<void *>(k.host[r]));
    const WindowCells &g = k.cells;
    const bool r3 = amt_keep_rank(r) == 3;
    const size_t es = g.es, idim = (size_t)g.idim, levels = r3 ? (size_t)g.nk : 1, kd = r3 ? (size_t)g.kdim : 1, k1 = r3 ? (size_t)g.k1 : 0;
    for (long j = k.j_start; j <= k.j_end; ++j)
        for (size_t l = 0; l < levels; ++l) {
            char *row = host + ((((size_t)(j - k.jms)) * kd + k1 + l) * idim + (size_t)g.i0) * es;
            for (long i = 0; i < g.ni; ++i) {
                if (fill) {
                    if (es == 8) memcpy(row + (size_t)i * 8, &kCanary64, 8);
                    else memcpy(row + (size_t)i * 4, &kCanary32, 4);
                } else if (memcmp(row + (size_t)i * es, es == 8 ? (const void *)&kCanary64 : (const void *)&kCanary32, es) != 0) {
                    return false;
                }
            }
        }
    return true;
}

// everything the device holds that the host does not: brought down before the copies are given up
int amt_keep_flush(HostWorkspace &ws)
{
    if (ws.device < 0 || !ws.res.any_stale()) return AMT_OK;
    DeviceScope dev(ws.device);
    for (int r = 0; r < NKEEP; ++r) AMT_HIP(amt_keep_fetch(ws, r));
    return AMT_OK;
}
}  // namespace

static int host_release_local()
{
    const int rc = amt_keep_flush(tl_workspace);              // what only the device holds comes down before the buffers go
    tl_workspace.release();
    return rc;
}

static int host_cache_enable_local(int on)
{
    HostWorkspace &ws = tl_workspace;
    if (!on && ws.res.enabled && ws.device >= 0) {
        DeviceScope dev(ws.device);
        for (hipStream_t st : {ws.up, ws.comp, ws.down})
            if (st) (void)hipStreamSynchronize(st);
        for (int r = 0; r < NCACHE; ++r) {        // the cached inputs go; deferred outputs are another setting
            if (ws.res.buf[r]) (void)hipFree(ws.res.buf[r]);
            ws.res.buf[r] = nullptr; ws.res.bytes[r] = 0; ws.res.active[r] = ws.res.valid[r] = false; ws.res.host[r] = nullptr;
        }
    }
    ws.res.enabled = on != 0;
    return AMT_OK;
}

static int host_cache_check_local(int on)
{
    tl_workspace.res.check = on != 0;
    return AMT_OK;
}

static int host_invalidate_local(const void *host_ptr)
{
    // "the host array was rewritten": a cached input goes up again with the next call; for a deferred output the HOST
    // is the truth again (whatever the device still held for it is given up)
    HostWorkspace::Kept &r = tl_workspace.res;
    for (int q = 0; q < NKEEP; ++q)
        if (!host_ptr || r.host[q] == host_ptr) { r.valid[q] = false; r.stale[q] = false; r.poisoned[q] = false; }
    return AMT_OK;                                            // an array that is not kept is uploaded anyway
}

static int host_defer_local(const void *host_ptr, int on)
{
    HostWorkspace &ws = tl_workspace;
    HostWorkspace::Kept &k = ws.res;
    if (on) {
        if (!host_ptr) { k.defer_all = true; return AMT_OK; }
        if (k.deferred(host_ptr)) return AMT_OK;
        if (k.ndefer >= 16) return amt_fail(AMT_ERR_INVALID_ARG, "amt_host_defer: more than 16 deferred arrays");
        k.defer_ptr[k.ndefer++] = host_ptr;
        return AMT_OK;
    }
    // off: what the device holds for it comes down first, then the array is an ordinary output again
    for (int r = NCACHE; r < NKEEP; ++r)
        if (k.buf[r] && (!host_ptr || k.host[r] == host_ptr)) {
            if (k.stale[r] && ws.device >= 0) {
                DeviceScope dev(ws.device);
                AMT_HIP(amt_keep_fetch(ws, r));
            }
            k.valid[r] = false;                               // the next call uploads from the host again
        }
    if (!host_ptr) { k.defer_all = false; k.ndefer = 0; return AMT_OK; }
    if (k.defer_all) return amt_fail(AMT_ERR_INVALID_ARG, "amt_host_defer(ptr, 0) after amt_host_defer(NULL, 1): turn all off with NULL");
    for (int q = 0; q < k.ndefer; ++q)
        if (k.defer_ptr[q] == host_ptr) { k.defer_ptr[q] = k.defer_ptr[--k.ndefer]; break; }
    return AMT_OK;
}

static int host_fetch_local(const void *host_ptr)
{
    HostWorkspace &ws = tl_workspace;
    if (ws.device < 0) return AMT_OK;
    DeviceScope dev(ws.device);
    for (int r = NCACHE; r < NKEEP; ++r)
        if ((!host_ptr || ws.res.host[r] == host_ptr) && ws.res.poisoned[r])
            return amt_fail(AMT_ERR_PRECONDITION, "deferred output %s: its device copy is undefined since a call failed part-way (some rows may be "
                            "a sub-step ahead); nothing is brought down -- amt_host_invalidate(ptr) makes the host array the truth again", amt_keep_name(r));
    for (int r = NCACHE; r < NKEEP; ++r)
        if (!host_ptr || ws.res.host[r] == host_ptr) AMT_HIP(amt_keep_fetch(ws, r));
    return AMT_OK;
}

static int host_stale_local(const void *host_ptr)
{
    const HostWorkspace::Kept &k = tl_workspace.res;
    for (int r = NCACHE; r < NKEEP; ++r)
        if (k.poisoned[r] && (!host_ptr || k.host[r] == host_ptr)) return -1;      // undefined after a failed call
    for (int r = NCACHE; r < NKEEP; ++r)
        if (k.stale[r] && (!host_ptr || k.host[r] == host_ptr)) return 1;
    return 0;
}

// One-shot call = upload, kernel, download.  Three regimes, chosen per call:
//  * streamed (3-D arrays page-locked by the caller -- amt_host_pin / hipHostRegister /
//    hipHostMalloc, once, like the reference driver's cudaHostAlloc, advance_mu_t_driver.cu:
//    97-167): the window's j rows are cut into chunks; chunk c runs
//      H2D (its rows + one halo row each side of the five arrays the stencil reads across rows)
//      -> kernel -> D2H (the window's cells of ww, t, t_ave)
//    through device buffer set c % 2, the three stages on an upload, a compute and a download
//    stream chained by events, so that both directions of the host link stay busy;
//  * streamed with a download thread (3-D arrays pageable, more than one chunk): a copy from or
//    to pageable memory blocks its host thread, so the downloads are issued by a second thread
//    (two threads drive both directions of the link at full rate, one cannot; pinning inside
//    the call costs more than it saves: 61 vs 41 ms at 512x60x512 fp64);
//  * packed (pageable and small -- WRF patch sizes): every blocking copy costs ~0.2 ms, 29 of
//    them more than everything else, so the arrays are gathered into a page-locked staging
//    buffer that mirrors the device arena and cross the link in one copy each way.
// The 2-D and 1-D arrays (1/NK of the data) go up once before the first chunk and come down once
// after the last, packed when they are pageable.  Chunks are legal because a row's outputs depend
// on other rows' INPUTS only.  The reference does one synchronous piece per call and allocates
// and frees everything around it (advance_mu_t_no_async.cu:178-306,366-423).
static bool amt_is_pinned(const void *ptr)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

extern "C" int amt_host_pin(void *ptr, size_t bytes)
{
    if (!ptr) return amt_fail(AMT_ERR_INVALID_ARG, "null pointer");
    AMT_HIP(hipHostRegister(ptr, bytes, hipHostRegisterPortable));       // page-locked for every device (amt_host_set_devices)
    return AMT_OK;
}

extern "C" int amt_host_unpin(void *ptr)
{
    if (!ptr) return amt_fail(AMT_ERR_INVALID_ARG, "null pointer");
    AMT_HIP(hipHostUnregister(ptr));
    return AMT_OK;
}

namespace {
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// A call that fails after its first kernel went out leaves the deferred in/out copies (level 1 of ww, t, mu: advanced in place,
// chunk by chunk) partly a sub-step ahead: a retry would apply the sub-step twice to those rows and a fetch would bring a
// half-advanced state down.  They are marked undefined.
struct FailGuard {
    HostWorkspace::Kept &k;
    bool launched = false, ok = false;
    ~FailGuard()
    {
        if (!launched || ok) return;
        for (int r = NCACHE; r < NKEEP; ++r)
            if (k.active[r] && (k.stale[r] || k.valid[r])) { k.valid[r] = k.stale[r] = false; k.poisoned[r] = true; }
    }
};

// download thread: takes chunks in order as the main thread reports them launched, reports them drained so that their buffer
// set can be reused
struct Downloader {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    int n_launched = 0, n_drained = 0;
    bool stop = false;
    hipError_t err = hipSuccess;
    // false: no thread to be had
    bool start(int device, int nchunk, std::function<hipError_t(int)> download_and_wait)
    {
        try {
            th = std::thread([this, device, nchunk, download_and_wait] {
                hipError_t e = hipSetDevice(device);
                for (int c = 0; c < nchunk; ++c) {
                    {
                        std::unique_lock<std::mutex> lk(m);
                        cv.wait(lk, [&] { return stop || n_launched > c; });
                        if (n_launched <= c) return;
                    }
                    if (e == hipSuccess) e = download_and_wait(c);
                    {
                        std::lock_guard<std::mutex> lk(m);
                        if (e != hipSuccess) err = e;
                        n_drained = c + 1;
                    }
                    cv.notify_all();
                }
            });
        } catch (const std::exception &) {
            return false;
        }
        return true;
    }
    void launched(int c)
    {
        { std::lock_guard<std::mutex> lk(m); n_launched = c + 1; }
        cv.notify_all();
    }
    bool wait_drained(int c)                                  // false: a download failed
    {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return n_drained > c; });
        return err == hipSuccess;
    }
    hipError_t finish()                                       // all launched chunks drain, then the thread ends
    {
        { std::lock_guard<std::mutex> lk(m); stop = true; }
        cv.notify_all();
        if (th.joinable()) th.join();
        return err;
    }
    ~Downloader() { (void)finish(); }
};

// ---- the per-call context: what the stages below share
template <typename T>
struct Oneshot {
    const AmtArgs<T> &h;
    AmtParams<T> p;
    AmtWindow w;
    int device = 0;
    HostWorkspace &ws = tl_workspace;
    HostWorkspace::Kept &res = ws.res;
    const T *host[AMT_F_COUNT];
    bool halo[AMT_F_COUNT];                                   // goes up with the rows below and above its chunk (amt_halo.h)
    bool keep_want[AMT_F_COUNT] = {};                         // stays on the device between calls under the current settings
    bool pinned = true, pinned_small = true;                  // the 3-D arrays / the 2-D and 1-D ones
    size_t r3, r2, n1, ni;                                    // elements per j row of a 3-D / 2-D array, of a 1-D array; window columns
    int nj;
    WindowCells cells;
    Plan pl;
    Arena ar;
    T *dev[2][AMT_F_COUNT];
    int res_of[AMT_F_COUNT];                                  // kept entry of a field, -1: not kept
    bool res_upload[NKEEP] = {};
    long res_hi[NKEEP];                                       // highest row uploaded so far in this call
    char *stage = nullptr;                                    // staging buffer: mirrors the arena from stage_base on
    size_t stage_base = 0;
    FailGuard fail_guard{res};

    explicit Oneshot(const AmtArgs<T> &args) : h(args) {}
    T *kept(int f) const { return reinterpret_cast<T *>(res.buf[res_of[f]]); }
    T *staged(const T *devptr) const                          // the staging twin of a device address
    {
        return reinterpret_cast<T *>(stage + ((reinterpret_cast<const char *>(devptr) - ws.arena) - stage_base));
    }
    struct Chunk { int s, c0, c1; };                          // chunk c: buffer set s, rows c0..c1 of the window
    Chunk chunk(int c) const
    {
        const int c0 = w.j_start + (int)(c * pl.rows);
        return {c % pl.nset, c0, (c0 + pl.rows - 1 < w.j_end) ? (int)(c0 + pl.rows - 1) : w.j_end};
    }

    // ---- stage: the arrays, the plan and the layout of this call (pointer queries and host arithmetic)
    void describe()
    {
        amt_args_get_fields(h, host);
        r3 = (size_t)p.idim * p.kdim; r2 = (size_t)p.idim; n1 = (size_t)p.kdim;
        nj = w.j_end - w.j_start + 1;
        ni = (size_t)(p.i1 - p.i0 + 1);
        cells.es = sizeof(T); cells.idim = p.idim; cells.kdim = p.kdim; cells.i0 = p.i0; cells.ni = (long)ni; cells.k1 = p.k1; cells.nk = p.nk;
        int nbig = 0;                                         // 3-D arrays that need chunk buffers: all but the kept ones
        for (int f = 0; f < AMT_F_COUNT; ++f) {
            halo[f] = amt_halo_receives(AMT_HALO_BELOW, f) || amt_halo_receives(AMT_HALO_ABOVE, f);
            (amt_field_rank(f) == 3 ? pinned : pinned_small) &= amt_is_pinned(host[f]);
            nbig += amt_field_rank(f) == 3;
        }
        for (int r = 0; r < NKEEP; ++r) {
            const int f = kKeepField[r];
            keep_want[f] = r < NCACHE ? res.enabled : res.deferred(host[f]);
            if (keep_want[f] && amt_field_rank(f) == 3) --nbig;
        }
        pl = oneshot_plan(r3, r2, n1, nj, sizeof(T), pinned, pinned_small, nbig);
        ar = oneshot_layout(pl, r3, r2, n1, sizeof(T), keep_want);
    }

    // ---- stage: the thread's workspace on this device, with an arena of the planned size
    int acquire()
    {
        // Test hook (tests/test_gpu_20_host_cache.py, the one-GPU twin of the two-device test): AMT_TEST_PRETEND_DEVICE_CHANGE=n makes
        // the n-th one-shot call of a thread behave as if the thread had moved to another device since its last call -- the workspace
        // of the "old" device is given up exactly as prepare() gives it up, only the device number stays the same.
        const long calls_of_this_thread = ++tl_oneshot_calls;
        const char *pretend_env = getenv("AMT_TEST_PRETEND_DEVICE_CHANGE");
        const bool pretend_move = pretend_env && *pretend_env && atol(pretend_env) == calls_of_this_thread && ws.device >= 0;
        if (ws.device >= 0 && (ws.device != device || pretend_move) && ws.res.any_stale()) {
            // the thread moved to another device: prepare() gives the old device's workspace up, and deferred outputs whose only
            // current copy lives there must come down to their host arrays first (nothing the device alone holds is ever dropped,
            // ADVICE r04) -- on the OLD device, whose streams still exist
            const int rc = amt_keep_flush(ws);
            if (rc != AMT_OK) return rc;
        }
        if (pretend_move) ws.release();                       // what prepare() does when device != ws.device
        const hipError_t e = ws.prepare(device, pl.big_bytes + pl.small_bytes);
        if (e == hipErrorOutOfMemory) return amt_fail(AMT_ERR_ALLOC, "hipMalloc of %zu bytes failed", pl.big_bytes + pl.small_bytes);
        AMT_HIP(e);
        for (int s = 0; s < 2; ++s)
            for (int f = 0; f < AMT_F_COUNT; ++f)
                dev[s][f] = ar.off[s][f] == kNoSlot ? nullptr : reinterpret_cast<T *>(ws.arena + ar.off[s][f]);
        return AMT_OK;
    }

    // checksum of exactly the rows a call uploads of cached field f (rows j_start-1 / j_end+1 of a 3-D one only for the halo arrays)
    uint64_t uploaded_sum(int f) const
    {
        const int lo = halo[f] ? w.j_start - 1 : w.j_start, hi = halo[f] ? w.j_end + 1 : w.j_end;
        const int rank = amt_field_rank(f);
        return rank == 3 ? amt_host_sum(host[f] + (size_t)(lo - h.jms) * r3, (size_t)(hi - lo + 1) * r3 * sizeof(T))
             : rank == 2 ? amt_host_sum(host[f] + (size_t)(w.j_start - 1 - h.jms) * r2, r2 * pl.wrow * sizeof(T))
                         : amt_host_sum(host[f], n1 * sizeof(T));
    }

    // ---- stage: kept arrays, open.  Cached inputs and deferred outputs (whole-window copies): re-keyed when anything about the
    // call changed, then what this call has to upload of them and -- check mode -- whether the host side kept its word
    int keep_open()
    {
        for (int f = 0; f < AMT_F_COUNT; ++f) res_of[f] = -1;
        for (int r = 0; r < NKEEP; ++r) res_hi[r] = (long)w.j_start - 2;
        bool want[NKEEP];
        bool any_want = false;
        for (int r = 0; r < NKEEP; ++r) {
            want[r] = keep_want[kKeepField[r]];
            any_want = any_want || want[r];
        }
        const int key[16] = {(int)sizeof(T), h.ims, h.ime, h.kms, h.kme, h.jms, h.jme, w.j_start, w.j_end, p.i0, p.i1, p.nk, p.k1, device, 0, 0};
        bool same = memcmp(res.key, key, sizeof key) == 0;
        for (int r = 0; r < NKEEP && same; ++r)
            same = want[r] == res.active[r] && (!want[r] || res.host[r] == host[kKeepField[r]]);
        if (!same) {
            // another patch, another layout, other arrays or other settings: what only the device holds goes down to the
            // arrays it belongs to, then start over (nothing is in flight between calls)
            const int rc = amt_keep_flush(ws);
            if (rc != AMT_OK) return rc;
            res.drop();
            memcpy(res.key, key, sizeof key);
            res.cells = cells;
            res.j_start = w.j_start; res.j_end = w.j_end; res.jms = h.jms;
            for (int r = 0; r < NKEEP; ++r) {
                if (!want[r]) continue;
                const size_t each = (amt_keep_rank(r) == 3 ? r3 * pl.wrow : amt_keep_rank(r) == 2 ? r2 * pl.wrow : n1) * sizeof(T);
                const hipError_t e = hipMalloc((void **)&res.buf[r], each);
                if (e != hipSuccess) {
                    (void)hipGetLastError();
                    res.drop();
                    memset(res.key, 0, sizeof res.key);
                    return amt_fail(AMT_ERR_ALLOC, "kept arrays: hipMalloc of %zu bytes for %s failed (amt_host_cache_enable(0) / "
                                    "amt_host_defer(NULL, 0) run without them)", each, amt_keep_name(r));
                }
                res.bytes[r] = each;
                res.active[r] = true;
                res.host[r] = host[kKeepField[r]];
            }
        }
        for (int r = 0; r < NKEEP && any_want; ++r) {
            if (!res.active[r]) continue;
            const int f = kKeepField[r];
            res_of[f] = r;
            if (res.poisoned[r])
                return amt_fail(AMT_ERR_PRECONDITION, "deferred output %s: an earlier call failed part-way and its device copy is undefined; "
                                "call amt_host_invalidate for it (the host array, as last fetched, is the truth again) before the next sub-step",
                                amt_keep_name(r));
            res_upload[r] = !res.valid[r] && kAmtField[f].in;
            if (!res.check) continue;
            if (r < NCACHE) {
                // debug mode: a cached array that changed on the host without amt_host_invalidate is an error
                const uint64_t now_sum = uploaded_sum(f);
                if (res.valid[r] && now_sum != res.sum[r]) {
                    res.valid[r] = false;
                    return amt_fail(AMT_ERR_PRECONDITION, "residency cache: %s changed on the host since it was uploaded "
                                    "but amt_host_invalidate was not called for it (amt_host_cache_check)", amt_keep_name(r));
                }
                res.sum[r] = now_sum;
            } else if (res.stale[r] && !amt_keep_canary(res, r, false)) {
                // debug mode: the host array of a deferred output was written while the device held the truth
                return amt_fail(AMT_ERR_PRECONDITION, "deferred output %s was written on the host while its device copy was newer: "
                                "call amt_host_invalidate for it (the host is the truth) or amt_host_fetch before writing "
                                "(amt_host_cache_check)", amt_keep_name(r));
            }
        }
        return AMT_OK;
    }

    // ---- stage: kept arrays, close.  What the device copies are worth after a call that ended with rc
    void keep_close(int rc)
    {
        fail_guard.ok = (rc == AMT_OK);
        for (int r = 0; r < NKEEP; ++r) {
            if (!res.active[r]) continue;
            if (r < NCACHE) {
                res.valid[r] = (rc == AMT_OK);                // a cached input of a failed call simply goes up again
            } else if (rc == AMT_OK) {
                // the device copy is the truth from here on.  (After a call that FAILED once kernels were out, fail_guard marks the
                // deferred copies undefined: amt_host_fetch / the next call refuse them until amt_host_invalidate.)
                res.valid[r] = res.stale[r] = true;
                if (res.check) amt_keep_canary(res, r, true);
            }
        }
    }

    // ---- stage: the page-locked staging buffer of a packed call
    int stage_open()
    {
        stage_base = pl.pack_big ? 0 : ar.small_begin;
        if (!pl.pack_small) return AMT_OK;
        const hipError_t e = ws.stage_reserve(ar.end - stage_base);
        if (e == hipErrorOutOfMemory) return amt_fail(AMT_ERR_ALLOC, "hipHostMalloc of %zu bytes failed", ar.end - stage_base);
        AMT_HIP(e);
        stage = ws.stage;
        return AMT_OK;
    }

    // ---- stage: the 1-D and 2-D arrays go up, once
    int upload_small()
    {
        for (int f = 0; f < AMT_F_COUNT; ++f) {
            const int rank = amt_field_rank(f);
            if (rank == 3 || !kAmtField[f].in) continue;      // muave, muts, mudf: outputs only
            const size_t n = rank == 1 ? n1 : r2 * pl.wrow;
            const T *src = rank == 1 ? host[f] : host[f] + (size_t)(w.j_start - 1 - h.jms) * r2;
            if (res_of[f] >= 0) {                             // cached 2-D / 1-D input, deferred mu: up only while the device copy is not valid
                if (res_upload[res_of[f]]) AMT_HIP(hipMemcpyAsync(kept(f), src, n * sizeof(T), hipMemcpyHostToDevice, ws.up));
                continue;
            }
            if (pl.pack_small) memcpy(staged(dev[0][f]), src, n * sizeof(T));
            else AMT_HIP(hipMemcpyAsync(dev[0][f], src, n * sizeof(T), hipMemcpyHostToDevice, ws.up));
        }
        if (pl.pack_small && !pl.pack_big)
            AMT_HIP(hipMemcpyAsync(ws.arena + ar.small_begin, stage, ar.end - ar.small_begin, hipMemcpyHostToDevice, ws.up));
        return AMT_OK;
    }

    // level 1 of rows c0..c1 of ww, the only part of it the routine reads
    int upload_ww_level1(int s, int c0, int c1)
    {
        const int f = AMT_F_WW;
        const T *src = host[f] + (size_t)(c0 - h.jms) * r3 + (size_t)p.k1 * p.idim;
        const size_t pitch = r3 * sizeof(T), width = (size_t)p.idim * sizeof(T), nrow = (size_t)(c1 - c0 + 1);
        if (res_of[f] >= 0) {                                 // deferred: goes up only while the device copy is not valid
            if (res_upload[res_of[f]])
                AMT_HIP(hipMemcpy2DAsync(kept(f) + (size_t)(c0 - (w.j_start - 1)) * r3 + (size_t)p.k1 * p.idim, pitch, src, pitch, width, nrow,
                                         hipMemcpyHostToDevice, ws.up));
            return AMT_OK;
        }
        T *dst = dev[s][f] + r3 + (size_t)p.k1 * p.idim;
        if (pl.pack_big)
            for (int j = c0; j <= c1; ++j) memcpy(staged(dst) + (size_t)(j - c0) * r3, src + (size_t)(j - c0) * r3, width);
        else
            AMT_HIP(hipMemcpy2DAsync(dst, pitch, src, pitch, width, nrow, hipMemcpyHostToDevice, ws.up));
        return AMT_OK;
    }

    // ---- stage: upload of chunk c -- its rows, plus one halo row each side of the arrays the stencil reads across rows
    int upload_chunk(int c)
    {
        const Chunk k = chunk(c);
        const int s = k.s, c0 = k.c0, c1 = k.c1, ja = c0 - 1;  // device row 0 <-> Fortran row ja
        for (int f = 0; f < AMT_F_COUNT; ++f) {
            if (amt_field_rank(f) != 3 || !kAmtField[f].in) continue;
            if (f == AMT_F_WW) {
                if (int rc = upload_ww_level1(s, c0, c1)) return rc;
                continue;
            }
            int lo = halo[f] ? c0 - 1 : c0;
            const int hi = halo[f] ? c1 + 1 : c1;
            if (res_of[f] >= 0) {
                // kept: its rows go up only while the device copy is not valid, and every row ONCE per call -- a later chunk
                // starts behind what the earlier ones uploaded (its lower halo rows are already there, and the kernel of the
                // chunk before may be reading them: ADVICE r03)
                const int r = res_of[f];
                if (res_upload[r]) {
                    if (lo <= res_hi[r]) lo = (int)res_hi[r] + 1;
                    if (lo <= hi)
                        AMT_HIP(hipMemcpyAsync(kept(f) + (size_t)(lo - (w.j_start - 1)) * r3, host[f] + (size_t)(lo - h.jms) * r3,
                                               (size_t)(hi - lo + 1) * r3 * sizeof(T), hipMemcpyHostToDevice, ws.up));
                    res_hi[r] = hi;
                }
                continue;
            }
            const size_t n = (size_t)(hi - lo + 1) * r3 * sizeof(T);
            if (pl.pack_big) memcpy(staged(dev[s][f]) + (size_t)(lo - ja) * r3, host[f] + (size_t)(lo - h.jms) * r3, n);
            else AMT_HIP(hipMemcpyAsync(dev[s][f] + (size_t)(lo - ja) * r3, host[f] + (size_t)(lo - h.jms) * r3, n, hipMemcpyHostToDevice, ws.up));
        }
        if (pl.pack_big)                                      // one chunk: everything, small arrays included
            AMT_HIP(hipMemcpyAsync(ws.arena, stage, ar.end, hipMemcpyHostToDevice, ws.up));
        AMT_HIP(hipEventRecord(ws.uploaded[s], ws.up));
        return AMT_OK;
    }

    // ---- stage: launch of chunk c, as a tile of the same domain (global jds, jde) whose arrays all begin at row c0 - 1.
    // Returns what the kernel call returned in `rc`; its own return value is that of the stream calls around it.
    int launch_chunk(int c, int &rc)
    {
        const Chunk k = chunk(c);
        const int s = k.s, c0 = k.c0, c1 = k.c1, ja = c0 - 1;
        AmtArgs<T> d = h;
        T *q[AMT_F_COUNT];
        for (int f = 0; f < AMT_F_COUNT; ++f) {
            const int rank = amt_field_rank(f);
            const size_t row = rank == 3 ? r3 : r2;
            q[f] = rank == 1 ? (res_of[f] >= 0 ? kept(f) : dev[0][f])
                 : res_of[f] >= 0 ? kept(f) + (size_t)(ja - (w.j_start - 1)) * row
                 : rank == 2 ? dev[0][f] + (size_t)(ja - (w.j_start - 1)) * row : dev[s][f];
        }
        amt_args_set_fields(d, q);
        d.jms = ja; d.jme = c1 + 1; d.jts = c0; d.jte = c1;
        AMT_HIP(hipStreamWaitEvent(ws.comp, ws.uploaded[s], 0));
        fail_guard.launched = true;
        rc = amt_device_call<T>(ws.comp, AMT_VARIANT_AUTO, d);
        if (rc == AMT_OK && getenv("AMT_TEST_FAIL_AFTER_LAUNCH"))   // test hook: a failure after the first kernel went out
            rc = amt_fail(AMT_ERR_HIP, "AMT_TEST_FAIL_AFTER_LAUNCH: simulated failure after chunk %d was launched", c);
        if (rc == AMT_OK) AMT_HIP(hipEventRecord(ws.computed[s], ws.comp));
        return AMT_OK;
    }

    // ---- stage: download of chunk c -- its window cells of ww, t, t_ave: nothing else of the host arrays is touched
    hipError_t download_chunk(int c)
    {
        const Chunk k = chunk(c);
        hipError_t e = hipStreamWaitEvent(ws.down, ws.computed[k.s], 0);
        for (int f = 0; f < AMT_F_COUNT && p.nk > 0 && e == hipSuccess; ++f) {
            if (!kAmtField[f].out || amt_field_rank(f) != 3 || res_of[f] >= 0) continue;   // deferred outputs stay on the device
            e = amt_window_down(cells, 3, const_cast<T *>(host[f]), (size_t)(k.c0 - h.jms), dev[k.s][f], 1, (size_t)(k.c1 - k.c0 + 1), ws.down);
        }
        return e != hipSuccess ? e : hipEventRecord(ws.drained[k.s], ws.down);
    }

    // ---- stage: the outputs that come down once, after the last kernel
    int download_small()
    {
        AMT_HIP(hipStreamWaitEvent(ws.down, ws.computed[(pl.nchunk - 1) % pl.nset], 0));
        if (!pl.pack_small) {
            for (int f = 0; f < AMT_F_COUNT; ++f) {
                if (!kAmtField[f].out || amt_field_rank(f) != 2 || res_of[f] >= 0) continue;
                // the window's cells only (a strided copy): two host threads running tiles that split i
                // must not rewrite each other's columns with what they uploaded
                AMT_HIP(amt_window_down(cells, 2, const_cast<T *>(host[f]), (size_t)(w.j_start - h.jms), dev[0][f], 1, (size_t)nj, ws.down));
            }
            return AMT_OK;
        }
        const size_t from = pl.pack_big ? ar.out3_begin : ar.small_begin;
        AMT_HIP(hipMemcpyAsync(stage + (from - stage_base), ws.arena + from, ar.small_out_end - from, hipMemcpyDeviceToHost, ws.down));
        AMT_HIP(hipStreamSynchronize(ws.down));
        for (int f = 0; f < AMT_F_COUNT; ++f) {               // scatter: the window's cells only
            if (!kAmtField[f].out || res_of[f] >= 0) continue;   // deferred outputs stay on the device
            T *to = const_cast<T *>(host[f]);
            if (amt_field_rank(f) == 2) {
                for (int j = w.j_start; j <= w.j_end; ++j)
                    memcpy(to + (size_t)(j - h.jms) * r2 + p.i0, staged(dev[0][f]) + (size_t)(j - w.j_start + 1) * r2 + p.i0, ni * sizeof(T));
            } else if (pl.pack_big) {
                for (int j = w.j_start; j <= w.j_end; ++j)
                    for (int k = 0; k < p.nk; ++k) {
                        const size_t e = (size_t)(p.k1 + k) * p.idim + p.i0;
                        memcpy(to + (size_t)(j - h.jms) * r3 + e, staged(dev[0][f]) + (size_t)(j - w.j_start + 1) * r3 + e, ni * sizeof(T));
                    }
            }
        }
        return AMT_OK;
    }
};
}  // namespace

template <typename T>
static int amt_host_call(const AmtArgs<T> &h)
{
    Oneshot<T> o(h);
    bool empty = false;
    int rc = amt_build_params(h, o.p, o.w, &empty);
    if (rc != AMT_OK || empty) return rc;
    int ndev = 0;
    AMT_HIP(hipGetDeviceCount(&ndev));
    if (ndev < 1) return amt_fail(AMT_ERR_NO_DEVICE, "no HIP device visible");
    AMT_HIP(hipGetDevice(&o.device));
    o.describe();
    const Plan &pl = o.pl;
    const bool trace = getenv("AMT_STREAM_TRACE") != nullptr;
    const double t_begin = now_ms();

    if ((rc = o.acquire()) != AMT_OK) return rc;
    WorkspaceScope scope{o.ws};                               // drains the three streams on every way out
    if ((rc = o.keep_open()) != AMT_OK) return rc;
    if ((rc = o.stage_open()) != AMT_OK) return rc;
    const double t_alloc = now_ms();
    if ((rc = o.upload_small()) != AMT_OK) return rc;

    Downloader dl;                                            // pageable 3-D arrays, several chunks: the downloads are issued by a second thread
    const bool threaded = pl.may_thread && pl.nchunk > 1 &&   // (none to be had: they are queued from this one, the pageable order)
                          dl.start(o.device, pl.nchunk, [&o](int c) {
                              const hipError_t e = o.download_chunk(c);
                              return e != hipSuccess ? e : hipStreamSynchronize(o.ws.down);
                          });
    for (int c = 0; c < pl.nchunk; ++c) {
        if (c >= pl.nset) {                                   // buffer set c % nset is free again
            if (threaded) { if (!dl.wait_drained(c - pl.nset)) break; }
            else AMT_HIP(hipStreamWaitEvent(o.ws.up, o.ws.drained[c % pl.nset], 0));
        }
        if (int e = o.upload_chunk(c)) return e;
        if (int e = o.launch_chunk(c, rc)) return e;
        if (rc != AMT_OK) break;
        if (threaded) dl.launched(c);
        else if (!pl.pack_big) AMT_HIP(o.download_chunk(c));
    }
    if (threaded && dl.finish() != hipSuccess && rc == AMT_OK)
        rc = amt_fail(AMT_ERR_HIP, "download of a chunk failed: %s", hipGetErrorString(dl.err));
    if (rc == AMT_OK)
        if (int e = o.download_small()) return e;

    const double t_enq = now_ms();
    for (hipStream_t st : {o.ws.up, o.ws.comp, o.ws.down}) {
        hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess && rc == AMT_OK)
            rc = amt_fail(AMT_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
    }
    o.keep_close(rc);
    if (trace)
        fprintf(stderr, "amt one-shot: %d chunk(s) of %ld rows, 3-D %s%s, small arrays %s; alloc %.2f ms, enqueue %.2f ms, drain %.2f ms\n",
                pl.nchunk, pl.rows, o.pinned ? "pinned" : pl.pack_big ? "packed" : "pageable", threaded ? " + download thread" : "",
                o.pinned_small ? "pinned" : pl.pack_small ? "packed" : "pageable", t_alloc - t_begin, t_enq - t_alloc, now_ms() - t_enq);
    return rc;
}

// ---------------------------------------------------------------------------
// One call, several devices: the j range of the tile fanned over device slots (amt_host_set_devices / AMT_ONESHOT_DEVICES).
//
// The reference's host call IS the multi-GPU call: advance_mu_t_no_async.cu:108-162 splits j over `GPUs` devices inside one
// advance_mu_t(...), refills each device's halo rows from the HOST arrays (:135-160), launches and gathers per device
// (:329-390).  Here the calling thread owns one WORKER THREAD per device slot; a call cuts jts..jte into contiguous pieces
// (uneven where the rows do not divide) and every worker runs the ordinary one-shot call on its piece -- a tile of the same
// domain, global ids..jde unchanged, so the window rule clips each piece as it clips the whole (module_small_step_em.f90:
// 91-106), and the rows a piece reads across its edges come from the host arrays, as in the reference: no traffic between
// the devices at all.  A worker is a host thread, so everything a thread keeps between calls (streams, arena, residency cache,
// deferred outputs: HostWorkspace above) exists once per slot, on the slot's device, and the control calls (amt_host_cache_*,
// amt_host_defer / _fetch / _stale / _invalidate / _release) are forwarded to every slot.  The host link is the bound of the
// one-shot path: n devices on n links carry n times the rows.  Slots may name one device several
// times (how the tests run on a one-GPU box).
// ---------------------------------------------------------------------------
void amt_march_note_kernel(const char *name);                 // amt_kernel_march.hip: what amt_march_last_kernel reports
namespace {
struct FanWorker {
    int device = 0;
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::function<int()> job;
    bool has_job = false, done = false, stop = false;
    int rc = AMT_OK;
    std::string error, kernel;

    void main()
    {
        (void)hipSetDevice(device);
        for (;;) {
            std::function<int()> f;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return stop || has_job; });
                if (!has_job) return;                          // stop: the thread's workspace is released by its destructor
                f = job;
            }
            (void)hipSetDevice(device);
            const int r = f();
            {
                std::lock_guard<std::mutex> lk(m);
                rc = r;
                error = r == AMT_OK ? "" : amt_last_error();
                kernel = amt_march_last_kernel();
                has_job = false;
                done = true;
            }
            cv.notify_all();
        }
    }
    void post(std::function<int()> f)
    {
        { std::lock_guard<std::mutex> lk(m); job = std::move(f); has_job = true; done = false; }
        cv.notify_all();
    }
    int wait()
    {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return done; });
        return rc;
    }
};

struct Fan {
    std::vector<std::unique_ptr<FanWorker>> slots;
    bool env_checked = false;
    bool active() const { return !slots.empty(); }

    // every slot runs f on its own thread; the first failure (by slot) is the call's, with its text
    int all(const std::function<int(int slot)> &f, int *max_rc = nullptr)
    {
        for (size_t q = 0; q < slots.size(); ++q) slots[q]->post([f, q] { return f((int)q); });
        int first = AMT_OK, worst = 0;
        std::string text;
        for (auto &w : slots) {
            const int rc = w->wait();
            if (max_rc) {                                      // amt_host_stale: -1 (undefined) beats 1 (stale) beats 0
                if (rc < 0) worst = -1;
                else if (rc > 0 && worst == 0) worst = 1;
            } else if (rc != AMT_OK && first == AMT_OK) {
                first = rc;
                text = w->error;
            }
        }
        if (max_rc) { *max_rc = worst; return AMT_OK; }
        return first == AMT_OK ? AMT_OK : amt_fail(first, "%s", text.c_str());
    }
    int stop()
    {
        if (slots.empty()) return AMT_OK;
        const int rc = all([](int) { return host_release_local(); });     // what only a slot's device holds comes down first
        for (auto &w : slots) {
            { std::lock_guard<std::mutex> lk(w->m); w->stop = true; }
            w->cv.notify_all();
            if (w->th.joinable()) w->th.join();
        }
        slots.clear();
        return rc;
    }
    int start(int n, const int *ids)
    {
        int ndev = 0;
        AMT_HIP(hipGetDeviceCount(&ndev));
        for (int q = 0; q < n; ++q)
            if (ids[q] < 0 || ids[q] >= ndev) return amt_fail(AMT_ERR_INVALID_ARG, "amt_host_set_devices: device %d of %d visible", ids[q], ndev);
        int rc = stop();
        if (rc == AMT_OK) rc = host_release_local();           // what the calling thread's own device copies hold comes down: the slots read the host arrays
        if (rc != AMT_OK) return rc;
        const HostWorkspace::Kept &mine = tl_workspace.res;    // the calling thread's settings go to every slot
        try {                                                  // std::thread and the containers throw; nothing may leave through the C-ABI
            for (int q = 0; q < n; ++q) {
                std::unique_ptr<FanWorker> w(new FanWorker);
                w->device = ids[q];
                FanWorker *raw = w.get();
                slots.push_back(std::move(w));
                slots.back()->th = std::thread([raw] { raw->main(); });
            }
        } catch (const std::exception &e) {
            if (!slots.empty() && !slots.back()->th.joinable()) slots.pop_back();      // the slot whose thread did not start
            (void)stop();
            return amt_fail(AMT_ERR_ALLOC, "amt_host_set_devices: could not start %d slot threads: %s", n, e.what());
        }
        const bool enabled = mine.enabled, check = mine.check, defer_all = mine.defer_all;
        std::vector<const void *> deferred(mine.defer_ptr, mine.defer_ptr + mine.ndefer);
        return all([=](int) {
            int r = host_cache_enable_local(enabled);
            if (r == AMT_OK) r = host_cache_check_local(check);
            if (r == AMT_OK && defer_all) r = host_defer_local(nullptr, 1);
            for (const void *q : deferred)
                if (r == AMT_OK) r = host_defer_local(q, 1);
            return r;
        });
    }
    // A thread that ends takes its slots down in order (deferred outputs come down first).  The MAIN thread's destructor runs at
    // process exit, possibly after the HIP runtime's own teardown: there the workers are left to the operating system, like
    // the main thread's HostWorkspace.
    ~Fan()
    {
        if ((long)syscall(SYS_gettid) != (long)getpid()) { (void)stop(); return; }
        for (auto &w : slots) { w->th.detach(); (void)w.release(); }
    }
};
thread_local Fan tl_fan;

// AMT_ONESHOT_DEVICES="0,1,2" | "all": the device slots of every thread that has not called amt_host_set_devices (hosts that
// cannot add a call: the Fortran drop-in module is one CALL).  Read on a thread's first one-shot or control call.
int fan_from_env()
{
    Fan &fan = tl_fan;
    if (fan.env_checked) return AMT_OK;
    fan.env_checked = true;
    const char *e = getenv("AMT_ONESHOT_DEVICES");
    if (!e || !*e) return AMT_OK;
    std::vector<int> ids;
    if (!strcmp(e, "all")) {
        int ndev = 0;
        AMT_HIP(hipGetDeviceCount(&ndev));
        for (int d = 0; d < ndev; ++d) ids.push_back(d);
    } else {
        for (const char *q = e; *q;) {
            char *end = nullptr;
            const long v = strtol(q, &end, 10);
            if (end == q) return amt_fail(AMT_ERR_INVALID_ARG, "AMT_ONESHOT_DEVICES must be a comma-separated list of device numbers or 'all', not '%s'", e);
            ids.push_back((int)v);
            q = *end == ',' ? end + 1 : end;
            if (*end && *end != ',') return amt_fail(AMT_ERR_INVALID_ARG, "AMT_ONESHOT_DEVICES must be a comma-separated list of device numbers or 'all', not '%s'", e);
        }
    }
    if (ids.empty()) return AMT_OK;
    if (ids.size() == 1) {                                     // one device: no fan, the calls of this thread go there
        AMT_HIP(hipSetDevice(ids[0]));
        return AMT_OK;
    }
    return fan.start((int)ids.size(), ids.data());
}

template <typename T>
int amt_host_call_fanned(const AmtArgs<T> &h)
{
    Fan &fan = tl_fan;
    // the preconditions of the whole tile, once, on the calling thread (host arithmetic): a bad call fails before any piece runs
    {
        AmtParams<T> p;
        AmtWindow w;
        bool empty = false;
        const int rc = amt_build_params(h, p, w, &empty);
        if (rc != AMT_OK || empty) return rc;
    }
    const int n = (int)fan.slots.size();
    const long rows = (long)h.jte - h.jts + 1;
    const int rc = fan.all([&h, n, rows](int q) {
        const int lo = h.jts + (int)((rows * q) / n), hi = h.jts + (int)((rows * (q + 1)) / n) - 1;
        if (hi < lo) return (int)AMT_OK;                       // fewer rows than slots: this one has none
        AmtArgs<T> mine = h;
        mine.jts = lo;
        mine.jte = hi;
        return amt_host_call<T>(mine);
    });
    if (rc == AMT_OK && !fan.slots[0]->kernel.empty()) amt_march_note_kernel(fan.slots[0]->kernel.c_str());
    return rc;
}
}  // namespace

extern "C" int amt_host_set_devices(int n, const int *device_ids)
{
    if (n < 0 || (n > 0 && !device_ids) || n > 64) return amt_fail(AMT_ERR_INVALID_ARG, "bad device list");
    tl_fan.env_checked = true;                                 // an explicit call outranks AMT_ONESHOT_DEVICES
    if (n == 0) return tl_fan.stop();
    return tl_fan.start(n, device_ids);
}

extern "C" int amt_host_devices(int *device_ids, int cap)
{
    const Fan &fan = tl_fan;
    for (int q = 0; q < (int)fan.slots.size() && q < cap && device_ids; ++q) device_ids[q] = fan.slots[q]->device;
    return (int)fan.slots.size();
}

#define AMT_FAN_OR_LOCAL(local_call)                                              \
    do {                                                                           \
        if (int rc_ = fan_from_env()) return rc_;                                  \
        if (tl_fan.active()) {                                                     \
            const int rc_ = tl_fan.all([=](int) { return local_call; });           \
            if (rc_ != AMT_OK) return rc_;                                         \
        }                                                                          \
        return local_call;                                                         \
    } while (0)

extern "C" int amt_host_cache_enable(int on) { AMT_FAN_OR_LOCAL(host_cache_enable_local(on)); }
extern "C" int amt_host_cache_check(int on) { AMT_FAN_OR_LOCAL(host_cache_check_local(on)); }
extern "C" int amt_host_invalidate(const void *host_ptr) { AMT_FAN_OR_LOCAL(host_invalidate_local(host_ptr)); }
extern "C" int amt_host_defer(const void *host_ptr, int on) { AMT_FAN_OR_LOCAL(host_defer_local(host_ptr, on)); }
extern "C" int amt_host_fetch(const void *host_ptr) { AMT_FAN_OR_LOCAL(host_fetch_local(host_ptr)); }
extern "C" int amt_host_release(void) { AMT_FAN_OR_LOCAL(host_release_local()); }
extern "C" int amt_host_stale(const void *host_ptr)
{
    (void)fan_from_env();
    int worst = host_stale_local(host_ptr);
    if (tl_fan.active()) {
        int w = 0;
        (void)tl_fan.all([=](int) { return host_stale_local(host_ptr); }, &w);
        if (w < 0 || worst < 0) worst = -1;
        else if (w > 0) worst = 1;
    }
    return worst;
}

extern "C" int amt_advance_mu_t_f32(AMT_SIG(float))
{
    AMT_PACK_ARGS(float)
    if (int rc = fan_from_env()) return rc;
    return tl_fan.active() ? amt_host_call_fanned<float>(a) : amt_host_call<float>(a);
}
extern "C" int amt_advance_mu_t_f64(AMT_SIG(double))
{
    AMT_PACK_ARGS(double)
    if (int rc = fan_from_env()) return rc;
    return tl_fan.active() ? amt_host_call_fanned<double>(a) : amt_host_call<double>(a);
}
