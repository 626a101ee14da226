// amt_oneshot_plan.h -- the host arithmetic of the one-shot call (amt_oneshot.hip): how the window's rows are cut into chunks,
// which transfer regime carries them, and where every array lies in the device arena.  No HIP call: tests/oneshot_plan_check.cpp
// runs these two functions on the host over many shapes (not installed).
#pragma once
#include "amt_internal.h"

inline int amt_env_flag(const char *name, int dflt)
{
    const char *v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}
inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// ---- stage: plan.  How the window's nj rows are cut into chunks and which regime carries them: host arithmetic, no HIP call.
struct Plan {
    long rows;                                                // rows per chunk
    int nchunk, nset;                                         // chunks; device buffer sets of the 3-D arrays
    size_t crow, wrow;                                        // device rows per 3-D buffer set / of a 2-D array (the window's +-1)
    bool may_thread, pack_small, pack_big;
    size_t small_bytes, big_bytes;
};
// r3, r2: elements per j row of a 3-D / 2-D array; n1: elements of a 1-D array; nbig: the 3-D arrays that stream through chunk buffers
inline Plan oneshot_plan(size_t r3, size_t r2, size_t n1, int nj, size_t esize, bool pinned, bool pinned_small, int nbig)
{
    Plan pl;
    // chunking: ~320 MB of 3-D arrays per chunk (measured best at 1024x60x1024 fp64), counting the arrays that stream
    const char *env_rows = getenv("AMT_STREAM_ROWS");         // test/tuning knob: rows per chunk
    pl.may_thread = !pinned && amt_env_flag("AMT_STREAM_THREAD", 1);
    pl.rows = env_rows ? atol(env_rows) : (pinned || pl.may_thread) ? (long)((320u << 20) / (r3 * esize * (size_t)(nbig > 0 ? nbig : 1)) + 1) : (long)nj;
    if (pl.rows < 1) pl.rows = 1;
    if (pl.rows > nj) pl.rows = nj;
    pl.nchunk = (int)((nj + pl.rows - 1) / pl.rows);
    pl.nset = pl.nchunk > 1 ? 2 : 1;
    pl.crow = (size_t)pl.rows + 2;
    pl.wrow = (size_t)nj + 2;
    // packing (see above): the small arrays when they are pageable, the 3-D ones too when they are pageable, one chunk and small
    pl.small_bytes = 12 * (r2 * pl.wrow * esize + 256) + 4 * (n1 * esize + 256);
    pl.big_bytes = (size_t)pl.nset * nbig * (r3 * pl.crow * esize + 256);
    const bool allow_pack = amt_env_flag("AMT_STREAM_PACK", 1) != 0;
    pl.pack_small = allow_pack && !pinned_small && pl.small_bytes <= ((size_t)32 << 20);
    pl.pack_big = pl.pack_small && !pinned && pl.nchunk == 1 && pl.big_bytes <= ((size_t)64 << 20);
    return pl;
}

// ---- stage: arena layout.  [3-D inputs][3-D outputs][small outputs][small inputs] in 256-byte steps -- what comes down is one
// contiguous range, and so is everything a packed call sends up.  Offsets into the workspace's arena; a 3-D array that is kept
// on the device (keep_want) lives in its whole-window copy and gets no slot.
constexpr size_t kNoSlot = ~(size_t)0;
struct Arena {
    size_t off[2][AMT_F_COUNT];                               // per buffer set
    size_t out3_begin, small_begin, small_out_end, end;
};
inline Arena oneshot_layout(const Plan &pl, size_t r3, size_t r2, size_t n1, size_t esize, const bool *keep_want)
{
    static const struct { bool big, out; } classes[4] = {{true, false}, {true, true}, {false, true}, {false, false}};
    Arena a;
    size_t used = 0, begin[4];
    auto take = [&used](size_t bytes) { const size_t off = align256(used); used = off + bytes; return off; };
    for (int c = 0; c < 4; ++c) {
        begin[c] = align256(used);
        for (int f = 0; f < AMT_F_COUNT; ++f) {
            const int rank = amt_field_rank(f);
            if ((rank == 3) != classes[c].big || kAmtField[f].out != classes[c].out) continue;
            if (rank == 3 && keep_want[f]) {
                a.off[0][f] = a.off[1][f] = kNoSlot;
            } else if (rank == 3) {
                for (int s = 0; s < pl.nset; ++s) a.off[s][f] = take(r3 * pl.crow * esize);
                if (pl.nset == 1) a.off[1][f] = a.off[0][f];
            } else {
                a.off[0][f] = a.off[1][f] = take((rank == 2 ? r2 * pl.wrow : n1) * esize);
            }
        }
    }
    a.out3_begin = begin[1]; a.small_begin = begin[2]; a.small_out_end = begin[3]; a.end = used;
    return a;
}
