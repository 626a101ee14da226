// Stand-alone host check of the one-shot call's plan and arena layout (csrc/amt_oneshot_plan.h): no HIP call is made.
//   chunks tile the window's rows exactly; slots are disjoint, 256-byte aligned and inside big_bytes + small_bytes;
//   the two ranges a packed call copies are contiguous and hold exactly what has to cross.
// Built and run by tests/test_oneshot_plan.py (with the undefined-behaviour sanitizer on); exit status 0 = every case held.
#include "amt_oneshot_plan.h"
#include <vector>

static long failures = 0, cases = 0;
#define CHECK(cond)                                                                                         \
    do {                                                                                                    \
        if (!(cond) && failures++ < 20) fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, what); \
    } while (0)

struct Slot { size_t lo, hi; int f; };

static void check_case(size_t idim, size_t kdim, int nj, size_t es, bool pinned, bool pinned_small, int keep_mode, const char *what)
{
    ++cases;
    const size_t r3 = idim * kdim, r2 = idim, n1 = kdim;
    bool keep_want[AMT_F_COUNT] = {};
    int nbig = 0;
    for (int f = 0; f < AMT_F_COUNT; ++f) {
        const bool cached = kAmtField[f].in && !kAmtField[f].out && f != AMT_F_U && f != AMT_F_V;
        keep_want[f] = ((keep_mode & 1) && cached) || ((keep_mode & 2) && kAmtField[f].out);
        nbig += amt_field_rank(f) == 3 && !keep_want[f];
    }
    const Plan pl = oneshot_plan(r3, r2, n1, nj, es, pinned, pinned_small, nbig);
    const Arena ar = oneshot_layout(pl, r3, r2, n1, es, keep_want);

    // chunks tile j_start..j_end exactly (chunk c: rows c * rows .. min((c + 1) * rows, nj) - 1 of the window)
    CHECK(pl.rows >= 1 && pl.rows <= nj);
    CHECK((long)pl.nchunk * pl.rows >= nj && (long)(pl.nchunk - 1) * pl.rows < nj);
    CHECK(pl.nset == (pl.nchunk > 1 ? 2 : 1) && pl.crow == (size_t)pl.rows + 2 && pl.wrow == (size_t)nj + 2);
    CHECK(!pl.pack_big || (pl.pack_small && pl.nchunk == 1 && !pinned));
    CHECK(!pl.pack_small || !pinned_small);

    // slots: aligned, inside the arena, disjoint
    std::vector<Slot> slots;
    for (int f = 0; f < AMT_F_COUNT; ++f) {
        const int rank = amt_field_rank(f);
        const size_t bytes = (rank == 3 ? r3 * pl.crow : rank == 2 ? r2 * pl.wrow : n1) * es;
        if (rank == 3 && keep_want[f]) { CHECK(ar.off[0][f] == kNoSlot && ar.off[1][f] == kNoSlot); continue; }
        const int nslot = rank == 3 ? pl.nset : 1;
        for (int s = 0; s < nslot; ++s) slots.push_back({ar.off[s][f], ar.off[s][f] + bytes, f});
        if (nslot == 1) CHECK(ar.off[1][f] == ar.off[0][f]);
    }
    for (size_t a = 0; a < slots.size(); ++a) {
        CHECK(slots[a].lo % 256 == 0 && slots[a].hi <= ar.end);
        for (size_t b = a + 1; b < slots.size(); ++b) CHECK(slots[a].hi <= slots[b].lo || slots[b].hi <= slots[a].lo);
    }
    CHECK(ar.end <= pl.big_bytes + pl.small_bytes);
    CHECK(ar.out3_begin <= ar.small_begin && ar.small_begin <= ar.small_out_end && ar.small_out_end <= ar.end);

    // the packed ranges: what goes up is [small_begin, end) (small arrays only) or [0, end); what comes down is
    // [small_begin or out3_begin, small_out_end).  A slot lies inside a range exactly when it has to cross in that direction.
    for (const Slot &s : slots) {
        const bool big = amt_field_rank(s.f) == 3;
        const bool in_small_range = s.lo >= ar.small_begin && s.hi <= ar.end;
        CHECK(in_small_range == !big);                                             // the small arrays, all of them, and no 3-D one
        const size_t from = pl.pack_big ? ar.out3_begin : ar.small_begin;
        const bool comes_down = kAmtField[s.f].out && (pl.pack_big || !big);
        const bool in_down_range = s.lo >= from && s.hi <= ar.small_out_end;
        const bool outside_down_range = s.hi <= from || s.lo >= ar.small_out_end;
        CHECK(in_down_range || outside_down_range);                                // never half inside
        if (pl.pack_small) CHECK(in_down_range == comes_down);
    }
}

int main()
{
    const size_t shapes[][3] = {{1, 2, 1}, {3, 2, 1}, {18, 9, 16}, {39, 6, 11}, {72, 13, 32}, {72, 13, 22}, {152, 25, 42}, {66, 41, 66},
                                {202, 13, 42}, {132, 4, 9}, {520, 61, 512}, {702, 61, 152}, {1032, 61, 1024}, {4104, 61, 64}};
    const char *rows_env[] = {nullptr, "1", "5", "7", "13", "1000", "0", "-3"};
    char what[200];
    for (const char *rows : rows_env)
        for (int knobs = 0; knobs < 4; ++knobs) {
            if (rows) setenv("AMT_STREAM_ROWS", rows, 1); else unsetenv("AMT_STREAM_ROWS");
            setenv("AMT_STREAM_PACK", knobs & 1 ? "0" : "1", 1);
            setenv("AMT_STREAM_THREAD", knobs & 2 ? "0" : "1", 1);
            for (const auto &sh : shapes)
                for (size_t es : {(size_t)4, (size_t)8})
                    for (int pin = 0; pin < 4; ++pin)
                        for (int keep_mode = 0; keep_mode < 4; ++keep_mode) {
                            snprintf(what, sizeof what, "rows=%s knobs=%d shape=%zux%zux%zu es=%zu pin=%d keep=%d", rows ? rows : "-", knobs,
                                     sh[0], sh[1], sh[2], es, pin, keep_mode);
                            check_case(sh[0], sh[1], (int)sh[2], es, pin & 1, pin & 2, keep_mode, what);
                        }
        }
    printf("%ld cases, %ld failures\n", cases, failures);
    return failures ? 1 : 0;
}
