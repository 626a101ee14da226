// Stand-alone host check of the work-item decomposition of the streaming kernels (csrc/amt_chunk_index.h, called by
// amt_stage.hip and amt_sumflux.hip): no HIP call is made.  On the device the 64-bit branch needs a job of more than 2^31 - 1
// work items -- tens of GB --; on the host it is integer arithmetic.
//   * wherever total = nk * nj * chunks <= 2^31 - 1 the narrow (32-bit divisions) and the wide path agree;
//   * the wide path returns the exact (j, k, i0, cnt), against 128-bit arithmetic, for totals and e up to 2^40 and past it;
//   * e = 2^31 - 1, 2^31, 2^32 - 1 and 2^32 are among the samples of every job that has them;
//   * the vectors a caller passes in (a file of "kPer ni nk nj e j k i0 cnt" lines, computed elsewhere) hold as well.
// Built and run by tests/test_chunk_index.py with the undefined-behaviour and address sanitizers on; exit status 0 = all held.
#include "amt_chunk_index.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef unsigned __int128 u128;

static long failures = 0, checks = 0, narrow_checks = 0, wide_only = 0, boundaries = 0;

static void fail(const char *what, int per, long ni, long nk, long nj, long e)
{
    if (failures++ < 20) fprintf(stderr, "%s: kPer %d ni %ld nk %ld nj %ld e %ld\n", what, per, ni, nk, nj, e);
}

template <int kPer>
static void check_one(long ni, long nk, long nj, long e, const long *expect)
{
    const long chunks = (ni + kPer - 1) / kPer;
    const u128 total = (u128)nk * (u128)nj * (u128)chunks;
    if ((u128)e >= total) return;
    // plain 128-bit arithmetic from the definition: e = (j * nk + k) * chunks + c
    const u128 r = (u128)e / (u128)chunks, c = (u128)e % (u128)chunks;
    const long j_want = (long)(r / (u128)nk), k_want = (long)(r % (u128)nk), i0_want = (long)(c * (u128)kPer);
    const long left = ni - i0_want;
    const int cnt_want = (int)(left < kPer ? left : kPer);
    if (expect && (expect[0] != j_want || expect[1] != k_want || expect[2] != i0_want || expect[3] != cnt_want))
        fail("the caller's vector differs from 128-bit arithmetic", kPer, ni, nk, nj, e);
    const AmtChunk wide = amt_chunk_index<kPer>(e, chunks, nk, ni, false);
    const long j = wide.j, k = wide.k, i0 = wide.i0;
    const int cnt = wide.cnt;
    ++checks;
    if (j != j_want || k != k_want || i0 != i0_want || cnt != cnt_want) fail("wide path", kPer, ni, nk, nj, e);
    if (!(j >= 0 && j < nj && k >= 0 && k < nk && i0 >= 0 && i0 < ni && cnt >= 1 && cnt <= kPer && i0 + cnt <= ni && i0 % kPer == 0))
        fail("a result outside its range", kPer, ni, nk, nj, e);
    if ((u128)(((u128)j * (u128)nk + (u128)k) * (u128)chunks + (u128)(i0 / kPer)) != (u128)e) fail("not the inverse", kPer, ni, nk, nj, e);
    if (total <= (u128)0x7fffffffL) {                              // what the kernels call narrow
        const AmtChunk narrow = amt_chunk_index<kPer>(e, chunks, nk, ni, true);
        ++narrow_checks;
        if (narrow.j != j || narrow.k != k || narrow.i0 != i0 || narrow.cnt != cnt) fail("narrow and wide paths differ", kPer, ni, nk, nj, e);
    } else {
        ++wide_only;
    }
}

static void check_any(int per, long ni, long nk, long nj, long e, const long *expect = nullptr)
{
    if (per == 2) check_one<2>(ni, nk, nj, e, expect);
    else check_one<4>(ni, nk, nj, e, expect);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static void check_job(int per, long ni, long nk, long nj)
{
    const long chunks = (ni + per - 1) / per;
    const u128 total128 = (u128)nk * (u128)nj * (u128)chunks;
    if (total128 > ((u128)1 << 62)) return;
    const long total = (long)total128;
    std::vector<long> es = {0, 1, chunks - 1, chunks, chunks + 1, chunks * nk - 1, chunks * nk, chunks * nk + 1, total - 1, total - chunks,
                            total / 2, total / 3};
    for (const long edge : {(1L << 31) - 1, 1L << 31, (1L << 32) - 1, 1L << 32, (1L << 40) - 1, 1L << 40}) {
        for (long d = -2; d <= 2; ++d) es.push_back(edge + d);
        if (edge < total && edge <= (1L << 32)) ++boundaries;
    }
    for (int q = 0; q < 400; ++q) es.push_back((long)(rnd() % (uint64_t)total));
    for (const long e : es)
        if (e >= 0) check_any(per, ni, nk, nj, e);
}

int main(int argc, char **argv)
{
    // jobs on both sides of 2^31 - 1 work items, up to 2^40 and a little past it; row lengths with every tail
    const long nis[] = {1, 2, 3, 4, 5, 7, 8, 9, 17, 63, 64, 65, 602, 4096, 4099};
    const long nks[] = {1, 2, 5, 61, 300};
    const long njs[] = {1, 7, 4096, 1L << 20, (1L << 31) - 1};
    for (const int per : {2, 4})
        for (const long ni : nis)
            for (const long nk : nks)
                for (const long nj : njs) check_job(per, ni, nk, nj);
    // exactly at the threshold: total = 2^31 - 1 (narrow) and 2^31 (wide), one chunk per run, one level
    for (const int per : {2, 4}) {
        check_job(per, 1, 1, (1L << 31) - 1);
        check_job(per, 1, 1, 1L << 31);
        check_job(per, per, 1, 1L << 32);
        check_job(per, 3 * per + 1, 1L << 9, 1L << 29);            // 2^40 work items
        check_job(per, 3 * per + 1, 3, (1L << 31) - 1);
    }
    long vectors = 0;
    if (argc > 1) {
        FILE *f = fopen(argv[1], "r");
        if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        long per, ni, nk, nj, e, expect[4];
        while (fscanf(f, "%ld %ld %ld %ld %ld %ld %ld %ld %ld", &per, &ni, &nk, &nj, &e, &expect[0], &expect[1], &expect[2], &expect[3]) == 9) {
            const long before = checks;
            check_any((int)per, ni, nk, nj, e, expect);
            if (checks == before) fail("a vector outside its job", (int)per, ni, nk, nj, e);
            ++vectors;
        }
        fclose(f);
    }
    printf("chunk index: %ld checks, %ld of them narrow against wide, %ld on jobs too large for the narrow path, %ld boundary samples, "
           "%ld vectors, %ld failures\n", checks, narrow_checks, wide_only, boundaries, vectors, failures);
    return failures ? 1 : 0;
}
