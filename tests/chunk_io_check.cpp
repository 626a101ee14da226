// Stand-alone host check of the chunk load and store the streaming kernels share (csrc/amt_chunk_io.h): no HIP call is made.
// For float and double, every cnt in 0..kPer, every element phase of the chunk's start behind a 16-byte boundary, and `wide`
// true only for a whole chunk on a boundary (and false there as well):
//   * a load returns the elements < cnt, bit for bit, and +0.0 in the lanes behind them;
//   * a store changes exactly the elements < cnt: the rest of the buffer, guards on both sides included, keeps its bytes.
// Each case runs twice: in a buffer with kPer guard elements on both sides of a whole chunk's room, and in an allocation that
// ENDS with element cnt - 1, so that the address sanitizer sees an access behind cnt.  Built and run by
// tests/test_chunk_index.py with the address and undefined-behaviour sanitizers on; exit status 0 = all held.
#include "amt_chunk_io.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static long failures = 0, loads = 0, stores = 0, wides = 0;

static void fail(const char *what, int bytes, int cnt, int phase, bool wide, bool exact)
{
    if (failures++ < 20) fprintf(stderr, "%s: %d-byte elements, cnt %d, phase %d, wide %d, %s buffer\n", what, bytes, cnt, phase, (int)wide, exact ? "exact" : "guarded");
}

// element e of a buffer: a NaN whose payload names it, so that no two elements and no zero look alike
template <typename T> static T mark(unsigned salt, unsigned e)
{
    T v;
    if (sizeof(T) == 8) { const uint64_t u = 0x7FF8000000000000ull | ((uint64_t)salt << 16) | (e + 1); memcpy(&v, &u, sizeof v); }
    else { const uint32_t u = 0x7FC00000u | (salt << 8) | (e + 1); memcpy(&v, &u, sizeof v); }
    return v;
}

// `front` elements, then the chunk, then `back` elements, in an allocation on a 16-byte boundary that ends with the last one
template <typename T> struct Buffer {
    T *raw;
    size_t n;
    Buffer(size_t n_, unsigned salt) : raw(nullptr), n(n_)
    {
        void *q = nullptr;
        if (posix_memalign(&q, 16, n * sizeof(T))) abort();
        raw = static_cast<T *>(q);
        for (size_t e = 0; e < n; ++e) raw[e] = mark<T>(salt, (unsigned)e);
    }
    ~Buffer() { free(raw); }
    bool is(size_t e, T v) const { return memcmp(raw + e, &v, sizeof v) == 0; }
};

template <typename T>
static void check_case(int cnt, int phase, bool wide, bool exact)
{
    typedef typename AmtVec16<T>::type V;
    constexpr int kPer = 16 / (int)sizeof(T);
    // guarded: a whole 16-byte block of guards in front, the phase, room for a whole chunk, kPer guards behind
    const size_t front = exact ? (size_t)phase : (size_t)(kPer + phase), back = exact ? 0 : (size_t)(kPer - cnt + kPer);
    const size_t n = front + (size_t)cnt + back;
    const T zero = T(0);
    {
        Buffer<T> src(n, 1);
        const V v = amt_chunk_load<T>(src.raw + front, wide, cnt);
        ++loads;
        for (int i = 0; i < kPer; ++i) {
            const T got = v[i];
            const T want = i < cnt ? src.raw[front + i] : zero;
            if (memcmp(&got, &want, sizeof got)) fail(i < cnt ? "a loaded element differs" : "a lane behind cnt is not +0.0", (int)sizeof(T), cnt, phase, wide, exact);
        }
        for (size_t e = 0; e < n; ++e)
            if (!src.is(e, mark<T>(1, (unsigned)e))) fail("a load changed its source", (int)sizeof(T), cnt, phase, wide, exact);
    }
    {
        Buffer<T> dst(n, 2);
        V v;
        for (int i = 0; i < kPer; ++i) v[i] = mark<T>(3, (unsigned)i);
        amt_chunk_store<T>(dst.raw + front, wide, cnt, v);
        ++stores;
        for (size_t e = 0; e < n; ++e) {
            const bool inside = e >= front && e < front + (size_t)cnt;
            if (!dst.is(e, inside ? mark<T>(3, (unsigned)(e - front)) : mark<T>(2, (unsigned)e)))
                fail(inside ? "a stored element differs" : "a store changed an element outside the chunk", (int)sizeof(T), cnt, phase, wide, exact);
        }
    }
    if (wide) ++wides;
}

template <typename T>
static void check_type()
{
    constexpr int kPer = 16 / (int)sizeof(T);
    for (int cnt = 0; cnt <= kPer; ++cnt)
        for (int phase = 0; phase < kPer; ++phase)
            for (int exact = 0; exact < 2; ++exact) {
                check_case<T>(cnt, phase, false, exact != 0);
                if (cnt == kPer && phase == 0) check_case<T>(cnt, phase, true, exact != 0);     // what a caller may call wide
            }
}

int main()
{
    check_type<float>();
    check_type<double>();
    printf("chunk io: %ld loads, %ld stores, %ld of the cases wide, %ld failures\n", loads, stores, wides, failures);
    return failures ? 1 : 0;
}
