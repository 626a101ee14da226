// Stand-alone host run of the pressure-diagnosis kernel's own text (csrc/amt_p_rho_kernel.h): no HIP call is made.  The header
// is compiled as host C++ behind a few stand-ins -- blockIdx, threadIdx, gridDim, blockDim are globals, readfirstlane is the
// identity, the address-space macro is empty -- and a launch is run as nested loops over members, level groups, blocks and the
// 256 threads of a block, one thread after another: the kernel has no communication between threads, so any order is a valid
// one.  Every array of a call is then compared, WHOLE and as bytes, with a plain loop nest written from the contract
// (include/amt_advance_mu_t.h section 16): one rounding per operation, built with -ffp-contract=off.  Cells the contract does
// not read or write hold a NaN whose payload names array and cell, so a stray write and a stray read both show; every array
// is an allocation that ends with its last element, so the address sanitizer sees what leaves it.
//   p_rho_host_check [-x] cases.txt      lines "dtype ni nk nj members mode step gridDim.x row_phase array_phases idim"
// dtype f32 | f64; row_phase: the elements in front of the run in its memory row; idim: the elements of a memory row;
// array_phases 0: every array starts on a 16-byte boundary, q > 0: array number n starts (n * q) mod P elements behind one.
// -x: name every case in front of its run and stop at the first one that differs.  Exit status 0 = every case equal.  Built and run by tests/test_prho_host.py with the
// address and undefined-behaviour sanitizers, and once per mutant of the header, which must NOT come out equal.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct HostDim3 { unsigned x, y, z; };
static HostDim3 blockIdx, threadIdx, gridDim, blockDim;
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(n)
#define __builtin_amdgcn_readfirstlane(x) (x)
#define AMT_GLOBAL
#include "amt_p_rho_kernel.h"

namespace {
uint64_t mix(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

template <typename T> T poison(int array, size_t cell);
template <> double poison<double>(int array, size_t cell)
{
    const uint64_t u = 0x7FF8000000000000ull | ((uint64_t)(array + 1) << 40) | (uint64_t)(cell + 1);
    double v; memcpy(&v, &u, sizeof v); return v;
}
template <> float poison<float>(int array, size_t cell)
{
    const uint32_t u = 0x7FC00000u | ((uint32_t)(array + 1) << 18) | (uint32_t)((cell % 0x3FFFFu) + 1);
    float v; memcpy(&v, &u, sizeof v); return v;
}

// an array of n elements whose first one sits `phase` elements behind a 16-byte boundary and whose last one ends the allocation
template <typename T>
struct Array {
    T *raw = nullptr, *at = nullptr;
    size_t n = 0, phase = 0;
    void make(size_t n_, size_t phase_, int number)
    {
        n = n_; phase = phase_;
        void *q = nullptr;
        if (posix_memalign(&q, 16, (n + phase) * sizeof(T))) abort();
        raw = static_cast<T *>(q);
        at = raw + phase;
        for (size_t e = 0; e < n + phase; ++e) raw[e] = poison<T>(number, e);
    }
    void copy(const Array &o)
    {
        n = o.n; phase = o.phase;
        void *q = nullptr;
        if (posix_memalign(&q, 16, (n + phase) * sizeof(T))) abort();
        raw = static_cast<T *>(q);
        at = raw + phase;
        memcpy(raw, o.raw, (n + phase) * sizeof(T));
    }
    bool same(const Array &o) const { return memcmp(raw, o.raw, (n + phase) * sizeof(T)) == 0; }
    ~Array() { free(raw); }
};

struct Case {
    char dtype[8];
    long ni, nk, nj, members, mode, step, grid, row_phase, array_phases, idim;
};

const char *const kNames[13] = {"al", "p", "ph", "pm1", "alt", "c2a", "t", "t_old", "mu", "muts", "rdnw", "znu", "dnw"};
const double kRange[13][2] = {{-2, 2}, {-2, 2}, {-50, 50}, {-2, 2}, {0.7, 1.3}, {5, 15}, {-3, 3}, {-5, 5}, {-0.2, 0.2}, {0.8, 1.2},
                              {-9, -4}, {0.05, 0.95}, {-0.3, -0.1}};

// the contract, cell by cell; k ascending inside a column because mode 2 is a recurrence
template <typename T>
void reference(Array<T> *a, const Case &c, long kdim, long jdim, long first3, long first2, T t0, T smdiv)
{
    T *al = a[0].at, *p = a[1].at, *ph = a[2].at, *pm1 = a[3].at;
    const T *alt = a[4].at, *c2a = a[5].at, *t = a[6].at, *told = a[7].at, *mu = a[8].at, *muts = a[9].at;
    const T *rdnw = a[10].at + 1, *znu = a[11].at + 1, *dnw = a[12].at + 1;
    for (long m = 0; m < c.members; ++m)
        for (long j = 0; j < c.nj; ++j)
            for (long k = 0; k < c.nk; ++k)
                for (long i = 0; i < c.ni; ++i) {
                    const long e = m * (c.idim * kdim * jdim) + j * (kdim * c.idim) + k * c.idim + first3 + i, up = e + c.idim;
                    const long e2 = m * (c.idim * jdim) + j * c.idim + first2 + i;
                    const T a1 = mu[e2] * told[e];
                    const T a2 = t[e] - a1;
                    const T num = alt[e] * a2;
                    const T a3 = t0 + told[e];
                    const T den = muts[e2] * a3;
                    const T q = num / den;
                    T x, v;
                    if (c.mode == 1) {
                        const T r = T(-1) / muts[e2];
                        const T b1 = alt[e] * mu[e2];
                        const T b2 = ph[up] - ph[e];
                        const T b3 = rdnw[k] * b2;
                        const T b4 = b1 + b3;
                        v = r * b4;
                        const T b5 = q - v;
                        x = c2a[e] * b5;
                    } else {
                        x = mu[e2] * znu[k];
                        const T b1 = x / c2a[e];
                        v = q - b1;
                        const T b2 = muts[e2] * v;
                        const T b3 = mu[e2] * alt[e];
                        const T b4 = b2 + b3;
                        const T b5 = dnw[k] * b4;
                        ph[up] = ph[e] - b5;
                    }
                    al[e] = v;
                    if (c.step == 0) {
                        p[e] = x;
                    } else {
                        const T d1 = x - pm1[e];
                        const T d2 = smdiv * d1;
                        p[e] = x + d2;
                    }
                    pm1[e] = x;
                }
}

template <typename T, int MODE>
void launch(const AmtPRhoJob<T> &job, unsigned grid, unsigned groups, unsigned members)
{
    gridDim = {grid, groups, members};
    blockDim = {256, 1, 1};
    for (unsigned z = 0; z < members; ++z)
        for (unsigned y = 0; y < groups; ++y)
            for (unsigned x = 0; x < grid; ++x)
                for (unsigned th = 0; th < 256; ++th) {
                    blockIdx = {x, y, z};
                    threadIdx = {th, 0, 0};
                    amt_p_rho_kernel<T, MODE>(job);
                }
}

template <typename T>
bool run(const Case &c, long number)
{
    const long P = 16 / (long)sizeof(T);
    const long kdim = c.nk + 2, jdim = c.nj + 2;                   // one level below kts, level kte on top; a row in front, one behind
    const long first3 = (kdim + 1) * c.idim + c.row_phase, first2 = c.idim + c.row_phase;
    const size_t n3 = (size_t)(c.idim * kdim * jdim * c.members), n2 = (size_t)(c.idim * jdim * c.members), n1 = (size_t)kdim;
    if (c.row_phase + c.ni > c.idim) { fprintf(stderr, "case %ld: the run does not fit its row\n", number); return false; }
    Array<T> got[13], want[13];
    for (int n = 0; n < 13; ++n) got[n].make(n < 8 ? n3 : n < 10 ? n2 : n1, (size_t)((n * c.array_phases) % P), n);
    // finite values where the contract reads: the cells of alt, c2a, t, t_old and, at step != 0, pm1; the columns of mu, muts;
    // ph on kts..kte in mode 1, on kts alone in mode 2; the levels of rdnw in mode 1, of znu and dnw in mode 2
    const auto value = [&](int n, size_t e) {
        const double u = (double)(mix((uint64_t)number * 131 + (uint64_t)n * 0x100000000ull + e) >> 11) * (1.0 / 9007199254740992.0);
        return (T)(kRange[n][0] + (kRange[n][1] - kRange[n][0]) * u);
    };
    for (long m = 0; m < c.members; ++m)
        for (long j = 0; j < c.nj; ++j) {
            for (long k = 0; k <= c.nk; ++k)
                for (long i = 0; i < c.ni; ++i) {
                    const size_t e = (size_t)(m * (c.idim * kdim * jdim) + j * (kdim * c.idim) + k * c.idim + first3 + i);
                    if (k < c.nk) {
                        for (int n = 4; n < 8; ++n) got[n].at[e] = value(n, e);
                        if (c.step != 0) got[3].at[e] = value(3, e);
                    }
                    if (c.mode == 1 || k == 0) got[2].at[e] = value(2, e);
                }
            for (long i = 0; i < c.ni; ++i) {
                const size_t e = (size_t)(m * (c.idim * jdim) + j * c.idim + first2 + i);
                got[8].at[e] = value(8, e);
                got[9].at[e] = value(9, e);
            }
        }
    for (long k = 0; k < c.nk; ++k) {
        if (c.mode == 1) got[10].at[1 + k] = value(10, (size_t)k);
        else { got[11].at[1 + k] = value(11, (size_t)k); got[12].at[1 + k] = value(12, (size_t)k); }
    }
    for (int n = 0; n < 13; ++n) want[n].copy(got[n]);
    const T t0 = (T)300.0, smdiv = (T)0.1;
    reference<T>(want, c, kdim, jdim, first3, first2, t0, smdiv);

    AmtPRhoJob<T> job{};
    job.al = got[0].at; job.p = got[1].at; job.ph = got[2].at; job.pm1 = got[3].at;
    job.alt = got[4].at; job.c2a = got[5].at; job.t = got[6].at; job.t_old = got[7].at; job.mu = got[8].at; job.muts = got[9].at;
    job.rdnw = got[10].at + 1; job.znu = got[11].at + 1; job.dnw = got[12].at + 1;
    job.ni = (int)c.ni; job.nk = (int)c.nk; job.nj = (int)c.nj;
    job.idim = c.idim; job.jstride3 = kdim * c.idim; job.mstride3 = c.idim * kdim * jdim; job.mstride2 = c.idim * jdim;
    job.first3 = first3; job.first2 = first2;
    job.t0 = t0; job.smdiv = smdiv;
    job.step0 = c.step == 0;
    if (c.mode == 1) launch<T, 1>(job, (unsigned)c.grid, (unsigned)((c.nk + AMT_P_RHO_GROUP - 1) / AMT_P_RHO_GROUP), (unsigned)c.members);
    else launch<T, 2>(job, (unsigned)c.grid, 1, (unsigned)c.members);

    bool ok = true;
    for (int n = 0; n < 13; ++n)
        if (!got[n].same(want[n])) {
            size_t e = 0;
            while (memcmp(got[n].raw + e, want[n].raw + e, sizeof(T)) == 0) ++e;
            fprintf(stderr, "case %ld: %s differs, first at element %ld of %zu\n", number, kNames[n], (long)e - (long)got[n].phase, got[n].n);
            ok = false;
        }
    return ok;
}
}  // namespace

int main(int argc, char **argv)
{
    bool stop = false;
    const char *path = nullptr;
    for (int k = 1; k < argc; ++k) {
        if (!strcmp(argv[k], "-x")) stop = true;
        else path = argv[k];
    }
    FILE *f = path ? fopen(path, "r") : nullptr;
    if (!f) { fprintf(stderr, "usage: p_rho_host_check [-x] cases.txt\n"); return 2; }
    long cases = 0, failures = 0;
    Case c;
    int got;
    while ((got = fscanf(f, "%7s %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld", c.dtype, &c.ni, &c.nk, &c.nj, &c.members, &c.mode, &c.step, &c.grid,
                         &c.row_phase, &c.array_phases, &c.idim)) == 11) {
        const bool wide = !strcmp(c.dtype, "f64");
        if ((!wide && strcmp(c.dtype, "f32")) || c.ni < 1 || c.nk < 1 || c.nj < 1 || c.members < 1 || (c.mode != 1 && c.mode != 2) || c.step < 0 ||
            c.grid < 1 || c.row_phase < 0 || c.array_phases < 0) {
            fprintf(stderr, "case %ld: not a case\n", cases);
            return 2;
        }
        if (stop) {                                                // what a sanitizer report then stands behind
            printf("case %ld: %s %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld\n", cases, c.dtype, c.ni, c.nk, c.nj, c.members, c.mode, c.step, c.grid,
                   c.row_phase, c.array_phases, c.idim);
            fflush(stdout);
        }
        const bool ok = wide ? run<double>(c, cases) : run<float>(c, cases);
        if (!ok) {
            if (failures++ < 20)
                fprintf(stderr, "FAILED %s %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld\n", c.dtype, c.ni, c.nk, c.nj, c.members, c.mode, c.step, c.grid,
                        c.row_phase, c.array_phases, c.idim);
            if (stop) break;
        }
        ++cases;
    }
    fclose(f);
    if (got != EOF && got != 11) { fprintf(stderr, "a line that is no case behind case %ld\n", cases); return 2; }
    printf("p_rho host check: %ld cases, %ld failures\n", cases, failures);
    return failures ? 1 : 0;
}
