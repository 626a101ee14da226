// Stand-alone host run of the momentum update's own kernel text (csrc/amt_uv_kernel.h): no HIP call is made.  The header is
// compiled as host C++ behind a few stand-ins -- blockIdx, threadIdx, gridDim, blockDim are globals, readfirstlane is the
// identity, the address-space macros are empty, the job is read where it lies -- and a launch is run as nested loops over
// members, parts and level groups, blocks and the 256 threads of a block, one thread after another: the kernel has no
// communication between threads, so any order is a valid one.  Every array of a call is then compared, WHOLE and as bytes,
// with a plain loop nest written from the contract (include/amt_advance_mu_t.h section 17): one rounding per operation, built
// with -ffp-contract=off.  Cells the contract neither reads nor writes hold a NaN whose payload names array and cell, so a
// stray write and a stray read both show; every array is an allocation that ends with its last element -- the last cell the
// call reads when the run ends its memory row -- so the address sanitizer sees what leaves it.
//   uv_host_check [-x] cases.txt      lines "dtype ni nk nj members nh gridDim.x row_phase array_phases idim shrink"
// dtype f32 | f64; nh: 1 non-hydrostatic; row_phase: the elements in front of the neighbour column in its memory row; idim: the
// elements of a memory row; array_phases 0: every array starts on a 16-byte boundary, q > 0: array number n starts (n * q) mod
// P elements behind one; shrink: the u part has `shrink` rows less, the v part `shrink` columns less (the whole-domain tile).
// -x: name every case in front of its run and stop at the first one that differs.  Exit status 0 = every case equal.
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
#define AMT_UV_CONST
#define AMT_UV_FRESH(q) ((void)0)
#define AMT_UV_JOB(T, job) (&(job))
#include "amt_uv_kernel.h"

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
    const uint32_t u = 0x7FC00000u | ((uint32_t)(array + 1) << 17) | (uint32_t)((cell % 0x1FFFFu) + 1);
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
    long ni, nk, nj, members, nh, grid, row_phase, array_phases, idim, shrink;
};

// the argument order of amt_advance_uv_device_*
enum { U, V, RU, RV, P, PB, PH, PHP, ALT, AL, MU, MUU, MUV, MUDF, CQU, CQV, MSFUX, MSFUY, MSFVX, MSFVXI, MSFVY, FNM, FNP, RDNW, NARR };
const char *const kNames[NARR] = {"u", "v", "ru_tend", "rv_tend", "p", "pb", "ph", "php", "alt", "al", "mu", "muu", "muv", "mudf", "cqu", "cqv",
                                  "msfux", "msfuy", "msfvx", "msfvx_inv", "msfvy", "fnm", "fnp", "rdnw"};
int rank_of(int n) { return n >= FNM ? 1 : (n >= MU && n <= MUDF) || (n >= MSFUX && n <= MSFVY) ? 2 : 3; }

template <typename T>
struct Scalars { T rdx, rdy, dts, cf1, cf2, cf3, emdiv; };

// One part of the contract, cell by cell.  (di, dj): where the neighbour lies.  Elements are counted from the first cell of
// the tile: first3 / first2 behind the array's start.
template <typename T>
void reference_part(Array<T> *a, const Case &c, long kdim, long jdim, long first3, long first2, const Scalars<T> &s, int part,
                    std::vector<T> &result)
{
    const long ni = part == 0 ? c.ni : c.ni - c.shrink, nj = part == 0 ? c.nj - c.shrink : c.nj;
    const long js3 = kdim * c.idim, nb3 = part == 0 ? 1 : js3, nb2 = part == 0 ? 1 : c.idim;
    const T *out = a[part == 0 ? U : V].at, *tend = a[part == 0 ? RU : RV].at, *cq = a[part == 0 ? CQU : CQV].at;
    const T *mass = a[part == 0 ? MUU : MUV].at, *num = a[part == 0 ? MSFUX : MSFVY].at, *den = a[part == 0 ? MSFUY : MSFVX].at;
    const T *p = a[P].at, *pb = a[PB].at, *ph = a[PH].at, *php = a[PHP].at, *alt = a[ALT].at, *al = a[AL].at, *mu = a[MU].at, *mudf = a[MUDF].at;
    const T *fnm = a[FNM].at + 1, *fnp = a[FNP].at + 1, *rdnw = a[RDNW].at + 1;
    const T rd = part == 0 ? s.rdx : s.rdy, half = T(0.5);
    const T dd = T(1) / rd;
    const T scale = (-s.emdiv) * dd;
    std::vector<T> dpn((size_t)c.nk + 1);
    for (long m = 0; m < c.members; ++m)
        for (long j = 0; j < nj; ++j)
            for (long i = 0; i < ni; ++i) {
                const long e2 = m * (c.idim * jdim) + j * c.idim + first2 + i, n2 = e2 - nb2;
                const long col = m * (c.idim * kdim * jdim) + j * js3 + first3 + i;
                const T mr = num[e2] / den[e2];
                const T c1 = mr * half;
                const T c2 = c1 * rd;
                const T cc = c2 * mass[e2];
                const T d1 = mudf[e2] - mudf[n2];
                const T d2 = scale * d1;
                const T md = part == 0 ? d2 / a[MSFUY].at[e2] : d2 * a[MSFVXI].at[e2];
                T mrd = T(0), hm = T(0);
                if (c.nh) {
                    mrd = mr * rd;
                    const T ms = mu[n2] + mu[e2];
                    hm = half * ms;
                    const auto sk = [&](long k) { const long e = col + k * c.idim; return (T)(p[e] + p[e - nb3]); };
                    const T t1 = s.cf1 * sk(0), t2 = s.cf2 * sk(1), t3 = s.cf3 * sk(2);
                    const T t4 = t1 + t2;
                    const T t5 = t4 + t3;
                    dpn[0] = half * t5;
                    for (long k = 1; k < c.nk; ++k) {
                        const T f1 = fnm[k] * sk(k), f2 = fnp[k] * sk(k - 1);
                        const T f3 = f1 + f2;
                        dpn[(size_t)k] = half * f3;
                    }
                    dpn[(size_t)c.nk] = T(0);
                }
                for (long k = 0; k < c.nk; ++k) {
                    const long e = col + k * c.idim, n = e - nb3, up = e + c.idim, nup = up - nb3;
                    const T g1 = ph[up] - ph[nup], g2 = ph[e] - ph[n];
                    const T g3 = g1 + g2;
                    const T a1 = alt[e] + alt[n], a2 = p[e] - p[n];
                    const T a3 = a1 * a2;
                    const T g4 = g3 + a3;
                    const T b1 = al[e] + al[n], b2 = pb[e] - pb[n];
                    const T b3 = b1 * b2;
                    const T g = g4 + b3;
                    T dpxy = cc * g;
                    if (c.nh) {
                        const T w1 = php[e] - php[n];
                        const T w = mrd * w1;
                        const T e1 = dpn[(size_t)k + 1] - dpn[(size_t)k];
                        const T e2_ = rdnw[k] * e1;
                        const T e3 = e2_ - hm;
                        const T we = w * e3;
                        dpxy = dpxy + we;
                    }
                    const T x1 = s.dts * tend[e];
                    const T x2 = out[e] + x1;
                    const T y1 = s.dts * cq[e];
                    const T y2 = y1 * dpxy;
                    const T x3 = x2 - y2;
                    result.push_back(x3 + md);
                }
            }
}

template <typename T>
void reference(Array<T> *a, const Case &c, long kdim, long jdim, long first3, long first2, const Scalars<T> &s)
{
    for (int part = 0; part < 2; ++part) {
        std::vector<T> result;
        reference_part<T>(a, c, kdim, jdim, first3, first2, s, part, result);
        const long ni = part == 0 ? c.ni : c.ni - c.shrink, nj = part == 0 ? c.nj - c.shrink : c.nj;
        T *out = a[part == 0 ? U : V].at;
        size_t r = 0;
        for (long m = 0; m < c.members; ++m)
            for (long j = 0; j < nj; ++j)
                for (long i = 0; i < ni; ++i)
                    for (long k = 0; k < c.nk; ++k)
                        out[m * (c.idim * kdim * jdim) + j * (kdim * c.idim) + k * c.idim + first3 + i] = result[r++];
    }
}

template <typename T, bool NH>
void launch(AmtUvJob<T> &job, unsigned grid, unsigned groups, unsigned members)
{
    gridDim = {grid, 2 * groups, members};
    blockDim = {256, 1, 1};
    for (unsigned z = 0; z < members; ++z)
        for (unsigned y = 0; y < 2 * groups; ++y)
            for (unsigned x = 0; x < grid; ++x)
                for (unsigned th = 0; th < 256; ++th) {
                    blockIdx = {x, y, z};
                    threadIdx = {th, 0, 0};
                    amt_uv_kernel<T, NH>(job);
                }
}

template <typename T>
bool run(const Case &c, long number)
{
    const long per = 16 / (long)sizeof(T);
    const long kdim = c.nk + 2, jdim = c.nj + 1;                   // one level below kts, level kte on top; one row in front
    const long first3 = (kdim + 1) * c.idim + c.row_phase + 1, first2 = c.idim + c.row_phase + 1;
    const size_t n3 = (size_t)(c.idim * kdim * jdim * c.members), n2 = (size_t)(c.idim * jdim * c.members), n1 = (size_t)kdim;
    if (c.row_phase + 1 + c.ni > c.idim) { fprintf(stderr, "case %ld: the run does not fit its row\n", number); return false; }
    Array<T> got[NARR], want[NARR];
    for (int n = 0; n < NARR; ++n) got[n].make(rank_of(n) == 3 ? n3 : rank_of(n) == 2 ? n2 : n1, (size_t)((n * c.array_phases) % per), n);
    const auto value = [&](int n, size_t e) {
        const double u = (double)(mix((uint64_t)number * 131 + (uint64_t)n * 0x100000000ull + e) >> 11) * (1.0 / 9007199254740992.0);
        const bool positive = n == MUU || n == MUV || n >= MSFUX;
        return (T)(positive ? 0.5 + u : -2.0 + 4.0 * u);
    };
    // finite values where the contract reads: per part the cells and their neighbours
    for (int part = 0; part < 2; ++part) {
        const long ni = part == 0 ? c.ni : c.ni - c.shrink, nj = part == 0 ? c.nj - c.shrink : c.nj;
        const int own3[3] = {part == 0 ? U : V, part == 0 ? RU : RV, part == 0 ? CQU : CQV};
        const int own2[4] = {part == 0 ? MUU : MUV, part == 0 ? MSFUX : MSFVY, part == 0 ? MSFUY : MSFVX, part == 0 ? MSFUY : MSFVXI};
        const int both3[6] = {P, PB, PH, PHP, ALT, AL}, both2[2] = {MU, MUDF};
        for (long m = 0; m < c.members; ++m)
            for (long j = 0; j < nj; ++j)
                for (long i = 0; i < ni; ++i) {
                    const long e2 = m * (c.idim * jdim) + j * c.idim + first2 + i, n2_ = e2 - (part == 0 ? 1 : c.idim);
                    for (int n : own2) got[n].at[e2] = value(n, (size_t)e2);
                    for (int n : both2) {
                        if (n == MU && !c.nh) continue;
                        got[n].at[e2] = value(n, (size_t)e2);
                        got[n].at[n2_] = value(n, (size_t)n2_);
                    }
                    for (long k = 0; k <= c.nk; ++k) {
                        const long e = m * (c.idim * kdim * jdim) + j * (kdim * c.idim) + k * c.idim + first3 + i;
                        const long nb = e - (part == 0 ? 1 : kdim * c.idim);
                        if (k < c.nk)
                            for (int n : own3) got[n].at[e] = value(n, (size_t)e);
                        for (int n : both3) {
                            if ((n == PHP && !c.nh) || (n != PH && k == c.nk)) continue;
                            got[n].at[e] = value(n, (size_t)e);
                            got[n].at[nb] = value(n, (size_t)nb);
                        }
                    }
                }
    }
    if (c.nh)
        for (long k = 0; k < c.nk; ++k) {
            got[RDNW].at[1 + k] = value(RDNW, (size_t)k);
            if (k > 0) { got[FNM].at[1 + k] = value(FNM, (size_t)k); got[FNP].at[1 + k] = value(FNP, (size_t)k); }
        }
    for (int n = 0; n < NARR; ++n) want[n].copy(got[n]);
    const Scalars<T> s = {(T)1.0e-3, (T)1.25e-3, (T)2.0, (T)1.5, (T)-0.75, (T)0.25, (T)0.01};
    reference<T>(want, c, kdim, jdim, first3, first2, s);

    AmtUvJob<T> job{};
    const T dx = T(1) / s.rdx, dy = T(1) / s.rdy;
    AmtUvPart<T> &pu = job.part[0], &pv = job.part[1];
    pu.out = got[U].at; pu.tend = got[RU].at; pu.cq = got[CQU].at; pu.mass = got[MUU].at;
    pu.msf_num = got[MSFUX].at; pu.msf_den = got[MSFUY].at; pu.msf_md = got[MSFUY].at; pu.rd = s.rdx; pu.md_scale = (-s.emdiv) * dx;
    pv.out = got[V].at; pv.tend = got[RV].at; pv.cq = got[CQV].at; pv.mass = got[MUV].at;
    pv.msf_num = got[MSFVY].at; pv.msf_den = got[MSFVX].at; pv.msf_md = got[MSFVXI].at; pv.rd = s.rdy; pv.md_scale = (-s.emdiv) * dy;
    pu.ni = (int)c.ni; pu.nj = (int)(c.nj - c.shrink); pv.ni = (int)(c.ni - c.shrink); pv.nj = (int)c.nj;
    job.p = got[P].at; job.pb = got[PB].at; job.ph = got[PH].at; job.php = got[PHP].at; job.alt = got[ALT].at; job.al = got[AL].at;
    job.mu = got[MU].at; job.mudf = got[MUDF].at; job.fnm = got[FNM].at + 1; job.fnp = got[FNP].at + 1; job.rdnw = got[RDNW].at + 1;
    job.nk = (int)c.nk;
    job.idim = c.idim; job.jstride3 = kdim * c.idim; job.mstride3 = c.idim * kdim * jdim; job.mstride2 = c.idim * jdim;
    job.first3 = first3; job.first2 = first2;
    job.dts = s.dts; job.cf1 = s.cf1; job.cf2 = s.cf2; job.cf3 = s.cf3;
    const unsigned groups = (unsigned)((c.nk + AMT_UV_GROUP - 1) / AMT_UV_GROUP);
    if (c.nh) launch<T, true>(job, (unsigned)c.grid, groups, (unsigned)c.members);
    else launch<T, false>(job, (unsigned)c.grid, groups, (unsigned)c.members);

    bool ok = true;
    for (int n = 0; n < NARR; ++n)
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
    if (!f) { fprintf(stderr, "usage: uv_host_check [-x] cases.txt\n"); return 2; }
    long cases = 0, failures = 0;
    Case c;
    int got;
    while ((got = fscanf(f, "%7s %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld", c.dtype, &c.ni, &c.nk, &c.nj, &c.members, &c.nh, &c.grid, &c.row_phase,
                         &c.array_phases, &c.idim, &c.shrink)) == 11) {
        const bool wide = !strcmp(c.dtype, "f64");
        if ((!wide && strcmp(c.dtype, "f32")) || c.ni < 1 || c.nk < 1 || c.nj < 1 || c.members < 1 || (c.nh && c.nk < 3) || c.grid < 1 ||
            c.row_phase < 0 || c.array_phases < 0 || c.shrink < 0 || c.shrink > 1) {
            fprintf(stderr, "case %ld: not a case\n", cases);
            return 2;
        }
        if (stop) {
            printf("case %ld: %s %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld\n", cases, c.dtype, c.ni, c.nk, c.nj, c.members, c.nh, c.grid, c.row_phase,
                   c.array_phases, c.idim, c.shrink);
            fflush(stdout);
        }
        const bool ok = wide ? run<double>(c, cases) : run<float>(c, cases);
        if (!ok) {
            if (failures++ < 20)
                fprintf(stderr, "FAILED %s %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld\n", c.dtype, c.ni, c.nk, c.nj, c.members, c.nh, c.grid, c.row_phase,
                        c.array_phases, c.idim, c.shrink);
            if (stop) break;
        }
        ++cases;
    }
    fclose(f);
    if (got != EOF && got != 11) { fprintf(stderr, "a line that is no case behind case %ld\n", cases); return 2; }
    printf("uv host check: %ld cases, %ld failures\n", cases, failures);
    return failures ? 1 : 0;
}
