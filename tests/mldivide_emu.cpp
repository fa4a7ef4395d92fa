// Stand-alone host program (its own main, CPU only): csrc/mldivide.hpp, the kernel's SOURCE, compiled for the host and run by
// 256 lock-stepped threads per workgroup -- __syncthreads goes through a std::barrier, the workgroup's LDS is one static array
// of the device's 160 KiB -- against tests/mldivide_ref.c (linked in), bit for bit, NaN matching NaN.  It checks the kernel's
// arithmetic order, the ownership of columns and rows by the lane groups over one and several rounds of 32 columns, the
// indexing, the barrier discipline (a lane that left a loop alone would leave the others waiting; a value read after another
// lane rewrote it would differ) and the launch slices over the row counts and the items without a GPU; it says nothing about
// the device's sqrt / division / fma.  Built and run by tests/test_mldivide_emu.py; by hand (optionally with
// -fsanitize=address,undefined for the index checks):
//   gcc -O2 -ffp-contract=off -c tests/mldivide_ref.c -o ref.o
//   g++ -std=c++20 -O1 -ffp-contract=off -Iepidemicmodeling_amd/csrc tests/mldivide_emu.cpp ref.o -o emu -lpthread && ./emu
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

struct Dim { unsigned x; };
static thread_local Dim threadIdx, blockIdx;
static std::barrier<> *group;
#define __global__
#define __launch_bounds__(x)
#define __shared__
#define EPI_DEV static inline
static void __syncthreads() { group->arrive_and_wait(); }
double ml_lds[20480];              // the workgroup's dynamic LDS: 160 KiB
using std::fma;
#include "mldivide.hpp"

extern "C" void mldivide_run(const double *X, const double *y, const int32_t *n_rows, int D, int F, int R, int K, double tol_scale,
                             double *m_out, int32_t *rank_out, int32_t *perm_out, double *rdiag_out, double *resid_out,
                             double *fitted_out, int32_t *status_out);
extern "C" long ml_recomputed_pub(void);
extern "C" long ml_ties_pub(void);

static void launch(unsigned blocks, MlArgs g)
{
    for (unsigned b = 0; b < blocks; b++) {
        std::barrier<> bar(kMlThreads);
        group = &bar;
        std::vector<std::thread> lanes;
        for (unsigned l = 0; l < (unsigned)kMlThreads; l++) lanes.emplace_back([=] { threadIdx.x = l; blockIdx.x = b; mldivide_items(g); });
        for (auto &t : lanes) t.join();
    }
}

static double rnd() { return (double)rand() / RAND_MAX; }
static size_t differ(const double *a, const double *b, size_t n)
{
    size_t bad = 0;
    for (size_t k = 0; k < n; k++) bad += memcmp(a + k, b + k, 8) != 0 && !(std::isnan(a[k]) && std::isnan(b[k]));
    return bad;
}

// nr: the row counts; counts: row counts carried per launch (the library's 64; 2 here exercises the slices); slice: workgroups
// per launch
struct Case { int D, F, K, R, nr[3], counts, slice; };

int main()
{
    const Case cases[] = {{1, 1, 1, 1, {1}, 64, 1 << 20},       {6, 5, 2, 4, {3, 5}, 64, 1 << 20},   {9, 2, 1, 3, {7}, 64, 1 << 20},
                          {257, 3, 3, 2, {255, 256, 257}, 64, 1 << 20}, {206, 96, 1, 2, {206}, 64, 1 << 20}, {400, 49, 1, 2, {400}, 64, 1 << 20},
                          {12, 7, 3, 5, {1, 7, 12}, 2, 3}};
    size_t total = 0, seen = 0;
    for (const Case &c : cases) {
        const int D = c.D, F = c.F, K = c.K, R = c.R;
        std::vector<double> X((size_t)D * F * R), y((size_t)D * R);
        for (int r = 0; r < R; r++)
            for (int f = 0; f < F; f++) {
                int lvl = rand() % 5;
                for (int t = 0; t < D; t++) {
                    if (rnd() < 0.1) lvl = rand() % 5;
                    X[((size_t)t * F + f) * R + r] = lvl;
                }
            }
        for (auto &v : y) v = 0.4 * (rnd() - 0.5);
        // region 0: a duplicated and a zero column (F >= 3), an exactly cancelled one; region 1: a NaN; region 2: an overflow
        if (F >= 3)
            for (int t = 0; t < D; t++) {
                X[((size_t)t * F + 2) * R] = X[((size_t)t * F) * R];
                X[((size_t)t * F + 1) * R] = 0.0;
            }
        if (F >= 5)
            for (int t = 0; t < D; t++) X[((size_t)t * F + 4) * R] = X[((size_t)t * F) * R] * (1.0 + 1e-9 * t) + 1e-7 * X[((size_t)t * F + 3) * R];
        if (R > 1) X[1] = NAN;
        if (R > 2) for (int t = 0; t < D; t++) X[((size_t)t * F) * R + 2] = 1e200 * (t + 1);
        const size_t NM = (size_t)K * F * R, NK = (size_t)K * R, NF = (size_t)K * D * R;
        std::vector<double> m1(NM, -7), m2 = m1, d1(NM, -7), d2 = d1, r1(NK, -7), r2 = r1, f1(NF, -7), f2 = f1;
        std::vector<int32_t> k1(NK, -7), k2 = k1, p1(NM, -7), p2 = p1, s1(NK, -7), s2 = s1;
        mldivide_run(X.data(), y.data(), c.nr, D, F, R, K, 1.0, m1.data(), k1.data(), p1.data(), d1.data(), r1.data(), f1.data(), s1.data());
        MlArgs g{};
        g.D = D; g.F = F; g.R = R; g.tol_scale = 1.0; g.X = X.data(); g.y = y.data();
        g.m = m2.data(); g.rank = k2.data(); g.perm = p2.data(); g.rdiag = d2.data(); g.resid = r2.data(); g.fitted = f2.data(); g.status = s2.data();
        for (int k0 = 0; k0 < K; k0 += c.counts) {                          // the launch loops of epi_mldiv_run_device
            const int kc = K - k0 < c.counts ? K - k0 : c.counts;
            g.k0 = k0;
            int nmax = 0;
            for (int kk = 0; kk < kc; kk++) { g.nr[kk] = c.nr[k0 + kk]; nmax = g.nr[kk] > nmax ? g.nr[kk] : nmax; }
            if (ml_lds_bytes(nmax, F) > sizeof ml_lds) { printf("LDS of n=%d F=%d does not fit\n", nmax, F); return 2; }
            const long long items = (long long)kc * R;
            for (long long i0 = 0; i0 < items; i0 += c.slice) {
                g.item0 = i0;
                launch((unsigned)(items - i0 < c.slice ? items - i0 : c.slice), g);
            }
        }
        size_t bad = differ(m1.data(), m2.data(), NM) + differ(d1.data(), d2.data(), NM) + differ(r1.data(), r2.data(), NK) + differ(f1.data(), f2.data(), NF) +
                     (memcmp(k1.data(), k2.data(), 4 * NK) != 0) + (memcmp(p1.data(), p2.data(), 4 * NM) != 0) + (memcmp(s1.data(), s2.data(), 4 * NK) != 0);
        int bits = 0;
        for (int32_t v : s1) bits |= v;
        seen |= (size_t)bits;
        printf("D=%d F=%d K=%d R=%d n_rows=%d..: differing values %zu  (status bits seen %d, rank[0] %d)\n", D, F, K, R, c.nr[0], bad, bits, k1[0]);
        total += bad;
    }
    printf("cases %zu, status bits seen %zu, recomputed norms %ld, ties %ld, differing values %zu\n", sizeof cases / sizeof cases[0], seen,
           ml_recomputed_pub(), ml_ties_pub(), total);
    return total != 0 || seen != 7 || ml_recomputed_pub() == 0 || ml_ties_pub() == 0;
}
