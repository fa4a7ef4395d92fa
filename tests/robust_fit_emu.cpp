// Stand-alone host program (its own main, CPU only): csrc/robust_fit.hpp, the kernels' SOURCE (with the ens_tree / ens_sort /
// ens_pick of csrc/ens_summary.hpp it includes), compiled for the host and run by 64 lock-stepped threads per workgroup --
// __shfl, __shfl_xor and __ballot go through a std::barrier -- against tests/robust_fit_ref.c (linked in), bit for bit, NaN
// matching NaN.  It checks the kernels' arithmetic order, indexing and the wave-uniform loop exit (a lane that left the loop
// alone would leave the others waiting at the barrier) without a GPU; it says nothing about the device's sqrt / division.
// Built and run by tests/test_robust_fit_emu.py; by hand (optionally with -fsanitize=address,undefined for the index checks):
//   gcc -O2 -ffp-contract=off -c tests/robust_fit_ref.c -o ref.o
//   g++ -std=c++20 -O1 -ffp-contract=off -Iepidemicmodeling_amd/csrc tests/robust_fit_emu.cpp ref.o -o emu -lpthread && ./emu
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
static std::barrier<> *wave;
// one barrier per exchange: the lanes alternate between two buffers, and a lane can reach its next write to a buffer only
// through the barrier of the exchange in between, which every lane passes after it has read this one
static double lane_f64[2][64];
static int lane_pred[2][64];
static thread_local unsigned exchange;
#define __global__
#define __launch_bounds__(x)
#define EPI_DEV static inline
static double __shfl_xor(double v, int h)
{
    const unsigned b = exchange++ & 1;
    lane_f64[b][threadIdx.x] = v;
    wave->arrive_and_wait();
    return lane_f64[b][threadIdx.x ^ (unsigned)h];
}
static double __shfl(double v, int src)
{
    const unsigned b = exchange++ & 1;
    lane_f64[b][threadIdx.x] = v;
    wave->arrive_and_wait();
    return lane_f64[b][src];
}
static unsigned long long __ballot(int p)
{
    const unsigned b = exchange++ & 1;
    lane_pred[b][threadIdx.x] = p != 0;
    wave->arrive_and_wait();
    unsigned long long m = 0;
    for (int l = 0; l < 64; l++) if (lane_pred[b][l]) m |= 1ull << l;
    return m;
}
static int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
// the launch helpers of the two headers are not used here: the names they mention only have to exist
typedef int hipError_t;
typedef void *hipStream_t;
struct dim3 { dim3(unsigned) {} };
static hipError_t hipGetLastError() { return 0; }
#define hipLaunchKernelGGL(...) ((void)0)
#include "robust_fit.hpp"

extern "C" void robfit_run(const double *X, const double *y, int R, int D, int n, int robust, int max_iter, double lower, double upper,
                           double *a, double *b_item, double *sigma, int32_t *iters, int32_t *status, double *weights, double *b);

template <class F> static void launch(F kernel, unsigned blocks, RfArgs g)
{
    for (unsigned b = 0; b < blocks; b++) {
        std::barrier<> bar(64);
        wave = &bar;
        std::vector<std::thread> lanes;
        for (unsigned l = 0; l < 64; l++) lanes.emplace_back([=] { threadIdx.x = l; blockIdx.x = b; kernel(g); });
        for (auto &t : lanes) t.join();
    }
}

template <int NV> static void run(RfArgs g, bool items)
{
    if (items) launch(robfit_items<NV>, (unsigned)(g.n * g.R), g);
    if (g.b) launch(robfit_intercept<NV>, (unsigned)g.R, g);
}

static double rnd() { return (double)rand() / RAND_MAX; }
static size_t differ(const double *a, const double *b, size_t n)
{
    size_t bad = 0;
    for (size_t k = 0; k < n; k++) bad += memcmp(a + k, b + k, 8) != 0 && !(std::isnan(a[k]) && std::isnan(b[k]));
    return bad;
}

// items = 0: only b is requested, so robfit_intercept fits the items itself
struct Case { int R, D, n, robust, max_iter, items; double lower, upper; };

int main()
{
    const double inf = INFINITY;
    const Case cases[] = {{7, 3, 1, 1, 50, 1, 0, inf}, {7, 4, 1, 1, 50, 1, 0, inf}, {7, 5, 2, 1, 50, 1, 0, inf}, {7, 63, 1, 1, 10, 1, 0, inf},
                          {3, 64, 1, 1, 3, 1, -inf, inf}, {2, 65, 1, 1, 5, 1, 0, inf}, {2, 129, 1, 1, 3, 1, 0, 0.05}, {1, 60, 12, 1, 3, 1, 0, inf},
                          {2, 300, 1, 1, 1, 1, 0, inf}, {2, 513, 1, 1, 2, 1, 0.02, 0.02}, {1, 1024, 1, 1, 2, 1, 0, inf}, {2, 60, 2, 0, 50, 1, -inf, inf},
                          {2, 60, 2, 1, 3, 0, 0, inf}, {2, 130, 2, 0, 50, 0, 0, inf}};
    size_t total = 0, seen = 0;
    for (const Case &c : cases) {
        const int R = c.R, D = c.D, n = c.n;
        std::vector<double> X((size_t)D * n * R), y((size_t)D * R);
        for (int r = 0; r < R; r++) {
            for (int k = 0; k < n; k++) {
                int lvl = rand() % 5;
                for (int d = 0; d < D; d++) {
                    if (rnd() < 0.08) lvl = rand() % 5;
                    X[((size_t)d * n + k) * R + r] = lvl;
                }
            }
            const double slope = r % 4 == 0 ? -0.02 : r % 4 == 1 ? 0.0 : r % 4 == 2 ? 0.03 : 0.1;
            for (int d = 0; d < D; d++) {
                double v = 0.2 + slope * X[((size_t)d * n + r % n) * R + r];
                if (r != 6) v += 0.01 * 2 * (rnd() + rnd() + rnd() - 1.5) + 0.001 * d;
                if (r == 4 && d % 10 == 3) v += d % 20 == 3 ? 0.5 : -0.5;
                y[(size_t)d * R + r] = v;
            }
        }
        for (int d = 0; d < D && R > 2; d++) X[((size_t)d * n + (n - 1)) * R + 2] = 3.0;                        // a constant column
        if (D <= 5 && R > 1) {                                                                                  // the slope lost (lower = 0)
            for (int d = 0; d < D; d++) { X[((size_t)d * n) * R + 1] = d == D - 1; y[(size_t)d * R + 1] = d == D - 1 ? -10.0 : 0.001 * (d % 3 - 1); }
        }
        if (R > 5) X[((size_t)(D - 1) * n + (n - 1)) * R + 5] = INFINITY;                                         // a non-finite item
        const size_t NI = (size_t)n * R;
        std::vector<double> a1(NI, -7), a2 = a1, bi1 = a1, bi2 = a1, s1 = a1, s2 = a1, w1((size_t)D * NI, -7), w2 = w1, b1(R, -7), b2 = b1;
        std::vector<int32_t> it1(NI, -7), it2 = it1, st1 = it1, st2 = it1;
        robfit_run(X.data(), y.data(), R, D, n, c.robust, c.max_iter, c.lower, c.upper, a1.data(), bi1.data(), s1.data(), it1.data(), st1.data(),
                   w1.data(), b1.data());
        RfArgs g{};
        g.R = R; g.D = D; g.n = n; g.robust = c.robust; g.max_iter = c.max_iter; g.lower = c.lower; g.upper = c.upper;
        g.X = X.data(); g.y = y.data(); g.b = b2.data();
        if (c.items) { g.a = a2.data(); g.b_item = bi2.data(); g.sigma = s2.data(); g.iters = it2.data(); g.status = st2.data(); g.weights = w2.data(); }
        if (D <= 64) run<1>(g, c.items); else if (D <= 128) run<2>(g, c.items); else if (D <= 256) run<4>(g, c.items);
        else if (D <= 512) run<8>(g, c.items); else run<16>(g, c.items);
        size_t bad = differ(b1.data(), b2.data(), R);
        if (c.items)
            bad += differ(a1.data(), a2.data(), NI) + differ(bi1.data(), bi2.data(), NI) + differ(s1.data(), s2.data(), NI) +
                   differ(w1.data(), w2.data(), w1.size()) + (memcmp(it1.data(), it2.data(), 4 * NI) != 0) + (memcmp(st1.data(), st2.data(), 4 * NI) != 0);
        int bits = 0, itmax = 0;
        for (size_t i = 0; i < NI; i++) { bits |= st1[i]; if (it1[i] > itmax) itmax = it1[i]; }
        seen |= (size_t)bits;
        printf("R=%d D=%d n=%d robust=%d max_iter=%d items=%d bounds [%g, %g]: differing values %zu  (status bits seen %d, most iterations %d)\n",
               R, D, n, c.robust, c.max_iter, c.items, c.lower, c.upper, bad, bits, itmax);
        total += bad;
    }
    printf("cases %zu, status bits seen %zu, differing values %zu\n", sizeof cases / sizeof cases[0], seen, total);
    return total != 0 || seen != 31;
}
