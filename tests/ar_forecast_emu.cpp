// Stand-alone host program (its own main, CPU only): csrc/ar_forecast.hpp, the kernels' SOURCE, compiled for the host and run
// by 64 lock-stepped threads per workgroup -- __shfl_xor, __ballot and __syncthreads go through a std::barrier -- against
// tests/ar_forecast_ref.c (linked in), bit for bit, NaN matching NaN.  It checks the kernels' arithmetic order and indexing
// without a GPU; it says nothing about the device's sqrt / division / fma or its LDS limits.  Built and run by
// tests/test_ar_forecast_emu.py; by hand (optionally with -fsanitize=address,undefined for the index checks):
//   gcc -O2 -ffp-contract=off -c tests/ar_forecast_ref.c -o ref.o
//   g++ -std=c++20 -O1 -ffp-contract=off -Iepidemicmodeling_amd/csrc tests/ar_forecast_emu.cpp ref.o -o emu -lpthread && ./emu
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
static double lane_f64[64];
static int lane_pred[64];
#define __global__
#define __launch_bounds__(x)
#define __shared__
#define EPI_DEV static inline
static void __syncthreads() { wave->arrive_and_wait(); }
static double __shfl_xor(double v, int h)
{
    lane_f64[threadIdx.x] = v;
    wave->arrive_and_wait();
    const double r = lane_f64[threadIdx.x ^ (unsigned)h];
    wave->arrive_and_wait();
    return r;
}
static unsigned long long __ballot(int p)
{
    lane_pred[threadIdx.x] = p != 0;
    wave->arrive_and_wait();
    unsigned long long m = 0;
    for (int l = 0; l < 64; l++) if (lane_pred[l]) m |= 1ull << l;
    wave->arrive_and_wait();
    return m;
}
double ar_lds[20480];              // the workgroup's dynamic LDS: 160 KiB
using std::fma;
#include "ar_forecast.hpp"

extern "C" void arf_run(const double *seg, const double *beta, const double *s0, const double *i0, const double *z, const double *drive,
                        const int32_t *series, const double *A_in, const double *nv_in, int R, int D, int L, int p, int H, int Sd, int fit,
                        int nv_mode, double dt, double *S, double *A_out, double *nv_out, int32_t *status);

// the launch geometry epi_arfc_run_device uses, for tests/test_ar_forecast_emu.py (this file also builds as a shared object)
extern "C" int emu_ar_blocks_per_region(int D) { return ar_blocks_per_region(D); }

template <class F, class... A> static void launch(F kernel, unsigned blocks, A... args)
{
    for (unsigned b = 0; b < blocks; b++) {
        std::barrier<> bar(64);
        wave = &bar;
        std::vector<std::thread> lanes;
        for (unsigned l = 0; l < 64; l++) lanes.emplace_back([=] { threadIdx.x = l; blockIdx.x = b; kernel(args...); });
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

// drive: 0 none, 1 with a series, 2 one column per chain; sick: 1 = a constant and a non-finite region, 2 = zero-mean segments
struct Case { int R, D, L, p, H, drive, given, sick, nv_mode; };

int main()
{
    const Case cases[] = {{5, 3, 120, 24, 7, 0, 0, 0, 0}, {5, 3, 120, 24, 7, 0, 0, 0, 1}, {1, 1, 2, 1, 1, 0, 0, 0, 0}, {2, 5, 288, 32, 3, 0, 0, 0, 0},
                          {3, 2, 38, 7, 4, 0, 0, 0, 0}, {3, 2, 40, 8, 4, 0, 0, 0, 0}, {3, 2, 38, 5, 4, 0, 0, 0, 0}, {3, 2, 88, 24, 4, 1, 0, 0, 0},
                          {3, 2, 68, 3, 4, 2, 0, 0, 0}, {3, 70, 20, 3, 5, 1, 0, 0, 0}, {70, 1, 20, 3, 5, 0, 0, 0, 0}, {5, 13, 20, 3, 5, 1, 1, 0, 0},
                          {5, 13, 20, 3, 5, 0, 1, 1, 0}, {5, 9, 50, 4, 6, 0, 0, 1, 0}, {2, 65, 60, 6, 30, 0, 0, 2, 0}};
    size_t total = 0;
    for (const Case &c : cases) {
        const int R = c.R, D = c.D, L = c.L, p = c.p, H = c.H, B = R * D, K = L + H, Sd = c.drive == 1 ? R + 2 : B;
        std::vector<double> seg((size_t)L * R), beta(R), s0(R), i0(R), z((size_t)H * B), drv((size_t)H * Sd), Ain((size_t)p * R), nvin(R);
        std::vector<int32_t> ser(B);
        for (int r = 0; r < R; r++) {
            double y1 = 0, y2 = 0;
            for (int t = -100; t < L; t++) {
                const double y = 1.2 * y1 - 0.5 * y2 + (c.sick == 2 ? 1.0 : 0.05) * (rnd() - 0.5);
                y2 = y1; y1 = y;
                if (t >= 0) seg[(size_t)t * R + r] = (c.sick == 2 ? 0.0 : 0.3) + y;
            }
            beta[r] = 0.1 + 0.2 * rnd(); s0[r] = 0.9 + 0.09 * rnd(); i0[r] = 1 - s0[r]; nvin[r] = 1e-3 * (1 + rnd());
            for (int k = 0; k < p; k++) Ain[(size_t)k * R + r] = k == 0 ? -0.9 : 0.01 * rnd();
        }
        if (c.sick == 1) {
            for (int t = 0; t < L; t++) seg[(size_t)t * R + 1] = 0.25;
            seg[(size_t)17 * R + 3] = INFINITY;
            Ain[(size_t)(p - 1) * R + 2] = NAN;
        }
        for (auto &v : z) v = 2 * (rnd() + rnd() + rnd() - 1.5);
        for (auto &v : drv) v = 0.4 * (rnd() - 0.5);
        for (auto &v : ser) v = rand() % Sd;
        std::vector<double> S1((size_t)K * 3 * B, -7), S2 = S1, A1((size_t)p * R, -7), A2 = A1, n1(R, -7), n2 = n1;
        std::vector<int32_t> st1(R, -7), st2 = st1;
        const double *dp = c.drive ? drv.data() : nullptr;
        const int32_t *sp = c.drive == 1 ? ser.data() : nullptr;
        arf_run(seg.data(), beta.data(), s0.data(), i0.data(), z.data(), dp, sp, c.given ? Ain.data() : nullptr, c.given ? nvin.data() : nullptr,
                R, D, L, p, H, Sd, !c.given, c.nv_mode, 0.5, S1.data(), A1.data(), n1.data(), st1.data());
        // what epi_arfc_run_device enqueues
        const double *A = Ain.data(), *nv = nvin.data();
        if (!c.given) {
            ArFitArgs f{};
            f.L = L; f.p = p; f.R = R; f.nv_mode = c.nv_mode; f.seg = seg.data(); f.A = A2.data(); f.nv = n2.data(); f.status = st2.data();
            if (ar_fit_lds_bytes(L, p) > sizeof ar_lds) { puts("LDS budget exceeded"); return 2; }
            launch(ar_fit, (unsigned)R, f);
            A = A2.data(); nv = n2.data();
        } else {
            A2 = Ain; n2 = nvin;
            launch(ar_given_status, (unsigned)((R + 63) / 64), L, R, (const double *)seg.data(), st2.data());
        }
        ArSimArgs g{};
        g.L = L; g.p = p; g.H = H; g.R = R; g.D = D; g.Sd = Sd; g.bpr = ar_blocks_per_region(D); g.dt = 0.5;
        g.seg = seg.data(); g.beta = beta.data(); g.s0 = s0.data(); g.i0 = i0.data(); g.A = A; g.nv = nv; g.z = z.data(); g.drive = dp;
        g.drive_series = sp; g.S = S2.data();
        if (ar_sim_lds_bytes(L, p) > sizeof ar_lds) { puts("LDS budget exceeded"); return 2; }
        launch(ar_simulate, (unsigned)(R * g.bpr), g);
        const size_t bS = differ(S1.data(), S2.data(), S1.size()), bA = differ(A1.data(), A2.data(), A1.size()), bn = differ(n1.data(), n2.data(), R);
        const size_t bs = memcmp(st1.data(), st2.data(), 4 * (size_t)R) != 0;
        size_t clamped = 0, nans = 0;
        for (size_t t = L; t < (size_t)K; t++)
            for (int cc = 0; cc < B; cc++) { clamped += S1[(t * 3 + 2) * B + cc] == 0.0; nans += std::isnan(S1[(t * 3 + 2) * B + cc]); }
        printf("R=%d D=%d L=%d p=%d H=%d drive=%d given=%d sick=%d nv_mode=%d: differing S %zu A %zu nv %zu status %zu  (clamped %.2f, NaN %.2f of the forecast)\n",
               R, D, L, p, H, c.drive, c.given, c.sick, c.nv_mode, bS, bA, bn, bs, (double)clamped / ((double)H * B), (double)nans / ((double)H * B));
        total += bS + bA + bn + bs;
    }
    printf("cases %zu, differing values %zu\n", sizeof cases / sizeof cases[0], total);
    return total != 0;
}
