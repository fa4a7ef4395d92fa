// Host build of the kernels' SOURCE (CPU only): csrc/path_functionals.hpp compiled by the host compiler without its kernels
// (EPI_PATHFN_HOST); the bodies of pathfn_paths and pathfn_combine (pathfn_path_lane, pathfn_combine_lane) are called one lane at a
// time over the grids epi_pathfn_run_device launches -- paths, segments and row groups last first, to show that nothing depends on
// the order lanes run in.  The days are cut into `segments` segments of whole blocks exactly as the library cuts them.  It checks
// the ring's addressing, the order of the sums, the segment records and their folding against tests/pathfn_ref.c without a GPU.
// Built as a shared object and driven by tests/test_pathfn_emu.py, which also writes the stand-in for <hip/hip_runtime.h> it is
// compiled against.
#include <cmath>
#include <cstdint>
#include <cstddef>
#include <vector>
#include <hip/hip_runtime.h>
#define __builtin_nontemporal_load(p) (*(p))
#define EPI_DEV __device__ __forceinline__
#define EPI_PATHFN_HOST 1
namespace epi {
#include "path_functionals.hpp"
}

template <int F32, int NT, int SEG>
static void run_seg(epi::PfArgs &a)
{
    const long long N = (long long)a.R * a.D;
    for (int s = a.nseg - 1; s >= 0; s--)
        for (long long p = N - 1; p >= 0; p--) {
            if (a.derive) {
                for (int q = a.rows - 1; q >= 3; q--) epi::pathfn_path_lane<F32, NT, 1, SEG>(a, (size_t)p, s, q);
                epi::pathfn_path_lane<F32, NT, 4, SEG>(a, (size_t)p, s, 0);
            } else {
                for (int q = a.rows - 1; q >= 0; q--) epi::pathfn_path_lane<F32, NT, 1, SEG>(a, (size_t)p, s, q);
            }
        }
    if (a.nseg > 1)
        for (int q = a.rows_out - 1; q >= 0; q--)
            for (long long p = N - 1; p >= 0; p--) epi::pathfn_combine_lane<NT>(a, (size_t)p, q);
}

template <int F32, int NT>
static void run(epi::PfArgs &a)
{
    if (a.nseg > 1) run_seg<F32, NT, 1>(a); else run_seg<F32, NT, 0>(a);
}

// returns the number of segments the days were cut into
extern "C" int emu_pathfn(int T, int rows, int R, int D, int n_thr, int f32, int derive, int k0, int k1, int segments, const void *src,
                          const double *population, const double *thr, const int32_t *first_day, double *peak_value, double *peak_day,
                          double *min_value, double *min_day, double *total, double *first_cross, double *days_above,
                          double *longest_run, int32_t *n_valid)
{
    epi::PfArgs a{};
    a.T = T; a.rows = rows; a.rows_out = rows + derive; a.R = R; a.D = D; a.n_thr = n_thr; a.derive = derive; a.k0 = k0; a.k1 = k1;
    a.src = src; a.population = population; a.thr = thr; a.first_day = first_day;
    a.peak_value = peak_value; a.peak_day = peak_day; a.min_value = min_value; a.min_day = min_day; a.total = total;
    a.first_cross = first_cross; a.days_above = days_above; a.longest_run = longest_run; a.n_valid = n_valid;
    const int nb = (k1 - k0 + epi::kPfBlock - 1) / epi::kPfBlock;
    const int want = segments < nb ? segments : nb, per = (nb + want - 1) / want;
    a.nseg = (nb + per - 1) / per; a.seg_days = per * epi::kPfBlock; a.nblk = nb;
    const size_t M = (size_t)a.rows_out * R * D;
    std::vector<double> mx((size_t)a.nseg * M, -7.0), mn((size_t)a.nseg * M, -7.0), bsum((size_t)nb * M, -7.0);
    std::vector<int32_t> pint((size_t)a.nseg * 3 * M, -7), pthr((size_t)a.nseg * 5 * (n_thr ? n_thr : 1) * M, -7);
    a.p_mx = mx.data(); a.p_mn = mn.data(); a.p_bsum = bsum.data(); a.p_int = pint.data(); a.p_thr = pthr.data();
    const int bucket = n_thr == 0 ? 0 : (n_thr <= 2 ? 2 : 8);
    if (f32) { if (bucket == 0) run<1, 0>(a); else if (bucket == 2) run<1, 2>(a); else run<1, 8>(a); }
    else { if (bucket == 0) run<0, 0>(a); else if (bucket == 2) run<0, 2>(a); else run<0, 8>(a); }
    return a.nseg;
}
