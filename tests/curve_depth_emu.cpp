// Host build of the kernels' SOURCE (CPU only): csrc/curve_depth.hpp compiled by the host compiler without its kernels
// (EPI_CDEPTH_HOST); the bodies of the lane-shaped kernels cdepth_combine, cdepth_rank, cdepth_fence and cdepth_outliers
// (cdepth_*_lane) are called one lane at a time over the grids epi_cdepth_run_device launches, last lane first, to show that
// nothing depends on the order lanes run in.  The wavefront-shaped depth pass cannot run here: its 32-day block records are
// written by a sequential loop below in the record format the pass writes (band, pairs, le | days << 24, members), so that the
// combining of the records, the packing and every later lane-shaped pass are checked against tests/curve_depth_ref.c without a
// GPU.  The fence envelope comes from the caller (the restatement's envelope of the fence_frac deepest paths).
// Built as a shared object and driven by tests/test_curve_depth_emu.py, which also writes the stand-in for <hip/hip_runtime.h>.
#include <cmath>
#include <cstdint>
#include <cstddef>
#include <vector>
#include <hip/hip_runtime.h>
#define EPI_DEV __device__ __forceinline__
#define EPI_CDEPTH_HOST 1
namespace epi {
using std::ceil;
#include "curve_depth.hpp"
}

template <int F32>
static void records(const epi::CdArgs &a)
{
    const size_t N = (size_t)a.R * a.D, M = (size_t)a.rows_out * N;
    for (size_t i = 0; i < (size_t)a.nblk * 4 * M; i++) a.rec[i] = 0;
    for (int q = 0; q < a.rows_out; q++)
        for (int r = 0; r < a.R; r++)
            for (int t = epi::cd_first_day(a, r); t < a.k1; t++) {
                const size_t p0 = (size_t)r * a.D;
                uint32_t n = 0;
                for (int e = 0; e < a.D; e++) { const double y = epi::cd_member<F32>(a, t, q, p0 + e); n += y == y; }
                uint32_t *rc = a.rec + (size_t)((t - a.k0) / epi::kCdBlock) * 4 * M + (size_t)q * N + p0;
                for (int d = 0; d < a.D; d++) {
                    const double x = epi::cd_member<F32>(a, t, q, p0 + d);
                    if (x != x) continue;
                    uint32_t below = 0, above = 0;
                    for (int e = 0; e < a.D; e++) {
                        const double y = epi::cd_member<F32>(a, t, q, p0 + e);
                        below += y < x;
                        above += y > x;
                    }
                    rc[d] += n * (n - 1) / 2 - below * (below - 1) / 2 - above * (above - 1) / 2;
                    rc[M + d] += n * (n - 1) / 2;
                    rc[2 * M + d] += (n - above) + (1u << 24);
                    rc[3 * M + d] += n;
                }
            }
}

template <int F32>
static void run(epi::CdArgs &a, bool fence)
{
    const long long N = (long long)a.R * a.D;
    records<F32>(a);
    for (int q = a.rows_out - 1; q >= 0; q--)
        for (long long p = N - 1; p >= 0; p--) epi::cdepth_combine_lane(a, (size_t)p, q);
    for (int q = a.rows_out - 1; q >= 0; q--)
        for (long long p = N - 1; p >= 0; p--) epi::cdepth_rank_lane(a, (size_t)p, q);
    if (!fence) return;
    for (int q = a.rows_out - 1; q >= 0; q--)
        for (long long p = N - 1; p >= 0; p--) epi::cdepth_fence_lane<F32>(a, (size_t)p, q);
    for (long long c = (long long)a.rows_out * a.R - 1; c >= 0; c--) epi::cdepth_outliers_lane(a, (size_t)c);
}

// returns the number of 32-day blocks
extern "C" int emu_cdepth(int T, int rows, int R, int D, int f32, int derive, int k0, int k1, const void *src, const double *population,
                          const int32_t *first_day, double fence_factor, double *fence_lo, double *fence_hi, double *depth, double *mhi,
                          double *band_count, double *pair_total, int32_t *n_valid, int32_t *depth_rank, int32_t *n_ranked,
                          int32_t *median_path, int32_t *out_days, int32_t *n_outliers)
{
    epi::CdArgs a{};
    a.T = T; a.rows = rows; a.rows_out = rows + derive; a.R = R; a.D = D; a.derive = derive; a.k0 = k0; a.k1 = k1;
    a.nblk = (k1 - k0 + epi::kCdBlock - 1) / epi::kCdBlock; a.nseg = a.nblk; a.seg_days = epi::kCdBlock;
    a.src = src; a.population = population; a.first_day = first_day; a.fence_factor = fence_factor;
    a.fence_lo = fence_lo; a.fence_hi = fence_hi;
    a.depth = depth; a.mhi = mhi; a.band_count = band_count; a.pair_total = pair_total; a.n_valid = n_valid;
    a.depth_rank = depth_rank; a.n_ranked = n_ranked; a.median_path = median_path; a.out_days = out_days; a.n_outliers = n_outliers;
    std::vector<uint32_t> rec((size_t)a.nblk * 4 * a.rows_out * R * D, 0xdeadbeefu);
    a.rec = rec.data();
    if (f32) run<1>(a, fence_factor > 0.0); else run<0>(a, fence_factor > 0.0);
    return a.nblk;
}
