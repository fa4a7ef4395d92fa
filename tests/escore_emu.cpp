// Host build of the kernels' SOURCE (CPU only): csrc/ens_score.hpp compiled by the host compiler without its wavefront kernel
// (EPI_ESCORE_HOST); the body of escore_regions (escore_region_lane) is called one lane at a time over the grid
// epi_escore_run_device launches, last lane first, to show that nothing depends on the order lanes run in.  The per-item arrays
// it reads are the caller's.  It checks the order of the sums, the window, first_day, the histogram's integer arithmetic and
// the addressing against tests/escore_ref.py without a GPU; it says nothing about the device's division.  Built as a shared
// object and driven by tests/test_escore_emu.py, which also writes the stand-in for <hip/hip_runtime.h> it is compiled against.
#include <cmath>
#include <cstdint>
#include <cstddef>
#include <hip/hip_runtime.h>
#define EPI_DEV __device__ __forceinline__
#define EPI_ESCORE_HOST 1
namespace epi {
#include "ens_score.hpp"
}

extern "C" void emu_escore_regions(int T, int rows_out, int R, int n_a, int n_bins, int k0, int k1, const int32_t *first_day,
                                   const double *crps, const double *wis, const double *ae, const int32_t *rank, const int32_t *ties,
                                   const int32_t *cover, const int32_t *count, double *crps_mean, double *wis_mean, double *ae_mean,
                                   int32_t *n_scored, double *cover_frac, int32_t *pit_hist)
{
    epi::EsArgs a{};
    a.T = T; a.rows_out = rows_out; a.R = R; a.n_a = n_a; a.n_bins = n_bins; a.k0 = k0; a.k1 = k1; a.first_day = first_day;
    a.crps = const_cast<double *>(crps); a.wis = const_cast<double *>(wis); a.ae = const_cast<double *>(ae);
    a.rank = const_cast<int32_t *>(rank); a.ties = const_cast<int32_t *>(ties); a.cover = const_cast<int32_t *>(cover);
    a.count = const_cast<int32_t *>(count);
    a.crps_mean = crps_mean; a.wis_mean = wis_mean; a.ae_mean = ae_mean; a.n_scored = n_scored; a.cover_frac = cover_frac;
    a.pit_hist = pit_hist;
    for (long long i = (long long)rows_out * R - 1; i >= 0; i--) epi::escore_region_lane(a, (int)(i / R), (int)(i % R));
}
