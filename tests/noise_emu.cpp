// Host build of the kernels' SOURCE (CPU only): csrc/noise.hpp and csrc/smoother_draws.hpp over csrc/ekf_device.hpp, compiled by the
// host compiler against the stand-in for <hip/hip_runtime.h> that tests/test_noise_emu.py writes.  emu_noise_fill walks the items of
// noise_fill one lane at a time, in launches of `groups` workgroups, last launch first; emu_sdraw_paths runs sdraw_gain_lane and then
// sdraw_path_lane with the noise mode asked for (1: z read, 3: z generated from the key), so that the seeded path is held to the
// path given the filled array without a GPU.  It says nothing about the device's sqrt / division.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <cstddef>
#include <vector>
#define __builtin_amdgcn_ballot_w64(p) ((p) ? 1ull : 0ull)
#define __builtin_amdgcn_readfirstlane(x) (x)
#define __builtin_nontemporal_load(p) (*(p))
#define __builtin_nontemporal_store(v, p) (*(p) = (v))
static int atomicOr(int32_t *p, int v) { const int o = *p; *p |= v; return o; }
using std::fma; using std::fmax; using std::fmin; using std::fabs; using std::sqrt; using std::ldexp; using std::ilogb;
#include "ekf_device.hpp"
#define EPI_SDRAW_HOST 1
namespace epi {
#include "smoother_draws.hpp"
}

extern "C" void emu_noise_fill(uint32_t seed_lo, uint32_t seed_hi, uint32_t stream, uint32_t t0, int nt, int rows, uint64_t lane0,
                               uint64_t n_lanes, int f32, int groups, void *out)
{
    epi::NoiseFillArgs a{};
    a.nk.seed_lo = seed_lo; a.nk.seed_hi = seed_hi; a.nk.stream = stream;
    a.rows = rows; a.f32 = f32; a.t0 = t0; a.lane0 = lane0; a.n_lanes = n_lanes;
    a.items = (uint64_t)nt * (uint64_t)((rows + 1) / 2) * n_lanes;
    a.out = out;
    const long long wgs = (long long)((a.items + epi::kNoiseWg - 1) / epi::kNoiseWg), nl = (wgs + groups - 1) / groups;
    for (long long l = nl - 1; l >= 0; l--)
        for (long long w = l * groups; w < wgs && w < (l + 1) * groups; w++)
            for (int th = 0; th < epi::kNoiseWg; th++) {
                const uint64_t item = (uint64_t)w * epi::kNoiseWg + th;
                if (item < a.items) epi::noise_fill_lane(a, item);
            }
}

extern "C" double emu_normal_draw(uint32_t seed_lo, uint32_t seed_hi, uint32_t stream, uint32_t t, uint32_t row, uint64_t lane)
{
    const epi::NoiseKey nk{seed_lo, seed_hi, stream};
    return epi::epi_normal_draw(nk, t, row, lane);
}

extern "C" void emu_sdraw_paths(int B, int T, int D, int k0, int clamp, int z_mode, uint32_t seed_lo, uint32_t seed_hi, uint32_t stream,
                                const double *S_PLUS, const double *P_PLUS, const double *S_MINUS, const double *P_MINUS, const double *prm,
                                const double *z, double *X)
{
    epi::SdArgs a{};
    a.B = B; a.T = T; a.D = D; a.k0 = k0; a.clamp = clamp; a.f32 = 0;
    epi::sdraw_geometry(B, 0, &a.blk, &a.nblk);
    a.S_PLUS = S_PLUS; a.P_PLUS = P_PLUS; a.S_MINUS = S_MINUS; a.P_MINUS = P_MINUS; a.prm = prm; a.z = z; a.X = X;
    const epi::NoiseKey nk{seed_lo, seed_hi, stream};
    std::vector<double> ws((size_t)T * B * epi::kSdRec, -7.0);
    a.ws = ws.data();
    double lds[12];
    a.tiles = (unsigned)B;
    for (long long w = 0; w < (long long)a.tiles * T; w++) epi::sdraw_gain_lane<1>(a, (size_t)(w / a.tiles), (size_t)(w % a.tiles), lds);
    for (size_t p = 0; p < (size_t)B * D; p++) {
        if (z_mode == 3) epi::sdraw_path_lane<3, 0>(a, p, nk);
        else epi::sdraw_path_lane<1, 0>(a, p);
    }
}
