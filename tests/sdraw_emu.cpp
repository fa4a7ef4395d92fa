// Host build of the kernels' SOURCE (CPU only): csrc/smoother_draws.hpp with csrc/ekf_device.hpp compiled by the host compiler; the
// body of each kernel (sdraw_gain_lane, sdraw_path_lane) is called one lane at a time over the grids epi_sdraw_run_device launches
// -- a wavefront ballot is the lane's own predicate, which is what the wave-uniform loops of sym_pinv_psd reduce to for a single
// lane.  The gain grid is walked in launches of `groups` workgroups with three workgroups per day past the end of the batch (their
// lanes work on the last chain and store nothing), the path grid in launches of `groups` workgroups of 256 lanes, last launch
// first.  It checks the arithmetic order, the addressing of both layouts and storages and the z / X element types against
// tests/sdraw_ref.py without a GPU; it says nothing about the device's sqrt / division.  Built as a shared object and driven by
// tests/test_sdraw_emu.py, which also writes the three-line stand-in for <hip/hip_runtime.h> this file is compiled against.
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

extern "C" void emu_sdraw(int B, int T, int D, int k0, int clamp, int lane_block, int f32, int z_mode, int out_f32, int groups,
                          const void *S_PLUS, const void *P_PLUS, const void *S_MINUS, const void *P_MINUS, const double *prm,
                          const void *z, const double *s_term, const double *P_term, void *X, int32_t *rank, int32_t *status,
                          double *J, double *L)
{
    epi::SdArgs a{};
    a.B = B; a.T = T; a.D = D; a.k0 = k0; a.clamp = clamp; a.f32 = f32;
    epi::sdraw_geometry(B, lane_block, &a.blk, &a.nblk);
    a.S_PLUS = S_PLUS; a.P_PLUS = P_PLUS; a.S_MINUS = S_MINUS; a.P_MINUS = P_MINUS; a.prm = prm; a.z = z; a.s_term = s_term;
    a.P_term = P_term; a.X = X; a.rank = rank; a.status = status; a.J = J; a.L = L;
    std::vector<double> ws((size_t)T * B * epi::kSdRec, -7.0);
    a.ws = ws.data();
    if (status) memset(status, 0, sizeof(int32_t) * (size_t)B);
    double lds[12];
    a.tiles = (unsigned)B + 3u;                               // workgroups of ONE lane
    const long long gg = (long long)a.tiles * T;
    for (long long w0 = 0; w0 < gg; w0 += groups)
        for (long long w = w0; w < gg && w < w0 + groups; w++)
            epi::sdraw_gain_lane<1>(a, (size_t)(w / a.tiles), (size_t)(w % a.tiles), lds);
    if (!X) return;
    const long long N = (long long)B * D, pg = (N + epi::kSdPathWg - 1) / epi::kSdPathWg;
    const long long nl = (pg + groups - 1) / groups;
    for (long long l = nl - 1; l >= 0; l--)
        for (long long w = l * groups; w < pg && w < (l + 1) * groups; w++)
            for (int th = 0; th < epi::kSdPathWg; th++) {
                const size_t p = (size_t)w * epi::kSdPathWg + th;
                if (p >= (size_t)N) continue;
                if (z_mode == 0) { if (out_f32) epi::sdraw_path_lane<0, 1>(a, p); else epi::sdraw_path_lane<0, 0>(a, p); }
                else if (z_mode == 1) { if (out_f32) epi::sdraw_path_lane<1, 1>(a, p); else epi::sdraw_path_lane<1, 0>(a, p); }
                else { if (out_f32) epi::sdraw_path_lane<2, 1>(a, p); else epi::sdraw_path_lane<2, 0>(a, p); }
            }
}
