// Host build of the kernels' SOURCE (CPU only): csrc/loglik.hpp with csrc/ekf_device.hpp compiled by the host compiler; the body
// of every kernel (ll_replay_lane, ll_block_lane, ll_chain_lane, ll_select_lane) is called one lane at a time, in the order the
// launches of epi_loglik_run_device give: the replay of every chain, every (chain, block) -- blocks in DESCENDING order here, to
// show that nothing depends on the order lanes run in --, every chain, every region.  It checks the arithmetic order, the
// addressing of both layouts and both storages and that padding lanes are neither read nor written against tests/loglik_ref.py
// without a GPU; it says nothing about the device's division.  Built as a shared object and driven by tests/test_loglik_emu.py,
// which also writes the three-line stand-in for <hip/hip_runtime.h> this file is compiled against.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <cstddef>
#include <vector>
#define __builtin_amdgcn_ballot_w64(p) ((p) ? 1ull : 0ull)
#define __builtin_amdgcn_readfirstlane(x) (x)
#define __builtin_nontemporal_load(p) (*(p))
#define __builtin_nontemporal_store(v, p) (*(p) = (v))
using std::fma; using std::fmax; using std::fabs; using std::sqrt; using std::ldexp; using std::ilogb;
#include "ekf_device.hpp"
#define EPI_LOGLIK_HOST 1
namespace epi {
#include "loglik.hpp"
}

extern "C" void emu_loglik(int m, int flip, int generic, int obs_type, int B, int T, int L, int Sx, int r_mode, int f32, int k0, int k1,
                           int G, int lane_block, const void *S_MINUS, const void *P_MINUS, const void *innov, const double *x,
                           const double *R_series, const double *R_scalar, const int32_t *x_series, const double *prm,
                           double *loglik, double *nis_mean, int32_t *n_valid, int32_t *status, double *S, double *nis, double *R_used,
                           int32_t *best, double *best_loglik)
{
    epi::LlArgs a{};
    a.B = B; a.T = T; a.L = L; a.Sx = Sx; a.r_mode = r_mode; a.f32 = f32; a.flip = flip; a.generic = generic; a.obs_type = obs_type;
    a.k0 = k0; a.k1 = k1; a.G = G; a.m = m; a.nb32 = (T + epi::kLlBlock - 1) / epi::kLlBlock;
    epi::ll_geometry(B, lane_block, &a.blk, &a.nblk);
    a.S_MINUS = S_MINUS; a.P_MINUS = P_MINUS; a.innov = innov; a.x = x; a.R_series = R_series; a.R_scalar = R_scalar;
    a.x_series = x_series; a.prm = prm;
    const size_t nB = (size_t)a.nb32 * B;
    std::vector<double> pt(nB, -7.0), pq(nB, -7.0), rk((size_t)T * B, -7.0), wl(B, -7.0), win((size_t)2 * L, -7.0);
    std::vector<int32_t> pn(nB, -7), pb(nB, -7), wn(B, -7), ws(B, -7);
    a.part_term = pt.data(); a.part_q = pq.data(); a.part_n = pn.data(); a.part_bad = pb.data();
    a.Rk = R_used ? R_used : (r_mode == 0 ? rk.data() : nullptr);
    a.loglik = loglik ? loglik : wl.data(); a.nis_mean = nis_mean;
    a.n_valid = n_valid ? n_valid : wn.data(); a.status = status ? status : ws.data();
    a.S = S; a.nis = nis; a.best = best; a.best_loglik = best_loglik;
    if (r_mode == 0)
        for (int c = 0; c < B; c++) epi::ll_replay_lane(a, c, win.data(), 1);
    for (int b = a.nb32 - 1; b >= 0; b--)
        for (int c = 0; c < B; c++) epi::ll_block_lane(a, c, b);
    for (int c = 0; c < B; c++) epi::ll_chain_lane(a, c);
    if (best || best_loglik)
        for (int r = 0; r < B / G; r++) epi::ll_select_lane(a, r);
}
