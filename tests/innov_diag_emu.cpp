// Host build of the kernels' SOURCE (CPU only): csrc/innov_diag.hpp with csrc/ekf_device.hpp and csrc/loglik.hpp compiled by the
// host compiler; the body of every kernel (id_block1_lane, id_chain1_lane, id_block2_lane, id_chain2_lane) is called one lane at
// a time, in the order the launches of epi_idiag_run_device give -- the blocks in DESCENDING order here, to show that nothing
// depends on the order lanes run in.  The LDS column of a lane is a plain array of stride 1, poisoned before every lane.  It checks
// the arithmetic order, the addressing of both layouts and storages and that padding lanes are neither read nor written against
// tests/innov_diag_ref.py without a GPU; it says nothing about the device's division or square root.  Built as a shared object
// and driven by tests/test_innov_diag_emu.py, which also writes the stand-in for <hip/hip_runtime.h> this file is compiled against.
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
#define EPI_IDIAG_HOST 1
namespace epi {
#include "loglik.hpp"
#include "innov_diag.hpp"
}

// outs: the 11 double outputs, then the 7 int32 ones, then acf, in the ABI's order; NULL = not requested
extern "C" void emu_idiag(int B, int T, int H, int f32, int flip, int k0, int k1, int lane_block, const void *e, const double *S,
                          void *const *outs)
{
    epi::IdArgs a{};
    a.B = B; a.T = T; a.H = H; a.f32 = f32; a.flip = flip; a.k0 = k0; a.k1 = k1; a.nb32 = (T + epi::kIdBlock - 1) / epi::kIdBlock;
    a.h3 = (int)((2 * (int64_t)(k1 - k0) + 3) / 6);
    int blk, nblk;
    epi::ll_geometry(B, lane_block, &blk, &nblk);
    a.bp = (size_t)blk * (size_t)nblk;
    a.e = e; a.S = S;
    double **d = (double **)outs;
    a.mean = d[0]; a.var = d[1]; a.skew = d[2]; a.kurt = d[3]; a.jb = d[4]; a.nis_sum = d[5]; a.nis_mean = d[6]; a.lb_q = d[7];
    a.het = d[8]; a.cusumsq_max = d[9]; a.max_abs = d[10];
    int32_t **i = (int32_t **)(outs + 11);
    a.n = i[0]; a.lb_lags = i[1]; a.het_n1 = i[2]; a.het_n2 = i[3]; a.cusumsq_step = i[4]; a.max_abs_step = i[5]; a.status = i[6];
    a.acf = (double *)outs[18];
    a.lags = (a.acf || a.lb_q) ? H : 0;
    const size_t nB = (size_t)a.nb32 * B;
    std::vector<std::vector<double>> wd(10, std::vector<double>(nB, -7.0)), cd(2, std::vector<double>(B, -7.0));
    std::vector<std::vector<int32_t>> wi(7, std::vector<int32_t>(nB, -7)), ci(2, std::vector<int32_t>(B, -7));
    std::vector<double> rc(nB * (size_t)(H ? H : 1), -7.0), col((size_t)epi::kIdBlock + H);
    a.p_sum = wd[0].data(); a.p_q = wd[1].data(); a.pre_q = wd[2].data(); a.r_m2 = wd[3].data(); a.r_m3 = wd[4].data();
    a.r_m4 = wd[5].data(); a.r_f = wd[6].data(); a.r_l = wd[7].data(); a.r_max = wd[8].data(); a.r_cs = wd[9].data();
    a.p_n = wi[0].data(); a.p_bad = wi[1].data(); a.pre_n = wi[2].data(); a.r_nf = wi[3].data(); a.r_nl = wi[4].data();
    a.r_maxk = wi[5].data(); a.r_csk = wi[6].data();
    a.c_mean = cd[0].data(); a.c_q = cd[1].data(); a.c_n = ci[0].data(); a.c_bad = ci[1].data();
    a.r_c = rc.data();
    for (int b = a.nb32 - 1; b >= 0; b--)
        for (int c = 0; c < B; c++) epi::id_block1_lane(a, c, b);
    for (int c = 0; c < B; c++) epi::id_chain1_lane(a, c);
    for (int b = a.nb32 - 1; b >= 0; b--)
        for (int c = 0; c < B; c++) {
            for (double &v : col) v = 1e300;
            epi::id_block2_lane(a, c, b, col.data(), 1);
        }
    for (int c = 0; c < B; c++) epi::id_chain2_lane(a, c);
}
