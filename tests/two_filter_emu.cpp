// Host build of the kernel's SOURCE (CPU only): csrc/two_filter.hpp with csrc/ekf_device.hpp compiled by the host compiler and
// run one lane at a time -- a wavefront ballot is the lane's own predicate, readfirstlane the lane's own value, which is what the
// wave-uniform loops of sym_pinv_psd / sym_pinv_two_sided / mrdivide reduce to for a single lane (a pair or a step is skipped
// only if NO lane needs it; lanes that do not take part apply the identity).  It checks the kernel's arithmetic order, its
// addressing of both layouts and both storages and the clamped tail workgroups against tests/two_filter_ref.py without a GPU;
// it says nothing about lanes of different ranks sharing a wavefront (that is tests/test_gpu_two_filter.py) nor about the
// device's sqrt / division.  Built as a shared object and driven by tests/test_two_filter_emu.py, which also writes the
// three-line stand-in for <hip/hip_runtime.h> this file is compiled against.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <cstddef>
struct Dim { unsigned x; };
static Dim threadIdx, blockIdx;
#define __global__
#define __launch_bounds__(...)
#define __shared__ static
#define __builtin_amdgcn_ballot_w64(p) ((p) ? 1ull : 0ull)
#define __builtin_amdgcn_readfirstlane(x) (x)
#define __builtin_nontemporal_load(p) (*(p))
#define __builtin_nontemporal_store(v, p) (*(p) = (v))
static int atomicOr(int32_t *p, int v) { const int o = *p; *p |= v; return o; }
using std::fma; using std::fmax; using std::fabs; using std::sqrt; using std::ldexp; using std::ilogb;
#include "ekf_device.hpp"
namespace epi {
template <int M> constexpr int pinv_wg() { return 1; }
#include "two_filter.hpp"
}
// the launch geometry epi_fuse_run_device / _host use, for tests/test_two_filter_emu.py
extern "C" void emu_fuse_geometry(int B, int lane_block, int *blk, int *nblk) { epi::fuse_geometry(B, lane_block, blk, nblk); }

extern "C" void emu_fuse(int m, int B, int T, int blk, int nblk, int f32, int form, int p_solver, const void *sf, const void *Pf,
                         const void *sb, const void *Pb, void *s_out, void *P_out, double *d2, int32_t *rank, int32_t *status)
{
    epi::FuseArgs a{};
    a.B = B; a.T = T; a.blk = blk; a.nblk = nblk; a.f32 = f32; a.form = form; a.p_solver = p_solver; a.tiles = (unsigned)B + 3u; a.wg0 = 0;
    a.sf = sf; a.Pf = Pf; a.sb = sb; a.Pb = Pb; a.s_out = s_out; a.P_out = P_out; a.d2 = d2; a.rank = rank; a.status = status;
    if (status) memset(status, 0, sizeof(int32_t) * (size_t)B);
    threadIdx.x = 0;
    for (unsigned w = 0; w < a.tiles * (unsigned)T; w++) {      // three workgroups per day lie past the end of the batch
        blockIdx.x = w;
        if (m == 6) epi::two_filter<6>(a); else epi::two_filter<3>(a);
    }
}
