// Host build of the kernel's SOURCE (CPU only): csrc/npi_plan.hpp with csrc/ekf_device.hpp compiled by the host compiler; the
// body of the kernel (plan_lane) is called one lane at a time, chains in DESCENDING order, to show that nothing depends on the
// order lanes run in.  The workspaces are laid out as epi_plan_run_device lays them out and start as a poison value.  It checks
// the arithmetic order and the addressing against tests/npi_plan_ref.c without a GPU; it says nothing about the device's
// division.  Built as a shared object and driven by tests/test_npi_plan_emu.py, which also writes the three-line stand-in for
// <hip/hip_runtime.h> this file is compiled against.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <cstddef>
#include <vector>
#define __builtin_amdgcn_ballot_w64(p) ((p) ? 1ull : 0ull)
#define __builtin_amdgcn_readfirstlane(x) (x)
#define __builtin_nontemporal_load(p) (*(p))
#define __builtin_nontemporal_store(v, p) (*(p) = (v))
using std::fma; using std::fmax; using std::fmin; using std::fabs; using std::sqrt; using std::ldexp; using std::ilogb;
#include "ekf_device.hpp"
#define EPI_PLAN_HOST 1
namespace epi {
#include "npi_plan.hpp"
}

extern "C" void emu_plan(int R, int P, int H, int n, int prefix_days, int max_iter, int max_halvings, double tol, const double *sp,
                         const double *u_min, const double *eps, const double *u_fixed, const double *u_init, const double *J0_prefix,
                         const double *J1_prefix, double *plan, double *J0, double *J1, double *F, double *gap, int32_t *iters,
                         int32_t *halvings, int32_t *status, double *states, double *mu, double *F_trace)
{
    const size_t B = (size_t)R * P;
    std::vector<double> u1((size_t)H * n * B, -7.0), x0((size_t)H * 3 * B, -7.0), x1((size_t)H * 3 * B, -7.0);
    std::vector<uint32_t> mask((size_t)H * B, 0xDEADBEEFu);
    epi::PlanArgs a{};
    a.R = R; a.P = P; a.H = H; a.n = n; a.max_iter = max_iter; a.max_halvings = max_halvings; a.prefix_days = prefix_days; a.tol = tol;
    a.sp = sp; a.u_min = u_min; a.eps = eps; a.u_fixed = u_fixed; a.u_init = u_init; a.J0_prefix = J0_prefix; a.J1_prefix = J1_prefix;
    a.ub[0] = plan; a.ub[1] = u1.data();
    a.xb[0] = states ? states : x0.data(); a.xb[1] = x1.data();
    a.want_states = states != nullptr;
    a.mask = mask.data();
    a.J0 = J0; a.J1 = J1; a.F = F; a.gap = gap; a.iters = iters; a.halvings = halvings; a.status = status;
    a.mu = mu; a.F_trace = F_trace;
    for (long long c = (long long)B - 1; c >= 0; c--) epi::plan_lane(a, (int)c);
}
