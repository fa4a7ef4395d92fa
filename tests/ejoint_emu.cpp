// Host build of the joint score's SOURCE (CPU only), as a stand-alone program: csrc/ens_joint.hpp compiled by the host compiler
// without its wavefront kernels (EPI_EJOINT_HOST).  What runs here is the header's own code: the workspace layout
// (ejoint_ws_size, ejoint_carve), the launch loop (ejoint_for_units), the block -> unit map of the pair kernel (ejoint_swizzle),
// the tile numbering (ejoint_tile_of) and the final pass (ejoint_final_lane), one lane at a time, last lane first.  The
// wavefront kernels' work per unit -- an item's pre-pass, a tile's sum, a day's v_s -- is written out sequentially below and put
// where the kernels put it, through the same indices.  Every output is compared, bit for bit (every NaN one value), with
// tests/ejoint_ref.c, which is linked in.  The workspace is exactly ejoint_ws_size bytes from malloc, so a slot outside it is an
// address-sanitizer report; every tile slot of a defined item must be written exactly once in every launch cut.  Built with
// -fsanitize=address,undefined and run by tests/test_ejoint_emu.py, which also writes the stand-in for <hip/hip_runtime.h>.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>
#define EPI_DEV __device__ __forceinline__
#define EPI_EJOINT_HOST 1
namespace epi {
#include "ens_joint.hpp"
}

extern "C" void ejoint_ref(int T, int rows, int R, int D, int Rt, int f32, int derive, int k0, int k1, int vs_order, int max_lag,
                           const void *src, const double *population, const double *truth, const int32_t *truth_series,
                           const int32_t *first_day, double *es, double *truth_term, double *spread_term, double *vs, int32_t *n_members,
                           int32_t *n_days, double *member_dist);

struct Case {
    int T, rows, R, D, Rt, f32, k0, k1;
    std::vector<double> s64, truth, pop;
    std::vector<float> s32;
    std::vector<int32_t> ts, fd;
    const void *src() const { return f32 ? (const void *)s32.data() : (const void *)s64.data(); }
    double load(size_t o) const { return f32 ? (double)s32[o] : s64[o]; }
    double form(int row, int t, int r, int e) const
    {
        const size_t B = (size_t)R * D, c = (size_t)r * D + e;
        if (row < rows) return load(((size_t)t * rows + row) * B + c);
        const size_t o = (size_t)t * rows * B + c;
        return ((pop[r] * load(o)) * load(o + B)) * load(o + 2 * B);
    }
    double y(int row, int t, int r) const { return truth[((size_t)t * (rows + 1) + row) * Rt + ts[r]]; }
};

static uint64_t rng_state = 88172645463325252ull;
static double uniform()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}

// the case of tests/ejoint_ref.py: 3 regions, 3 rows and the derived one, a window of W + 1 days with a day without truth in
// column 0, a member absent on one day only, a region without members, a first_day at k1 (variant 0) or past it (variant 1)
static Case make_case(int D, int W, int f32, int variant)
{
    Case c;
    c.T = W + 3; c.rows = 3; c.R = 3; c.D = D; c.Rt = 2; c.f32 = f32; c.k0 = 1; c.k1 = c.T - 1;
    const size_t B = (size_t)3 * D;
    c.s64.resize((size_t)c.T * 3 * B);
    for (double &v : c.s64) v = 0.5 + uniform();
    c.truth.resize((size_t)c.T * 4 * 2);
    for (size_t i = 0; i < c.truth.size(); i++) c.truth[i] = (0.5 + uniform()) * ((i / 2) % 4 == 3 ? 3.0e3 : 1.0);
    const int t_gap = c.k0 + (W + 1) / 2, t_abs = t_gap != c.k1 - 1 ? c.k1 - 1 : c.k0;
    for (int row = 0; row < 4; row++) c.truth[((size_t)t_gap * 4 + row) * 2 + 0] = NAN;
    c.s64[((size_t)t_gap * 3 + 0) * B + 0] = NAN;
    c.s64[((size_t)t_abs * 3 + 1) * B + (D > 1 ? 0 : 2 * D) + D / 2] = NAN;
    for (int row = 0; row < 3; row++)
        for (int e = 0; e < D; e++) c.s64[((size_t)(c.k0 + W / 2) * 3 + row) * B + D + e] = NAN;
    if (f32) {
        c.s32.assign(c.s64.begin(), c.s64.end());
        c.s64.clear();
    }
    c.pop = {3.0e3, 5.0e3, 4.0e3};
    c.ts = {0, 1, 0};
    if (variant == 0) c.fd = {0, 0, c.k1};
    else c.fd = {c.k0 + 1, c.k1 + 2, 0};
    return c;
}

static double tree(std::vector<double> a)
{
    for (size_t h = a.size() / 2; h >= 1; h /= 2)
        for (size_t i = 0; i < h; i++) a[i] = a[i] + a[i + h];
    return a[0];
}

static double gfun(double a, int vs_order) { return vs_order == 1 ? std::sqrt(std::fabs(a)) : std::fabs(a); }

// ---- what one workgroup of each wavefront kernel leaves behind, through the kernel's indices ----
static void unit_members(const Case &c, const epi::EjArgs &a, long long item)
{
    const int row = (int)(item / a.R), r = (int)(item % a.R), D = a.D;
    const int fd = a.first_day ? a.first_day[r] : 0;
    int P = 64;
    while (P < D) P *= 2;
    std::vector<double> d2(P, 0.0);
    std::vector<int> ok(P, 0);
    for (int e = 0; e < D; e++) ok[e] = 1;
    int W = 0;
    for (int t = a.k0 > fd ? a.k0 : fd; t < a.k1; t++) {
        const double y = c.y(row, t, r);
        if (y != y) continue;
        a.days[(size_t)item * a.wcap + W++] = t;
        for (int e = 0; e < D; e++) {
            const double x = c.form(row, t, r, e), d = x - y;
            if (x != x) ok[e] = 0;
            d2[e] = d2[e] + d * d;
        }
    }
    int n = 0;
    for (int j = 0; j < a.nb; j++) {
        unsigned long long m = 0;
        for (int l = 0; l < 64; l++)
            if (j * 64 + l < P && ok[j * 64 + l]) m |= 1ull << l, n++;
        a.mask[(size_t)item * a.nb + j] = m;
    }
    for (int e = 0; e < P; e++) {
        const double v = std::sqrt(d2[e]);
        if (a.member_dist && e < D) a.member_dist[(size_t)item * D + e] = ok[e] && W > 0 ? v : NAN;
        d2[e] = ok[e] ? v : 0.0;
    }
    a.n_mem[item] = n;
    a.n_day[item] = W;
    a.tsum[item] = tree(d2);
}

static void unit_pairs(const Case &c, const epi::EjArgs &a, long long u, std::vector<int> &hits)
{
    const long long item = u / a.tiles;
    const int tile = (int)(u % a.tiles);
    const int n = a.n_mem[item], W = a.n_day[item];
    if (n == 0 || W == 0) return;
    int I, J;
    epi::ejoint_tile_of(tile, a.nb, I, J);
    const int row = (int)(item / a.R), r = (int)(item % a.R);
    const unsigned long long mi = a.mask[(size_t)item * a.nb + I], mj = a.mask[(size_t)item * a.nb + J];
    std::vector<double> s(64, 0.0);
    for (int i = 0; i < 64; i++)
        for (int j = 0; j < 64; j++) {
            const bool on = ((mi >> i) & 1) && ((mj >> j) & 1) && (I != J || j > i);
            double d2 = 0.0;
            for (int w = 0; w < W && on; w++) {
                const int t = a.days[(size_t)item * a.wcap + w];
                const double d = c.form(row, t, r, I * 64 + i) - c.form(row, t, r, J * 64 + j);
                d2 = d2 + d * d;
            }
            s[i] = s[i] + (on ? std::sqrt(d2) : 0.0);
        }
    a.tile[(size_t)item * a.tiles + tile] = tree(s);
    hits[(size_t)item * a.tiles + tile]++;
}

static void unit_vario(const Case &c, const epi::EjArgs &a, long long u)
{
    const long long item = u / a.wcap;
    const int s = (int)(u % a.wcap), n = a.n_mem[item], W = a.n_day[item], D = a.D;
    if (n == 0 || W == 0 || s >= W) return;
    const int row = (int)(item / a.R), r = (int)(item % a.R);
    const int32_t *days = a.days + (size_t)item * a.wcap;
    int P = 64;
    while (P < D) P *= 2;
    double v = 0.0;
    for (int w = s + 1; w < W; w++) {
        if (a.max_lag > 0 && days[w] - days[s] > a.max_lag) break;
        std::vector<double> g(P, 0.0);
        for (int e = 0; e < D; e++)
            if ((a.mask[(size_t)item * a.nb + e / 64] >> (e % 64)) & 1) g[e] = gfun(c.form(row, days[s], r, e) - c.form(row, days[w], r, e), a.vs_order);
        const double term = gfun(c.y(row, days[s], r) - c.y(row, days[w], r), a.vs_order) - tree(g) / (double)n;
        v = v + term * term;
    }
    a.vrow[(size_t)item * a.wcap + s] = v;
}

static bool same(const void *p, const void *q, size_t n, bool f64)
{
    if (!f64) return std::memcmp(p, q, n * 4) == 0;
    const double *a = (const double *)p, *b = (const double *)q;
    for (size_t i = 0; i < n; i++)
        if (!((a[i] != a[i] && b[i] != b[i]) || std::memcmp(a + i, b + i, 8) == 0)) return false;
    return true;
}

static int run_case(const Case &c, int vs_order, int max_lag, long long cap, bool pairs)
{
    const int ro = c.rows + 1;
    const size_t items = (size_t)ro * c.R, col = items, md = items * c.D;
    std::vector<double> es(col), tt(col), sp(col), vs(col), dist(md), w_es(col), w_tt(col), w_sp(col), w_vs(col), w_dist(md);
    std::vector<int32_t> nm(col), nd(col), w_nm(col), w_nd(col);
    ejoint_ref(c.T, c.rows, c.R, c.D, c.Rt, c.f32, 1, c.k0, c.k1, vs_order, max_lag, c.src(), c.pop.data(), c.truth.data(), c.ts.data(),
               c.fd.data(), w_es.data(), w_tt.data(), w_sp.data(), w_vs.data(), w_nm.data(), w_nd.data(), w_dist.data());
    epi::EjArgs g{};
    g.T = c.T; g.rows = c.rows; g.rows_out = ro; g.R = c.R; g.D = c.D; g.Rt = c.Rt; g.f32 = c.f32; g.derive = 1; g.k0 = c.k0; g.k1 = c.k1;
    g.vs_order = vs_order; g.max_lag = max_lag;
    g.nb = (c.D + 63) / 64; g.tiles = g.nb * (g.nb + 1) / 2; g.wcap = c.k1 - c.k0;
    g.first_day = c.fd.data(); g.truth_series = c.ts.data();
    const size_t bytes = epi::ejoint_ws_size(items, (size_t)g.nb, (size_t)g.tiles, (size_t)g.wcap);
    void *ws = std::malloc(bytes);
    std::memset(ws, 0x7b, bytes);
    epi::ejoint_carve(g, ws, items, pairs, vs_order != 0);
    if ((char *)(g.days + items * g.wcap) != (char *)ws + bytes) { std::printf("the layout does not end at the workspace's size\n"); return 1; }
    g.es = pairs ? es.data() : nullptr; g.truth_term = tt.data(); g.spread_term = pairs ? sp.data() : nullptr;
    g.vs = vs_order ? vs.data() : nullptr; g.n_members = nm.data(); g.n_days = nd.data(); g.member_dist = dist.data();
    std::vector<int> hits(items * g.tiles, 0);
    long long launches = 0, seen = 0;
    auto sweep = [&](int which, long long units) {
        return epi::ejoint_for_units(units, cap, [&](long long u0, long long nu) {
            launches++;
            for (long long b = nu - 1; b >= 0; b--) {                 // last block first: nothing depends on the order
                if (which == 0) unit_members(c, g, u0 + b);
                else if (which == 2) unit_pairs(c, g, u0 + epi::ejoint_swizzle(b, nu), hits);
                else unit_vario(c, g, u0 + b);
                seen++;
            }
            return 0;
        });
    };
    sweep(0, (long long)items);
    if (pairs) sweep(2, (long long)items * g.tiles);
    if (vs_order) sweep(1, (long long)items * g.wcap);
    for (long long i = (long long)items - 1; i >= 0; i--) epi::ejoint_final_lane(g, (int)(i / c.R), (int)(i % c.R));
    int bad = 0;
    for (size_t i = 0; i < items && pairs; i++)
        for (int k = 0; k < g.tiles; k++) bad += hits[i * g.tiles + k] != (nm[i] > 0 && nd[i] > 0 ? 1 : 0);
    if (bad) std::printf("%d tile slots not written exactly once\n", bad);
    bad += !same(tt.data(), w_tt.data(), col, true) + !same(nm.data(), w_nm.data(), col, false) + !same(nd.data(), w_nd.data(), col, false) +
           !same(dist.data(), w_dist.data(), md, true);
    if (pairs) bad += !same(es.data(), w_es.data(), col, true) + !same(sp.data(), w_sp.data(), col, true);
    if (vs_order) bad += !same(vs.data(), w_vs.data(), col, true);
    const long long want = (long long)items + (pairs ? (long long)items * g.tiles : 0) + (vs_order ? (long long)items * g.wcap : 0);
    if (seen != want) { std::printf("%lld units seen, %lld expected\n", seen, want); bad++; }
    std::free(ws);
    if (bad) std::printf("case D=%d T=%d f32=%d vs_order=%d max_lag=%d cap=%lld: %d mismatches\n", c.D, c.T, c.f32, vs_order, max_lag, cap, bad);
    return bad;
}

int main()
{
    // the block -> unit map is a bijection for every launch size, the tile numbering the pinned order
    for (long long n = 1; n <= 70; n++) {
        std::vector<int> hit(n, 0);
        for (long long b = 0; b < n; b++) {
            const long long u = epi::ejoint_swizzle(b, n);
            if (u < 0 || u >= n || hit[u]++) { std::printf("swizzle(%lld, %lld) = %lld\n", b, n, u); return 1; }
        }
    }
    for (int nb = 1; nb <= 64; nb++) {
        int k = 0;
        for (int I = 0; I < nb; I++)
            for (int J = I; J < nb; J++, k++) {
                int i, j;
                epi::ejoint_tile_of(k, nb, i, j);
                if (i != I || j != J) { std::printf("tile_of(%d, %d)\n", k, nb); return 1; }
            }
        if (k != nb * (nb + 1) / 2) return 1;
    }
    const int Ds[7] = {1, 2, 63, 64, 65, 130, 300}, Ws[3] = {1, 2, 33};
    int cases = 0, bad = 0;
    for (int D : Ds)
        for (int W : Ws)
            for (int f32 = 0; f32 < 2; f32++)
                for (int variant = 0; variant < 2; variant++) {
                    const Case c = make_case(D, W, f32, variant);
                    bad += run_case(c, 1, 0, (long long)1 << 25, true);
                    bad += run_case(c, 2, 5, 4, true);                // launches of 4 units
                    bad += run_case(c, 2, 1, 7, false);               // no pair sum asked for: the tile pointer stays NULL
                    bad += run_case(c, 0, 0, 5, true);
                    cases += 4;
                }
    // D = 4 096: 64 blocks, 2 080 tiles an item, 24 960 tile units in launches of 1 003 (1 003 = 8 x 125 + 3: unequal groups of the
    // block -> unit map, a boundary inside every item, a ragged last launch of 888); float storage, W = 2
    {
        const Case c = make_case(4096, 2, 1, 1);
        bad += run_case(c, 1, 0, 1003, true);
        cases += 1;
    }
    if (bad) return 1;
    std::printf("ejoint emu ok: %d cases\n", cases);
    return 0;
}
