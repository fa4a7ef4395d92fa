// The host-pointer staging layer of epiekf.hip, which includes this file once (one translation unit: set_err, hip_fail and
// kMaxDevices are the ones defined there).  EVERY *_host entry point runs on it: HostCtx and its pool, with_ctx,
// place_and_run, HostIO, run_call and, for the calls without a placement search, run_host.
#pragma once
namespace epi {
constexpr size_t kStageBytes = (size_t)64 << 20;
constexpr size_t kStageSmallBytes = (size_t)8 << 20;   // dense calls above this go straight to / from the caller's arrays (HostIO::staged)
constexpr size_t kArenaKeepBytes = (size_t)2 << 30;   // an idle context keeps at most this much device memory
constexpr int kPoolPerDevice = 4;                      // idle contexts kept per device (64 MiB of pinned memory each)
struct HostCtx {
    int device = -1;
    hipStream_t stream = nullptr;
    char *arena = nullptr; size_t arena_bytes = 0;
    bool tuned = false;        // the arena is the fastest of several candidates (place_and_run): kept whatever its size
    char *pinned = nullptr;
    ~HostCtx()
    {
        if (device < 0) return;
        (void)hipSetDevice(device);
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        if (arena) (void)hipFree(arena);
        if (pinned) (void)hipHostFree(pinned);
    }
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= arena_bytes) return hipSuccess;
        hipError_t e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return e;
        if (arena) { (void)hipFree(arena); arena = nullptr; arena_bytes = 0; tuned = false; }
        size_t want = bytes + bytes / 4;
        e = hipMalloc((void **)&arena, want);
        if (e != hipSuccess) { (void)hipGetLastError(); want = bytes; e = hipMalloc((void **)&arena, want); }
        if (e != hipSuccess) { arena = nullptr; return e; }
        arena_bytes = want;
        return hipSuccess;
    }
};
static std::mutex g_pool_mu;
static std::vector<HostCtx *> g_pool;     // idle contexts of all devices
static HostCtx *ctx_acquire(int device, hipError_t *e)
{
    if (device < 0 || device >= kMaxDevices) { *e = hipErrorInvalidDevice; return nullptr; }
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        size_t pick = g_pool.size();               // the idle context of this device with the largest arena
        for (size_t i = 0; i < g_pool.size(); i++)
            if (g_pool[i]->device == device && (pick == g_pool.size() || g_pool[i]->arena_bytes > g_pool[pick]->arena_bytes)) pick = i;
        if (pick < g_pool.size()) { HostCtx *c = g_pool[pick]; g_pool.erase(g_pool.begin() + (long)pick); *e = hipSetDevice(device); return c; }
    }
    if ((*e = hipSetDevice(device)) != hipSuccess) return nullptr;
    HostCtx *c = new HostCtx();
    c->device = device;
    if ((*e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) { c->device = -1; delete c; return nullptr; }
    if ((*e = hipHostMalloc((void **)&c->pinned, kStageBytes, hipHostMallocDefault)) != hipSuccess) { delete c; return nullptr; }
    return c;
}
// back to the pool: a device keeps at most kPoolPerDevice idle contexts, and only ONE of them an arena above kArenaKeepBytes (the
// others hand theirs back to the device first; epi_host_pool_release frees everything).  Until round 6 every large arena was
// returned at once -- but hipFree takes ~30 ms per GiB on these boxes (24 GiB: 730 ms; hipMalloc 0.4 ms) and the next hipMalloc
// sometimes waits behind it for seconds: the headline sweep's host-pointer call took 16 ms or 0.7-6 s, the 9 375-chain shard with all
// outputs 118 or 200 ms, depending on whether the previous call's arena was still being returned (profiles/r06/host_calls.json).
static void ctx_release(HostCtx *c)
{
    bool big_kept = false;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (HostCtx *o : g_pool) big_kept = big_kept || (o->device == c->device && o->arena_bytes > kArenaKeepBytes);
    }
    if (c->arena_bytes > kArenaKeepBytes && !c->tuned && big_kept) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(c->arena);
        c->arena = nullptr; c->arena_bytes = 0;
    }
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        int same = 0;
        for (HostCtx *o : g_pool) same += o->device == c->device;
        if (same < kPoolPerDevice) { g_pool.push_back(c); return; }
    }
    delete c;
}
// body(cx) with a pooled context of `device`.  This scope owns two rules of a host call: the calling thread keeps its current
// device, and the context is released on every path.
template <class F>
static int with_ctx(int device, char *err, F &&body)
{
    int prev = 0;
    const bool have_prev = hipGetDevice(&prev) == hipSuccess;
    hipError_t e = hipSuccess;
    HostCtx *cx = ctx_acquire(device, &e);
    const bool ok = cx && e == hipSuccess;
    const int rc = ok ? body(cx) : EPI_OK;
    if (cx) ctx_release(cx);
    if (have_prev) (void)hipSetDevice(prev);
    if (ok) return rc;
    (void)hipGetLastError();       // reported here: the thread's next launch check must not find it
    return hip_fail(err, e, "hipSetDevice / context");
}

// Placement of a host call's arena (epi_batch_desc.placement_tries / epi_prescribe_desc.placement_tries, ABI 6).  Where the
// allocator puts the ~14 arrays a pass streams concurrently changes the forward kernel's and the smoother's time by 5-15 %
// (which PHYSICAL pages the allocation got: DESIGN.md 4, "Placement"); it is a property of the allocation and a host-pointer
// caller never sees the allocation.  When a call has to allocate a NEW arena and asks for `tries` > 1: the call's own kernels
// are run once untimed (clocks, code objects), then timed on up to `tries` candidate arenas, each allocated while the earlier
// ones are held (so that other memory is handed out) and each for at least ~15 ms of kernels; the fastest is kept -- with the
// complete results of its last run in it, nothing is computed again -- and stays with the pooled context whatever its size
// (epi_host_pool_release frees it).  compute(base, ev0, ev1) enqueues upload + kernels for the arena at `base` on the
// context's stream and records the two events (when given) around the kernels.
template <class F>
static int place_and_run(HostCtx *cx, size_t need, int tries, epi_placement_report *rep, F &&compute, char *err)
{
    if (rep) memset(rep, 0, sizeof *rep);
    const bool fresh = need > cx->arena_bytes;
    hipError_t e = cx->reserve(need);
    if (e != hipSuccess) return hip_fail(err, e, "device arena");
    if (tries <= 1 || !fresh) return compute(cx->arena, nullptr, nullptr);
    if (tries > EPI_PLACEMENT_MAX_TRIES) tries = EPI_PLACEMENT_MAX_TRIES;
    int rc = compute(cx->arena, nullptr, nullptr);
    if (rc != EPI_OK) return rc;
    if ((e = hipStreamSynchronize(cx->stream)) != hipSuccess) return hip_fail(err, e, "kernel execution (placement warm-up)");
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if ((e = hipEventCreate(&ev0)) != hipSuccess || (e = hipEventCreate(&ev1)) != hipSuccess) {
        if (ev0) (void)hipEventDestroy(ev0);
        return hip_fail(err, e, "hipEventCreate");
    }
    struct Cand { char *p; size_t bytes; float ms; };
    std::vector<Cand> cands;
    for (int i = 0; i < tries && rc == EPI_OK; i++) {
        Cand c{cx->arena, cx->arena_bytes, 0.0f};
        if (i > 0) {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < need + need / 16) { (void)hipGetLastError(); break; }
            if (hipMalloc((void **)&c.p, need) != hipSuccess) { (void)hipGetLastError(); break; }
            c.bytes = need;
        }
        float acc = 0.0f;
        int n = 0;
        do {
            rc = compute(c.p, ev0, ev1);
            if (rc != EPI_OK) break;
            if ((e = hipStreamSynchronize(cx->stream)) != hipSuccess) { rc = hip_fail(err, e, "kernel execution (placement try)"); break; }
            float ms = 0.0f;
            (void)hipEventElapsedTime(&ms, ev0, ev1);
            acc += ms; n++;
        } while (acc < 15.0f && n < 64);
        c.ms = n ? acc / (float)n : 0.0f;
        cands.push_back(c);
    }
    (void)hipEventDestroy(ev0); (void)hipEventDestroy(ev1);
    size_t best = 0;
    for (size_t i = 1; i < cands.size(); i++)
        if (rc == EPI_OK && cands[i].ms < cands[best].ms) best = i;
    if (rc != EPI_OK) best = 0;                       // an error: back to the first arena, the others are freed
    (void)hipStreamSynchronize(cx->stream);
    for (size_t i = 0; i < cands.size(); i++)
        if (i != best) (void)hipFree(cands[i].p);
    if (!cands.empty()) { cx->arena = cands[best].p; cx->arena_bytes = cands[best].bytes; }
    cx->tuned = rc == EPI_OK && cands.size() > 1;
    if (rep && rc == EPI_OK) {
        rep->tries = (int32_t)cands.size(); rep->chosen = (int32_t)best;
        for (size_t i = 0; i < cands.size(); i++) rep->ms[i] = cands[i].ms;
    }
    return rc;
}

// The arrays of one host call on one context: every array is `rows` rows of which this call moves a strided piece
// (columns [col0, col0 + cols) of a row of cols_full elements) to / from a contiguous device copy.  Calls whose arrays fit
// the pinned buffer are packed there and moved by ONE copy each way; larger ones go row block by row block.
struct HostIO {
    struct Piece { const char *src; char *dst; size_t rows, width, pitch, off; };
    std::vector<Piece> ins, outs;
    size_t off = 0, in_bytes = 0;
    size_t align = 256;
    static constexpr size_t kAbsent = (size_t)-1;      // the offset of an optional array the call does not have
    template <class T>
    static T *at(char *base, size_t o) { return o == kAbsent ? nullptr : (T *)(base + o); }
    size_t add_in(const void *host, size_t rows, size_t elem, size_t cols_full, size_t col0, size_t cols)
    {
        ins.push_back(Piece{host ? (const char *)host + col0 * elem : nullptr, nullptr, rows, cols * elem, cols_full * elem, off});
        const size_t o = off;
        off += (rows * cols * elem + align - 1) / align * align;
        in_bytes = off;
        return o;
    }
    size_t add_out(void *host, size_t rows, size_t elem, size_t cols_full, size_t col0, size_t cols)
    {
        // host == NULL: the device copy exists (kernels write it) but nothing is copied back
        outs.push_back(Piece{nullptr, host ? (char *)host + col0 * elem : nullptr, rows, cols * elem, cols_full * elem, off});
        const size_t o = off;
        off += (rows * cols * elem + align - 1) / align * align;
        return o;
    }
    // a whole dense array of `bytes` bytes, or kAbsent (NULL to the kernels) when the caller does not have it or it is empty
    size_t in(const void *host, size_t bytes) { return host && bytes ? add_in(host, 1, 1, bytes, 0, bytes) : kAbsent; }
    size_t out(void *host, size_t bytes) { return host && bytes ? add_out(host, 1, 1, bytes, 0, bytes) : kAbsent; }
    size_t reserve(size_t bytes)       // device-only scratch inside the same arena
    {
        off = (off + 255) & ~(size_t)255;
        const size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    }
    // The optional outputs of a struct S that is a plain list of them, spelled once: add_opt registers those the caller's
    // struct has (in table order), bind_opt points the device-side twin at their copies in the arena at `base`.
    template <class S, class T> struct Opt { T *S::*member; size_t rows; };
    template <class S, class T, size_t N>
    void add_opt(const S &host, const Opt<S, T> (&tab)[N], size_t (&o)[N], size_t cols)
    {
        for (size_t k = 0; k < N; k++)
            o[k] = host.*tab[k].member ? add_out(host.*tab[k].member, tab[k].rows, sizeof(T), cols, 0, cols) : kAbsent;
    }
    template <class S, class T, size_t N>
    static void bind_opt(S &dev, const Opt<S, T> (&tab)[N], const size_t (&o)[N], char *base)
    {
        for (size_t k = 0; k < N; k++) dev.*tab[k].member = at<T>(base, o[k]);
    }
    bool inputs_present() const
    {
        for (auto &p : ins) if (!p.src) return false;
        return true;
    }
    // (outputs must all have been added before the first reserve() for the staged download to be one copy; the code
    // below copies [in_bytes, out_end) where out_end is the end of the last output piece)
    size_t out_end() const { return outs.empty() ? in_bytes : outs.back().off + outs.back().rows * outs.back().width; }
    // A piece that covers whole rows (a call over all chains of the caller's arrays) is one contiguous range on both sides.
    static bool dense(const Piece &p) { return p.width == p.pitch || p.rows <= 1; }
    bool all_dense() const
    {
        for (auto &p : ins) if (!dense(p)) return false;
        for (auto &p : outs) if (p.dst && !dense(p)) return false;
        return true;
    }
    // Through the pinned buffer (ONE copy each way + the host's memcpy per row) or straight between the caller's arrays and
    // the device?  Measured on the pool's boxes (profiles/pcie_probe): a copy from / to pageable memory runs at 13 GB/s for 1
    // MiB and 54-56 GB/s from 16 MiB on, the pinned buffer at 37 / 55-57 GB/s, the host's memcpy out of it at 25 GB/s beyond
    // the caches -- so small calls (the reference's one-chain call: 0.66 MB in 11 arrays) are packed, large dense ones are
    // not, and strided pieces (a chain block of a multi-device call) are packed while they fit.
    bool staged() const
    {
        const size_t end = out_end();
        if (end > kStageBytes || in_bytes > kStageBytes) return false;
        return end <= kStageSmallBytes || !all_dense();
    }
    static hipError_t move(char *dev, const Piece &p, bool to_device, hipStream_t st)
    {
        if (dense(p))
            return to_device ? hipMemcpyAsync(dev, p.src, p.rows * p.width, hipMemcpyHostToDevice, st)
                             : hipMemcpyAsync(p.dst, dev, p.rows * p.width, hipMemcpyDeviceToHost, st);
        return to_device ? hipMemcpy2DAsync(dev, p.width, p.src, p.pitch, p.width, p.rows, hipMemcpyHostToDevice, st)
                         : hipMemcpy2DAsync(p.dst, p.pitch, dev, p.width, p.width, p.rows, hipMemcpyDeviceToHost, st);
    }
    hipError_t upload(HostCtx *cx, char *base) const
    {
        if (staged()) {
            for (auto &p : ins)
                for (size_t r = 0; r < p.rows; r++) memcpy(cx->pinned + p.off + r * p.width, p.src + r * p.pitch, p.width);
            return in_bytes ? hipMemcpyAsync(base, cx->pinned, in_bytes, hipMemcpyHostToDevice, cx->stream) : hipSuccess;
        }
        for (auto &p : ins) {
            const hipError_t e = move(base + p.off, p, true, cx->stream);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    // enqueues the copies back, waits for the stream, and (staged) scatters the rows into the caller's arrays
    hipError_t download(HostCtx *cx, const char *base) const
    {
        hipError_t e;
        if (staged()) {
            const size_t end = out_end();
            if (end > in_bytes && (e = hipMemcpyAsync(cx->pinned + in_bytes, base + in_bytes, end - in_bytes, hipMemcpyDeviceToHost, cx->stream)) != hipSuccess) return e;
            if ((e = hipStreamSynchronize(cx->stream)) != hipSuccess) return e;
            for (auto &p : outs)
                if (p.dst)
                    for (size_t r = 0; r < p.rows; r++) memcpy(p.dst + r * p.pitch, cx->pinned + p.off + r * p.width, p.width);
            return hipSuccess;
        }
        // Large pieces into memory the caller has never touched (a MEX gateway's freshly created outputs, np.empty) would be
        // faulted in page by page under the copy, by ONE thread inside the driver's pinning call: 14-17 GB/s instead of the
        // 33-52 GB/s resident pages reach (profiles/r06/host_calls.json).  A helper thread therefore populates the destination
        // of piece k + 1 on several threads (populate_pages) while piece k is on the wire; the copy of a piece is issued when
        // its pages are there.  Resident pages cost a page-table walk.
        std::vector<const Piece *> todo;
        size_t big = 0;
        for (auto &p : outs)
            if (p.dst) { todo.push_back(&p); if (span_bytes(p) >= kPopulateMinBytes) big++; }
        if (big == 0) {
            for (const Piece *p : todo)
                if ((e = move((char *)base + p->off, *p, false, cx->stream)) != hipSuccess) return e;
            return hipStreamSynchronize(cx->stream);
        }
        std::mutex mu;
        std::condition_variable cv;
        size_t ready = 0;                      // pieces [0, ready) are populated
        std::thread helper([&] {
            for (size_t k = 0; k < todo.size(); k++) {
                if (span_bytes(*todo[k]) >= kPopulateMinBytes) populate_pages(todo[k]->dst, span_bytes(*todo[k]), dense(*todo[k]));
                { std::lock_guard<std::mutex> lk(mu); ready = k + 1; }
                cv.notify_one();
            }
        });
        e = hipSuccess;
        for (size_t k = 0; k < todo.size() && e == hipSuccess; k++) {
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return ready > k; }); }
            e = move((char *)base + todo[k]->off, *todo[k], false, cx->stream);
        }
        helper.join();
        if (e != hipSuccess) return e;
        return hipStreamSynchronize(cx->stream);
    }
    // bytes of the caller's array a piece spans (a strided piece: first row's start to last row's end, gaps included -- they
    // belong to the same array)
    static size_t span_bytes(const Piece &p) { return p.rows ? (p.rows - 1) * p.pitch + p.width : 0; }
    static constexpr size_t kPopulateMinBytes = (size_t)8 << 20;
    // Make [p, p + bytes) resident and writable WITHOUT changing its contents: madvise(MADV_POPULATE_WRITE) per slice on up to
    // eight threads (page-table population scales with threads; one thread zeroes fresh pages at ~10 GB/s), falling back to
    // writing a byte of every page back to itself where the kernel does not know the advice (< 5.14; dense pieces only).
    static void populate_pages(char *p, size_t bytes, bool whole)
    {
        const size_t page = 4096;
        const uintptr_t a0 = (uintptr_t)p & ~(uintptr_t)(page - 1), a1 = ((uintptr_t)p + bytes + page - 1) & ~(uintptr_t)(page - 1);
        const size_t pages = (a1 - a0) / page;
        unsigned hw = std::thread::hardware_concurrency();
        size_t nt = bytes / ((size_t)16 << 20) + 1;
        const size_t cap = hw >= 16 ? 12 : (hw >= 4 ? hw / 2 : 1);
        if (nt > cap) nt = cap;
        // huge pages where the system grants them on request: 512 times fewer faults, the population is then bound by zeroing
        if (a1 - a0 >= ((size_t)4 << 20)) (void)madvise((void *)a0, a1 - a0, MADV_HUGEPAGE);
        auto slice = [=](size_t i) {
            const uintptr_t b = a0 + pages * i / nt * page, e = a0 + pages * (i + 1) / nt * page;
            if (e <= b) return;
#ifdef MADV_POPULATE_WRITE
            if (madvise((void *)b, e - b, MADV_POPULATE_WRITE) == 0) return;
#else
            if (madvise((void *)b, e - b, 23) == 0) return;
#endif
            // (a strided piece's gaps are other blocks' columns, which another device's copy may be writing right now: no
            // write-back there.)  The pages at the two ends may hold bytes outside [p, p + bytes): the byte touched is inside
            if (!whole) return;
            for (uintptr_t q = b; q < e; q += page) {
                uintptr_t t = q < (uintptr_t)p ? (uintptr_t)p : q;
                if (t >= (uintptr_t)p + bytes) break;
                volatile char *c = (volatile char *)t;
                *c = *c;
            }
        };
        std::vector<std::thread> th;
        for (size_t i = 1; i < nt; i++) th.emplace_back(slice, i);
        slice(0);
        for (auto &t : th) t.join();
    }
};

// One host call on a context: the arrays of `io` up, the kernels, the outputs back.  enqueue(base, stream) binds the device
// pointers for the arena at `base` and enqueues the kernels; place_and_run may ask for that on several candidate arenas, with
// ev0 / ev1 around the kernels, and every time the complete results are left in the arena.  This step owns the third rule of a
// host call: after upload() copies that read the caller's arrays / the pinned buffer may be in flight, so every error return
// waits for the stream first and neither is touched after the call has returned.
template <class F>
static int run_call(HostCtx *cx, const HostIO &io, int tries, epi_placement_report *report, char *err, F &&enqueue)
{
    hipError_t e = hipSuccess;
    auto compute = [&](char *base, hipEvent_t ev0, hipEvent_t ev1) -> int {
        if ((e = io.upload(cx, base)) != hipSuccess) { (void)hipStreamSynchronize(cx->stream); return hip_fail(err, e, "upload"); }
        if (ev0) (void)hipEventRecord(ev0, cx->stream);
        const int rc = enqueue(base, cx->stream);
        if (rc != EPI_OK) { (void)hipStreamSynchronize(cx->stream); return rc; }
        if (ev1) (void)hipEventRecord(ev1, cx->stream);
        return EPI_OK;
    };
    const int rc = place_and_run(cx, io.off + 256, tries, report, compute, err);
    if (rc != EPI_OK) return rc;
    if ((e = io.download(cx, cx->arena)) != hipSuccess) return hip_fail(err, e, "kernel execution / download");
    return EPI_OK;
}

// Every host call without a placement search: a pooled context of `device`, and the call on it.
template <class F>
static int run_host(int device, const HostIO &io, char *err, F &&enqueue)
{
    return with_ctx(device, err, [&](HostCtx *cx) { return run_call(cx, io, 0, nullptr, err, enqueue); });
}
}   // namespace epi
