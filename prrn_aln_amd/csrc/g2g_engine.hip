// g2g_engine.hip -- host side of level 0 (include/g2g.h): packs g2g_problem batches into one HBM arena,
// launches the forward + backtrack kernels (g2g_kernels.hip) on the context's stream and fetches results.
// No CPU fallback lives here: without a usable HIP device every entry point fails with G2G_ERR_NODEVICE.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <map>
#include <vector>
#include <thread>
#include <atomic>
#include <mutex>
#include <memory>
#include <algorithm>
#include <chrono>
#ifndef G2G_TU_ALL
#define G2G_TU_V1 1                 // this unit emits the v1 / traceback / calcSpScore kernels and the f3 / pairsum kernels; the strip
#endif                              // kernels come from the g2g_tu_*.hip units (g2g_device.h)
#include "../../include/g2g.h"
#include "g2g_device.h"
#include "g2g_internal.h"
#include "g2g_plan.h"                // the variant table and the plans of a run (host only)

#include "g2g_kernels.hip"          // one translation unit: kernels + launcher (no -fgpu-rdc needed)
#include "g2g_strip.h"            // primitives and scaffold of the strip kernels below
#include "g2g_kernels_v2.hip"
#include "g2g_kernels_v3.hip"
#include "g2g_kernels_v6.hip"
#include "g2g_kernels_v7.hip"
#include "g2g_kernels_v8.hip"

static thread_local std::string g_err;
// process-wide totals over every context (g2g_process_counters): runs, waits that gave up, DPs re-run, of those on v1, gaps seen
// by waiting waves, and the part of [1] / [2] that belongs to batches prepared with the INJECT_STALL test hook
static std::atomic<long long> g_tot[8];
static std::mutex g_report_mx;
static std::string g_last_report;
void g2g_set_error(const char *fmt, const char *a)
{
    char buf[512];
    snprintf(buf, sizeof buf, fmt, a);
    g_err = buf;
}
void g2g_errorf(const char *who, const char *fmt, ...)
{
    char buf[512];
    const int at = snprintf(buf, sizeof buf, "%s: ", who);
    va_list ap;
    va_start(ap, fmt);
    if (at >= 0 && (size_t) at < sizeof buf) vsnprintf(buf + at, sizeof buf - (size_t) at, fmt, ap);
    va_end(ap);
    g_err = buf;
}
extern "C" const char *g2g_last_error(void) { return g_err.c_str(); }
extern "C" int g2g_abi_version(void) { return G2G_ABI_VERSION; }

#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    g2g_set_error("HIP error: %s", hipGetErrorString(e_)); return G2G_ERR_DEVICE; } } while (0)

struct g2g_ctx {
    int device;
    int ok;
    hipStream_t stream;
    hipStream_t vstream[G2G_NVS];   // the persistent launches of a run are independent of each other: each takes the next of these streams
                                    // (round 2 gave some pairs of launches one stream by table, and a sweep was the SUM of their times)
    hipEvent_t ev[4];
    hipEvent_t vev[G2G_NVS + 1];    // join events of those streams; [G2G_NVS]: the fork event
    char *stage; size_t stage_cap;  // pinned host staging buffer of g2g_batch_prepare, kept between calls
    void *sp_slots; size_t sp_slots_cap;   // g2g_batch_spscore: the slots of the streamed walks (kept between calls, grows)
    long long n_gaps; double max_gap_ms;   // waiters that found themselves off the machine for more than 4 ms between two looks at the clock (g2g_wait_ge), longest such gap
    double rt_ticks_per_ms;         // rate of s_memrealtime on this device, measured at g2g_create (the waits' time limit is wall clock)
    std::map<std::string, std::pair<bool, std::string>> opt;   // g2g_set_option: name -> (present, value); see g2g_opt
    // Device memory belongs to the CONTEXT: every buffer a batch needs (arena, tile table, flags, the strips' column-score
    // scratch, list twins, the walks' workspace) is a block of this pool, handed back when the batch is freed and reused by the
    // next batch of similar size.  No hipMalloc / hipFree happens between the first and the last persistent launch of a run
    // (g2g_batch_run sizes and takes everything in a dry pass before it launches anything), and a refinement window -- one
    // batch per window -- allocates nothing once the pool holds its sizes.  Contents are as undefined as a fresh allocation's.
    struct DevBlock { char *p; size_t cap; };
    std::vector<DevBlock> pool;     // free blocks
    hipStream_t sp_stream; hipEvent_t sp_ev; void *sp_slots2; size_t sp_slots2_cap;    // the walks that run beside the DPs (g2g_batch_spscore_begin)
    long long n_dev_malloc, n_dev_free, n_pool_hits;   // hipMalloc / hipFree calls made for the pool, requests served from it
    int ncu;                        // compute units of the device
    std::shared_ptr<int> alive;     // 1 while the context exists: device slabs that outlive it (twins held by g2g_group objects) free themselves
    long long n_runs, n_timeouts, n_recovered, n_v1;   // g2g_ctx_counters: batch runs, waits that ran into the limit, DPs re-run, of those on v1
    struct MStream { int lo, n; hipStream_t s; unsigned long long used; };
    std::vector<MStream> mstream;   // streams confined to a share of the CUs (units lo .. lo + n - 1 of 32; see cu_share_stream)
    unsigned long long mstamp;
    long long n_mstreams;           // CU-mask streams created so far
    std::string last_timeout;       // report of the last recovered time-out (g2g_ctx_last_timeout)
};

// Tuning and diagnostic switches belong to a context (g2g_set_option / g2g_get_option); a name a context has not set
// reads the process environment variable G2G_<NAME>, so the environment only supplies defaults.  A switch is "on" when it
// has a value (any, also the empty string) and "off" when g2g_set_option was given NULL for it.
static const char *g2g_opt(const g2g_ctx *c, const char *name)
{
    if (c) {
        auto it = c->opt.find(name);
        if (it != c->opt.end()) return it->second.first ? it->second.second.c_str() : 0;
    }
    char env[96];
    snprintf(env, sizeof env, "G2G_%s", name);
    return getenv(env);
}
// A stage's timing switch leaves what it measured as an option of the context ("%.6f" milliseconds); add: summed onto the
// value the option holds.  g2g_note_events: the time between two recorded events of a stream that has been waited for.
static void g2g_note_ms(g2g_ctx *c, const char *name, double ms, bool add)
{
    if (add) { const char *old = g2g_opt(c, name); if (old) ms += atof(old); }
    char buf[32];
    snprintf(buf, sizeof buf, "%.6f", ms);
    c->opt[name] = std::make_pair(true, std::string(buf));
}
static hipError_t g2g_note_events(g2g_ctx *c, const char *name, hipEvent_t from, hipEvent_t to, bool add)
{
    float ms = 0;
    const hipError_t e = hipEventElapsedTime(&ms, from, to);
    g2g_note_ms(c, name, ms, add);
    return e;
}
extern "C" int g2g_set_option(g2g_ctx *c, const char *name, const char *value)
{
    if (!c || !name || !*name || strlen(name) > 64) { g2g_set_error("g2g_set_option: %s", "bad argument"); return G2G_ERR_ARG; }
    if (!strncmp(name, "G2G_", 4)) name += 4;
    c->opt[name] = std::make_pair(value != 0, std::string(value ? value : ""));
    return G2G_OK;
}
extern "C" void g2g_reset_options(g2g_ctx *c) { if (c) c->opt.clear(); }
extern "C" const char *g2g_get_option(const g2g_ctx *c, const char *name)
{
    if (!name) return 0;
    if (!strncmp(name, "G2G_", 4)) name += 4;
    return g2g_opt(c, name);
}

extern "C" __global__ void g2g_clock_kernel(unsigned long long *out) { *out = __builtin_amdgcn_s_memrealtime(); }

// The first HIP call of a process initialises the runtime, and that initialisation draws from / reseeds glibc's random()
// state (measured: srand(1); rand(); <HIP init>; rand() no longer gives 846930886).  The reference seeds its own generator
// from rand() (McRand, src/randiv.cc:41-50) and breaks ties with rand() elsewhere, so a drop-in library must leave that
// state alone: HIP initialises against a private state array, the caller's is put back.  (Later HIP calls do not touch it.)
struct RandStateGuard {
    char buf[256]; char *prev;
    RandStateGuard() { prev = initstate(1u, buf, sizeof buf); }
    ~RandStateGuard() { if (prev) setstate(prev); }
};

extern "C" g2g_ctx *g2g_create(int device)
{
    RandStateGuard keep_host_rand;
    // one hardware queue per concurrent persistent launch: HIP multiplexes a process's streams onto GPU_MAX_HW_QUEUES queues (4 by
    // default) and reads the variable when it initialises -- which this call does if nothing in the process did before
    // (setenv is not safe against a concurrent getenv in another thread: a multithreaded host either sets GPU_MAX_HW_QUEUES
    //  itself before it starts its threads -- the Python loader does -- or calls g2g_create before it starts them; the variable
    //  is only written here when it is unset)
    if (!getenv("GPU_MAX_HW_QUEUES")) setenv("GPU_MAX_HW_QUEUES", "8", 0);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        g2g_set_error("%s", "no HIP device visible");
        return NULL;
    }
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    if (device >= ndev) { g2g_set_error("%s", "device index out of range"); return NULL; }
    if (hipSetDevice(device) != hipSuccess) { g2g_set_error("%s", "hipSetDevice failed"); return NULL; }
    g2g_ctx *c = new g2g_ctx();
    c->device = device;
    c->ok = 0;
    c->stage = 0; c->stage_cap = 0;
    c->n_dev_malloc = c->n_dev_free = c->n_pool_hits = 0; c->ncu = 256;
    c->alive = std::make_shared<int>(1);
    c->n_runs = c->n_timeouts = c->n_recovered = c->n_v1 = 0;
    c->n_gaps = 0; c->max_gap_ms = 0; c->n_mstreams = 0;
    c->sp_slots = 0; c->sp_slots_cap = 0; c->sp_stream = 0; c->sp_ev = 0; c->sp_slots2 = 0; c->sp_slots2_cap = 0;
    c->mstamp = 0;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; g2g_set_error("%s", "stream"); return NULL; }
    for (int i = 0; i < 4; ++i) hipEventCreate(&c->ev[i]);
    for (int i = 0; i < G2G_NVS; ++i) hipStreamCreateWithFlags(&c->vstream[i], hipStreamNonBlocking);
    for (int i = 0; i < G2G_NVS + 1; ++i) hipEventCreateWithFlags(&c->vev[i], hipEventDisableTiming);
    // the code object must contain an image for this GPU (the library is built for gfx950 only)
    hipFuncAttributes fa;
    hipError_t e = hipFuncGetAttributes(&fa, (const void *) g2g_forward_kernel);
    if (e != hipSuccess) {
        g2g_set_error("no gfx950 kernel image usable on this device: %s", hipGetErrorString(e));
        (void) hipGetLastError();
    } else c->ok = 1;
    if (c->ok) {
        hipDeviceProp_t pr;
        if (hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0) c->ncu = pr.multiProcessorCount;
        // every strip kernel may use the whole LDS of a CU: said once, here, so that no run changes a function attribute
        // between two persistent launches
        const void *fns[] = {(const void *) g2g_v2_hf2, (const void *) g2g_v2_hf3, (const void *) g2g_v2_pf2, (const void *) g2g_v2_pf3,
                             (const void *) g2g_v3_hf2, (const void *) g2g_v3_hf3, (const void *) g2g_v3r_hf2, (const void *) g2g_v3r_hf3,
                             (const void *) g2g_v6_pf2, (const void *) g2g_v6_pf3};
        for (const void *f : fns)
            if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int) (160 * 1024)) != hipSuccess) (void) hipGetLastError();
    }
    c->rt_ticks_per_ms = 1.0e5;                              // nominal 100 MHz; measured below
    if (c->ok) {
        unsigned long long *d = 0, t[2] = {0, 0};
        if (hipMalloc((void **) &d, sizeof(unsigned long long)) == hipSuccess) {
            std::chrono::steady_clock::time_point h[2];
            for (int k = 0; k < 2; ++k) {
                hipLaunchKernelGGL(g2g_clock_kernel, dim3(1), dim3(1), 0, c->stream, d);
                hipStreamSynchronize(c->stream);
                h[k] = std::chrono::steady_clock::now();
                hipMemcpy(&t[k], d, sizeof t[k], hipMemcpyDeviceToHost);
                if (k == 0) std::this_thread::sleep_for(std::chrono::milliseconds(25));
            }
            const double ms = std::chrono::duration<double, std::milli>(h[1] - h[0]).count();
            if (t[1] > t[0] && ms > 1) c->rt_ticks_per_ms = (double) (t[1] - t[0]) / ms;
            hipFree(d);
        }
        (void) hipGetLastError();
    }
    return c;
}

extern "C" void g2g_destroy(g2g_ctx *c)
{
    if (!c) return;
    // G2G_LOG_FILE (plain environment): the phases of the tear-down with their times, appended to that file (a test runner captures
    // stderr; a tear-down that does not come back must still say where it stands)
    FILE *lf = getenv("G2G_LOG_FILE") ? fopen(getenv("G2G_LOG_FILE"), "a") : 0;
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!lf) return;
        fprintf(lf, "[g2g destroy %p] %-22s %8.1f ms\n", (void *) c, what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        fflush(lf);
    };
    hipSetDevice(c->device);
    lap("begin");
    // Order: everything idle first; then the MEMORY goes while every stream it was ever used on still exists (hipFree waits for the
    // device: round 4 saw tear-downs that never came back when some fifty pool blocks were freed behind destroyed CU-mask streams);
    // the streams and events last.
    hipDeviceSynchronize();
    lap("device idle");
    *c->alive = 0;
    for (auto &bk : c->pool) hipFree(bk.p);
    c->pool.clear();
    if (c->sp_slots) hipFree(c->sp_slots);
    if (c->sp_slots2) hipFree(c->sp_slots2);
    lap("device pool");
    if (c->stage) hipHostFree(c->stage);
    lap("pinned staging");
    for (int i = 0; i < 4; ++i) hipEventDestroy(c->ev[i]);
    for (int i = 0; i < G2G_NVS + 1; ++i) hipEventDestroy(c->vev[i]);
    if (c->sp_ev) hipEventDestroy(c->sp_ev);
    lap("events");
    for (auto &m : c->mstream) hipStreamDestroy(m.s);
    lap("CU-share streams");
    for (int i = 0; i < G2G_NVS; ++i) hipStreamDestroy(c->vstream[i]);
    if (c->sp_stream) hipStreamDestroy(c->sp_stream);
    lap("launch streams");
    hipStreamDestroy(c->stream);
    lap("main stream");
    if (lf) fclose(lf);
    delete c;
}

extern "C" int g2g_device_ok(g2g_ctx *c) { return c && c->ok; }
extern "C" void g2g_free(void *p) { free(p); }

// ---- the context's device-memory pool ----------------------------------------------------------------------------------
// Requests of 64 MB and more (arenas, the strips' scratch) take the smallest free block that fits, whatever its size -- batch
// sizes of a refinement loop vary call by call --; smaller ones only blocks of at most four times the request (a tile table
// must not sit on an arena).  New blocks are rounded up (1/8 for large ones) so that the next batch, a little larger, still
// fits.  The pool is trimmed when it holds more than 48 free blocks or when the device runs out of memory.
static const size_t POOL_BIG = (size_t) 64 << 20;
static void pool_trim(g2g_ctx *c, size_t keep_blocks)
{
    while (c->pool.size() > keep_blocks) {                   // smallest first (the big ones are the expensive ones to get back)
        size_t k = 0;
        for (size_t i = 1; i < c->pool.size(); ++i) if (c->pool[i].cap < c->pool[k].cap) k = i;
        hipFree(c->pool[k].p); ++c->n_dev_free;
        c->pool.erase(c->pool.begin() + k);
    }
}
static void *pool_take(g2g_ctx *c, size_t bytes, size_t *cap)
{
    if (!bytes) bytes = 16;
    const bool cache = !g2g_opt(c, "NO_ARENA_CACHE");
    int best = -1;
    if (cache)
        for (size_t i = 0; i < c->pool.size(); ++i) {
            const size_t cp = c->pool[i].cap;
            if (cp < bytes) continue;
            if (bytes < POOL_BIG && cp > std::max(4 * bytes, (size_t) 1 << 16)) continue;
            if (best < 0 || cp < c->pool[best].cap) best = (int) i;
        }
    if (best >= 0) {
        void *r = c->pool[best].p;
        *cap = c->pool[best].cap;
        c->pool.erase(c->pool.begin() + best);
        ++c->n_pool_hits;
        return r;
    }
    size_t want = bytes >= POOL_BIG ? bytes + bytes / 8 : bytes >= 4096 ? bytes + bytes / 4 : 4096;
    want = (want + 255) & ~(size_t) 255;
    if (!cache) want = bytes;
    void *r = 0;
    if (want >= POOL_BIG && cache) {                         // a new large block: the free large ones were all too small -- give them back first
        for (size_t i = c->pool.size(); i-- > 0; )
            if (c->pool[i].cap >= POOL_BIG) { hipFree(c->pool[i].p); ++c->n_dev_free; c->pool.erase(c->pool.begin() + i); }
    }
    hipError_t e = hipMalloc(&r, want);
    if (e != hipSuccess && want > bytes) { (void) hipGetLastError(); want = bytes; e = hipMalloc(&r, want); }
    if (e != hipSuccess) { (void) hipGetLastError(); pool_trim(c, 0); e = hipMalloc(&r, want); }
    if (e != hipSuccess) { (void) hipGetLastError(); return 0; }
    ++c->n_dev_malloc;
    *cap = want;
    return r;
}
static void pool_give(g2g_ctx *c, void *p, size_t cap)
{
    if (!p) return;
    if (g2g_opt(c, "NO_ARENA_CACHE")) { hipFree(p); ++c->n_dev_free; return; }
    g2g_ctx::DevBlock bk; bk.p = (char *) p; bk.cap = cap;
    c->pool.push_back(bk);
    if (c->pool.size() > 48) pool_trim(c, 32);
}
extern "C" void g2g_ctx_mem_counters(const g2g_ctx *c, long long out[4])
{
    if (!out) return;
    size_t held = 0;
    if (c) for (auto &bk : c->pool) held += bk.cap;
    out[0] = c ? c->n_dev_malloc : 0; out[1] = c ? c->n_dev_free : 0; out[2] = c ? c->n_pool_hits : 0; out[3] = (long long) held;
}

// ---- batch -----------------------------------------------------------------------------------

struct Blob {                       // host image of the input part of the arena
    // (a raw realloc'ed buffer: a std::vector zero-fills and copies 1.2 GB of profiles again and again while it
    // grows -- that was 1.1 s of a 1.3 s prepare for the bench sweep)
    char *p; size_t sz, cap;
    struct Copy { size_t off; const void *src; size_t bytes; };
    std::vector<Copy> later;        // big copies are deferred and done by a few host threads at once (flush)
    g2g_ctx *owner;                 // the buffer is the context's pinned staging area: it outlives the Blob (no page
                                    // faults and a DMA-able source on every call after the first)
    int pack_threads;               // option PACK_THREADS (0: one per core, at most 16)
    explicit Blob(g2g_ctx *c) : p(c->stage), sz(0), cap(c->stage_cap), owner(c), pack_threads(0), oom(false) {}
    ~Blob() { owner->stage = p; owner->stage_cap = cap; }
    Blob(const Blob &) = delete;
    Blob &operator=(const Blob &) = delete;
    bool oom;
    void grow(size_t need)
    {
        if (need <= cap || oom) return;
        const size_t c = need + need / 8 + ((size_t) 1 << 20);
        char *q = 0;
        if (hipHostMalloc((void **) &q, c, hipHostMallocDefault) != hipSuccess || !q) { (void) hipGetLastError(); oom = true; return; }
        if (sz) memcpy(q, p, sz);
        if (p) hipHostFree(p);
        p = q; cap = c;
    }
    void extend(size_t newsize) { if (newsize <= sz) return; grow(newsize); if (oom) return; memset(p + sz, 0, newsize - sz); sz = newsize; }
    size_t put_now(const void *src, size_t bytes)      // put() of a source that does not live until flush(): copied here, whatever its size
    {
        const size_t off = put(0, 0);
        extend(off + bytes);
        if (oom) return 0;
        if (bytes) memcpy(p + off, src, bytes);
        return off;
    }
    size_t put(const void *src, size_t bytes)
    {
        const size_t off = (sz + 15) & ~(size_t) 15;
        grow(off + bytes);
        if (oom) return 0;
        if (off > sz) memset(p + sz, 0, off - sz);
        if (bytes >= ((size_t) 64 << 10)) { Copy c = {off, src, bytes}; later.push_back(c); }
        else if (bytes) memcpy(p + off, src, bytes);
        sz = off + bytes;
        return off;
    }
    void flush()
    {
        if (later.empty() || oom) return;
        unsigned nthr = std::thread::hardware_concurrency();
        if (nthr > 16) nthr = 16;
        if (nthr < 1) nthr = 1;
        if (pack_threads >= 1 && pack_threads <= 64) nthr = (unsigned) pack_threads;
        if (nthr > later.size()) nthr = (unsigned) later.size();
        std::atomic<size_t> next(0);
        auto work = [&]() { for (size_t k; (k = next.fetch_add(1)) < later.size(); ) memcpy(p + later[k].off, later[k].src, later[k].bytes); };
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nthr; ++t) th.emplace_back(work);
        work();
        for (auto &t : th) t.join();
        later.clear();
    }
    char *data() { return p; }
    size_t size() const { return sz; }
};

// the problem index of a batch sits in a grid y / z dimension of some launches (limit 65535)
#define G2G_MAX_BATCH 32768
extern "C" void g2g_batch_free(g2g_batch *b);
// Variant slots (one queue, one persistent launch each): G2G_VARIANT of g2g_plan.h says which kernel each one is.
static_assert(G2G_PLAN_HDR == G2G_HDR, "g2g_plan.h and g2g_strip.h disagree about the queue heads");
struct g2g_batch {
    g2g_ctx *ctx;
    int n;
    std::vector<DevProb> dp;        // host copy with device pointers
    std::vector<int> status;
    std::vector<long long> cells;
    std::vector<size_t> out_off;    // per problem: offset of {score, ntrace, otrace} block
    std::vector<int> tcap;
    size_t out_lo, out_hi;          // the output blocks occupy arena [out_lo, out_hi)
    std::vector<long long> rr1;     // b.left - a.left + b.right - a.right per problem
    char *d_arena;
    size_t arena_bytes, in_bytes;
    size_t arena_cap;               // bytes actually allocated behind d_arena (>= arena_bytes when the arena was reused)
    DevProb *d_probs;
    int *d_idx1, *d_idx2;           // problems run by the v1 / v2 forward kernel
    int *d_idxp; int np;            // problems whose boundary chains run in the prologue kernel (the others: as queue entries)
    int n1, n2;
    int nsimmat;                    // DPs that read a column-score matrix (tile-mode test configurations): only then the matrix kernels run
    size_t lds2;                    // dynamic LDS bytes of the v2 launch
    size_t lds2p;                   // ... of the v2 prologue launch
    int v2_maxrows;                 // longest a-range among the v2 problems
    int v2_maxcols;                 // longest b-range ...
    size_t simtile_lds;             // LDS of the tiled column-score kernel
    size_t tiles_cap, flags_cap;    // pool blocks behind d_tiles / d_flags
    V2Tile *d_tiles;                // tiles: per variant (v2: hf2, hf3, pf2, pf3; v3: the same four) a queue ordered by wavefront i + j
    int var_off[G2G_NVAR + 1];      // variant v owns tiles [var_off[v], var_off[v+1])
    long long var_cells[G2G_NVAR];       // in-band cells of the DPs of variant v (the CU shares of a run are proportional to cells x cost)
    V3Lds v3lds[8];                 // LDS plan of the v3 variants
    V6Lds v6lds[6];                 // LDS plans of the v6 (_pf, one lane per cell, rank-form merges) launches: Noll 2, 3 x footprint class A / B / C
    int v2_cols;
    int v2_threads;                 // workgroup size of the v2 kernels: 256 (32-row strips) or 128 (16-row strips)
    int v2_sweep;                   // v2 (_pf): the same
    int v3_sweep;                   // v3r (_hf): strips as a pipeline with progress counters (one tile per strip)
    int v3_cols;                    // columns per v3 tile
    int *d_flags;                   // [0, G2G_HDR) queue heads, [G2G_HDR, +4) header of the waits, then tile flags / progress counters, then per-DP fail flags
    int nflags, gen;
    std::vector<int> flags0;        // initial contents of d_flags (re-uploaded when the 11-bit generation of the progress counters wraps)
    long long ntiles;
    float fwd_ms, tb_ms;
    double *simscr[G2G_NVAR]; size_t simscr_cap[G2G_NVAR];
    unsigned *twin[6]; size_t twin_cap[6];       // per v6 launch: HBM image of the dynamic lists' parts beyond their inline LDS slots
    bool v6_on;                     // this batch is large enough for v6 (else its _pf DPs go to v2: shorter critical path)
    int hdr_img[G2G_HDR + G2G_HDRN];       // host image of the queue heads + wait header of the current run
    std::vector<const g2g_problem *> src;        // the caller's problems (kept alive by the caller until the batch is freed): a DP
                                                 // that lost a wait is re-run from here on the non-polling kernel
    std::vector<char> ib;                        // per problem: runs on a bonus-aware strip kernel (g2g_v7_*_ib / g2g_v2_*_ib / g2g_v8_*_ib)
    std::vector<int> path_rec;                   // kernel generation of a recovered DP's successful re-run (g2g_batch_paths)
    int xq_off;                                  // offset in d_flags of the queue heads of the variant slots G2G_HDR .. G2G_NVAR - 1
    int fail_off;                                // offset of the per-DP fail flags in d_flags
    int dump_off;                                // offset of the time-out dump area in d_flags (0: none)
    int n_recovered;                             // DPs re-run after a time-out, over the life of the batch
    int last_timeouts, last_recovered;           // the same for the last g2g_batch_run: waits that gave up, DPs re-run
    std::vector<g2g_result> recovered;           // results of re-run DPs (trace owned by the batch until fetched)
    std::vector<char> was_recovered;
    bool injected;                               // prepared with the INJECT_STALL test hook: its time-outs are expected ones
    bool is_retry;                               // a batch of DPs that lost a wait, re-run on the ordinary kernels; ITS time-outs go to v1
    bool force_v1;                               // recovery batches: everything on g2g_forward_kernel   // per sweep-mode launch: strip-local column-score blocks (3 x 32 KB per workgroup)
};

// the per-family arrays of a batch and the queue head of a slot, by slot (G2G_VARIANT says which family a slot is)
static inline V3Lds &batch_v3lds(g2g_batch *b, int slot) { return b->v3lds[variant_v3_index(slot)]; }
static inline V6Lds &batch_v6lds(g2g_batch *b, int slot) { return b->v6lds[variant_v6_index(slot)]; }
static inline unsigned *&batch_twin(g2g_batch *b, int slot) { return b->twin[variant_v6_index(slot)]; }
static inline size_t &batch_twin_cap(g2g_batch *b, int slot) { return b->twin_cap[variant_v6_index(slot)]; }
static inline int *batch_qhead(g2g_batch *b, int slot) { return slot < G2G_HDR ? b->d_flags + slot : b->d_flags + b->xq_off + (slot - G2G_HDR); }

static int kind_of(int alnmode)
{
    switch (alnmode) {
    case G2G_NGP_ALB: case G2G_NGP_ALN: return 0;
    case G2G_HLF_ALB: case G2G_RHF_ALB: return 1;
    case G2G_GPF_ALB: return 2;
    case G2G_NTV_ALB: return 3;
    }
    // The other rectangular modes (HLF / RHF / GPF / NTV_ALN) are NOT on this path, for a reason: Fwd2c::forwardA starts every row
    // with `*hdiag = *h` (src/fwd2c.h:247), a struct assignment that makes the diagonal record SHARE the left boundary record's
    // gap-state arrays; from then on a growing triangle of records is updated in place through one array, in the row-major order
    // of the reference's loop.  The restatement in oracle/ reproduces that (all 24 rectangular goldens, every record type), but the
    // result depends on a sequential order no anti-diagonal sweep has.  DPunit carries no arrays: NGP_ALN is exact and built.
    return -1;
}
static bool is_rect(int alnmode) { return alnmode == G2G_NGP_ALN; }

static int check_problem(const g2g_problem *p)
{
    if (!p) return G2G_ERR_ARG;
    int kind = kind_of(p->alnmode);
    if (kind < 0) return G2G_ERR_MODE;           // rectangular (_ALN) and spliced engines: not on this path yet
    if (p->noll != 2 && p->noll != 3) return G2G_ERR_ARG;
    const g2g_side *s[2] = {&p->a, &p->b};
    for (int k = 0; k < 2; ++k) {
        if (s[k]->many < 1 || s[k]->len < 1 || !s[k]->seq || !s[k]->thk) return G2G_ERR_ARG;
        if (s[k]->left < 0 || s[k]->right > s[k]->len || s[k]->left >= s[k]->right) return G2G_ERR_ARG;
    }
    if (is_rect(p->alnmode)) {                       // the caller's band is not read: the DP covers the rectangle
        if (p->spb_fact != 0 && p->a.npfq > 0 && p->b.npfq > 0) return G2G_ERR_MODE;      // (the intron bonus table is forwardB's)
    } else {
    if (p->up < p->lw) return G2G_ERR_ARG;
    // the end corner must lie inside the band (stripe() guarantees it, aln2.cc:156-174)
    const int re_ = p->b.right - p->a.right, rs_ = p->b.left - p->a.left;
    if (re_ < p->lw || re_ > p->up || rs_ < p->lw || rs_ > p->up) return G2G_ERR_ARG;
    }
    if (kind == 1 && !p->a.has_gfq) return G2G_ERR_ARG;
    if (kind == 2 && (!p->a.has_gfq || !p->b.has_gfq)) return G2G_ERR_ARG;
    if (kind == 3 && (!p->a.gapdens || !p->b.gapdens || !p->a.postgapdens || !p->b.postgapdens || !p->crg2_kind)) return G2G_ERR_ARG;
    switch (p->sim2_kind) {
    case G2G_SIM00: case G2G_SIM11: case G2G_SIM12I: case G2G_SIM21I: case G2G_SIM22I: break;
    case G2G_SIM12W: if (!p->b.weight) return G2G_ERR_ARG; break;
    case G2G_SIM21W: if (!p->a.weight) return G2G_ERR_ARG; break;
    case G2G_SIM22W: if (!p->a.weight || !p->b.weight) return G2G_ERR_ARG; break;
    case G2G_SIM13: case G2G_SIM23I: if (!p->b.pseq) return G2G_ERR_ARG; break;
    case G2G_SIM23W: if (!p->b.pseq || !p->a.weight) return G2G_ERR_ARG; break;
    case G2G_SIM31: case G2G_SIM32I: if (!p->a.pseq) return G2G_ERR_ARG; break;
    case G2G_SIM32W: if (!p->a.pseq || !p->b.weight) return G2G_ERR_ARG; break;
    case G2G_SIM33: case G2G_SIM33N: if (!p->a.pseq || !p->b.pseq) return G2G_ERR_ARG; break;
    default: return G2G_ERR_MODE;
    }
    if (!p->simmtx && (p->sim2_kind == G2G_SIM11 || p->sim2_kind / 10 == 12 || p->sim2_kind / 10 == 21 || p->sim2_kind / 10 == 22))
        return G2G_ERR_ARG;
    return G2G_OK;
}

// offsets (relative to arena base) are stored in the pointer fields first, rebased after allocation
template <class T> static inline T *OFF(size_t off) { return (T *) (uintptr_t) (off + 1); }   // +1: 0 stays NULL
template <class T> static inline void rebase(T *&p, char *base) { if (p) p = (T *) (base + ((uintptr_t) p - 1)); }

// An array that already lives in this context's HBM (g2g_side::dev, left there by g2g_device_derive) is not packed: the
// descriptor field gets the twin's address once the arena's offsets have been rebased (Patch list).
struct DevPatch { const void **field; const void *value; };
template <class T> static inline bool use_twin(std::vector<DevPatch> &patches, const T *&field, const T *twin)
{
    if (!twin) return false;
    field = 0;
    DevPatch p = {(const void **) &field, (const void *) twin};
    patches.push_back(p);
    return true;
}
static void pack_side(Blob &bl, const g2g_side &s, DevSide &d, int kind, bool need_gfq, std::vector<DevPatch> &patches)
{
    memset(&d, 0, sizeof d);
    const g2g_side_dev *tw = (s.dev && s.dev->ctx == bl.owner && !g2g_opt(bl.owner, "NO_RESIDENT_INPUTS")) ? s.dev : 0;
    d.many = s.many; d.len = s.len; d.left = s.left; d.right = s.right; d.nils = s.nils;
    d.nelm = s.nelm; d.felm = s.felm; d.sumwt = s.sumwt > 0 ? s.sumwt : (double) s.many;
    const size_t cols = (size_t) s.len + 2;
    if (!use_twin(patches, d.seq, tw ? tw->seq : 0)) d.seq = OFF<const uint8_t>(bl.put(s.seq, cols * s.many));
    if (s.weight && !use_twin(patches, d.weight, tw ? tw->weight : 0)) d.weight = OFF<const double>(bl.put(s.weight, sizeof(double) * s.many));
    if (s.pseq && s.nelm > 0 && !use_twin(patches, d.pseq, tw ? tw->pseq : 0)) d.pseq = OFF<const double>(bl.put(s.pseq, sizeof(double) * cols * s.nelm));
    if (!use_twin(patches, d.thk, tw ? tw->thk : 0)) d.thk = OFF<const double>(bl.put(s.thk, sizeof(double) * cols * 3));
    if (need_gfq) {
        d.hetero = s.gfq.hetero;
        {   // r = [head?] + (t with glen + 1): the structure Gfq::seq2gfq gives the r view (reference src/gfreq.cc:218-226)
            bool ok = true;
            const int32_t *to = s.gfq.off[1], *ro = s.gfq.off[2], *tg = s.gfq.glen[1], *rg = s.gfq.glen[2];
            const double *tf = s.gfq.freq[1], *rf = s.gfq.freq[2];
            for (int i = 1; i <= s.len && ok; ++i) {            // positions 0 .. len-1 (position -1 is the boundary's: only the chains read it)
                const int tl = to[i + 1] - to[i] - 1, rl = ro[i + 1] - ro[i] - 1;        // entries without the terminator
                if (tl < 0 || rl < 0) { ok = false; break; }
                const int h = (rl > 0 && rg[ro[i]] == 0) ? 1 : 0;
                if (rl != tl + h) { ok = false; break; }
                for (int k = 0; k < tl; ++k)
                    if (rg[ro[i] + h + k] != tg[to[i] + k] + 1 || rf[ro[i] + h + k] != tf[to[i] + k]) { ok = false; break; }
            }
            d.r_from_t = ok ? 1 : 0;
        }
        for (int v = 0; v < 3; ++v) {
            const int nlist = s.len + 2;                       // offsets for positions -1..len-1 + end
            const int pool = s.gfq.off[v][s.len + 1];
            for (int i = 0; i + 1 < nlist; ++i) d.maxlist = std::max(d.maxlist, s.gfq.off[v][i + 1] - s.gfq.off[v][i]);
            if (!use_twin(patches, d.off[v], tw ? (const int *) tw->off[v] : 0)) d.off[v] = OFF<const int>(bl.put(s.gfq.off[v], sizeof(int) * nlist));
            if (!use_twin(patches, d.glen[v], tw ? (const int *) tw->glen[v] : 0)) d.glen[v] = OFF<const int>(bl.put(s.gfq.glen[v], sizeof(int) * pool));
            if (!use_twin(patches, d.freq[v], tw ? tw->freq[v] : 0)) d.freq[v] = OFF<const double>(bl.put(s.gfq.freq[v], sizeof(double) * pool));
        }
    }
    if (kind == 3) {
        d.gapdens = OFF<const double>(bl.put(s.gapdens, sizeof(double) * cols * s.many));
        d.postgapdens = OFF<const double>(bl.put(s.postgapdens, sizeof(double) * cols * s.many));
    }
    if (s.npfq > 0 && s.pfq_pos && s.pfq_dns) {
        d.npfq = s.npfq; d.pfq_step = s.pfq_step;
        d.pfq_pos = OFF<const int>(bl.put(s.pfq_pos, sizeof(int) * (size_t) s.npfq));
        d.pfq_dns = OFF<const double>(bl.put(s.pfq_dns, sizeof(double) * (size_t) s.npfq));
    }
}

// The intron-position bonus of forwardB (reference src/fwd2c.h:367-370,378-379,446-452,472; PfqItr src/gsinfo.h:132-231) as a
// table of cells.  The reference walks two cursors: `api` over a's exon boundaries (it advances by one entry at the end of
// every row whose codon holds the current entry), and per such row `bpi` over b's, restarted at the row's first column and
// advanced by one entry at every column whose codon holds ITS current entry -- a cursor that has fallen behind the column
// (two boundaries in one codon) never catches up.  Both walks depend only on the inputs and the band, not on scores.
struct BonusCell { int m, n; double h, mx; };
static bool in_codon(int pos, int step, int col) { return step == 1 ? pos == col : ((long long) col * step <= pos && pos < (long long) col * step + step); }
static void intron_bonus_table(const g2g_problem *p, std::vector<BonusCell> &out)
{
    out.clear();
    const g2g_side &a = p->a, &b = p->b;
    if (p->spb_fact == 0 || a.npfq <= 0 || b.npfq <= 0 || !a.pfq_pos || !b.pfq_pos || !a.pfq_dns || !b.pfq_dns) return;
    const int sa = a.pfq_step, sb = b.pfq_step;
    int ka = 0;
    while (ka < a.npfq && a.pfq_pos[ka] < (long long) a.left * sa) ++ka;
    for (int m = a.left; m < a.right; ++m) {
        if (ka >= a.npfq) break;                                   // (the cursor only moves forward)
        if (!in_codon(a.pfq_pos[ka], sa, m)) continue;
        const int n0 = std::max(m + p->lw, b.left), n9 = std::min(m + p->up + 1, b.right);
        int kb = 0;
        while (kb < b.npfq && b.pfq_pos[kb] < (long long) n0 * sb) ++kb;
        for (int n = n0; n < n9 && kb < b.npfq; ++n) {
            if (!in_codon(b.pfq_pos[kb], sb, n)) continue;
            const int apos = a.pfq_pos[ka], bpos = b.pfq_pos[kb];
            BonusCell c;
            c.m = m; c.n = n;
            const bool phase = sa == 1 || (apos - bpos) % sa == 0;   // match_score: the two positions in the same codon phase
            c.h = phase ? p->spb_fact * a.pfq_dns[ka] * b.pfq_dns[kb] : 0;
            c.mx = (phase && (sa == 1 || apos % sa == 0)) ? p->spb_fact * a.pfq_dns[ka] * b.pfq_dns[kb] : 0;
            out.push_back(c);
            ++kb;
        }
        ++ka;
    }
}

extern "C" int g2g_bonus_cells(const g2g_problem *p, int cap, int32_t *m, int32_t *n, double *h, double *mx)
{
    if (!p || cap < 0) { g2g_set_error("g2g_bonus_cells: %s", "bad argument"); return G2G_ERR_ARG; }
    std::vector<BonusCell> bc;
    if (!is_rect(p->alnmode)) intron_bonus_table(p, bc);
    for (size_t k = 0; k < bc.size() && k < (size_t) cap; ++k) {
        if (m) m[k] = bc[k].m;
        if (n) n[k] = bc[k].n;
        if (h) h[k] = bc[k].h;
        if (mx) mx[k] = bc[k].mx;
    }
    return (int) bc.size();
}

static void rebase_side(DevSide &d, char *base)
{
    rebase(d.seq, base); rebase(d.weight, base); rebase(d.pseq, base); rebase(d.thk, base);
    for (int v = 0; v < 3; ++v) { rebase(d.off[v], base); rebase(d.glen[v], base); rebase(d.freq[v], base); }
    rebase(d.gapdens, base); rebase(d.postgapdens, base);
    rebase(d.pfq_pos, base); rebase(d.pfq_dns, base);
}

// a batch gives its arena back to the context's pool
static void release_arena(g2g_batch *b)
{
    if (!b->d_arena) return;
    pool_give(b->ctx, b->d_arena, b->arena_cap);
    b->d_arena = 0;
}

// ---- g2g_batch_prepare: its steps ------------------------------------------------------------------------------------------
// What is decided -- the shape of the batch, the kernel of each DP, the queues -- is decided in g2g_plan.h from plain values
// (PrepOptions, DpFacts); the functions here pack, carve the arena, allocate and upload.
static_assert(G2G_PLAN_V2_TILE_COLS == G2G_V2_TILE_COLS, "g2g_plan.h and the build flags disagree about the widest v2 tile");
static PrepOptions prep_options(const g2g_ctx *c)
{
    PrepOptions o = prep_defaults(c->ncu);
    auto on = [&](const char *name) { return g2g_opt(c, name) != 0; };
    auto num = [&](const char *name, int unset) { const char *e = g2g_opt(c, name); return e ? atoi(e) : unset; };
    o.force_v1 = on("FORCE_V1"); o.no_v7 = on("NO_V7"); o.no_v8 = on("NO_V8"); o.force_v2 = on("FORCE_V2"); o.no_v6 = on("NO_V6");
    o.no_areg = on("NO_AREG"); o.no_strip_bonus = on("NO_STRIP_BONUS"); o.no_chainq = on("NO_CHAINQ"); o.no_simblk = on("NO_SIMBLK");
    o.v6_small = num("V6_SMALL_KB", 40) * 1024; o.v6_large = num("V6_LARGE_KB", 0) * 1024;
    o.v2_threads = num("V2_THREADS", 0); o.v2_cols = num("V2_COLS", 0); o.v3_cols = num("V3_COLS", 0);
    if (const char *e = g2g_opt(c, "V6_MIN_STRIPS")) { o.min_strips_set = true; o.min_strips = atoll(e); }
    o.v3_sweep = num("V3_SWEEP", 1); o.v2_sweep = num("V2_SWEEP", 1);
    if (const char *e = g2g_opt(c, "INJECT_STALL")) { o.inject = true; o.inject_victim = atoi(e); }
    return o;
}

// (new g2g_batch() zero-initialises every plain member: counters, device pointers, pool capacities, offsets)
static g2g_batch *new_batch(g2g_ctx *ctx, int n, const g2g_problem *const *prob, bool force_v1, const PrepOptions &o)
{
    g2g_batch *b = new g2g_batch();
    b->ctx = ctx; b->n = n; b->force_v1 = force_v1; b->injected = o.inject;
    b->src.assign(prob, prob + n);
    b->recovered.assign(n, g2g_result()); b->was_recovered.assign(n, 0); b->ib.assign(n, 0); b->path_rec.assign(n, 0);
    b->dp.resize(n); b->status.assign(n, G2G_OK); b->cells.assign(n, 0); b->out_off.assign(n, 0); b->tcap.assign(n, 0); b->rr1.assign(n, 0);
    b->v2_maxrows = b->v2_maxcols = 1;
    return b;
}

// size the staging buffer once (growing a pinned buffer means allocating and copying it again)
static size_t staging_estimate(const g2g_ctx *ctx, int n, const g2g_problem *const *prob)
{
    auto side_bytes = [&](const g2g_side &s) {
        const size_t cols = (size_t) s.len + 2;
        const g2g_side_dev *tw = (s.dev && s.dev->ctx == ctx) ? s.dev : 0;
        size_t t = 8 * (size_t) s.many + 24 * cols + 256;
        if (!(tw && tw->seq)) t += cols * s.many;
        if (s.pseq && s.nelm > 0 && !(tw && tw->pseq)) t += 8 * cols * s.nelm;
        if (s.has_gfq) for (int v = 0; v < 3; ++v) if (s.gfq.off[v] && !(tw && tw->freq[v])) t += 4 * cols + 12 * (size_t) s.gfq.off[v][s.len + 1] + 64;
        if (s.gapdens) t += 16 * cols * s.many;
        return t;
    };
    size_t est = (sizeof(DevProb) + 8) * (size_t) (n > 0 ? n : 1) + 4096;
    for (int i = 0; i < n; ++i) {
        const g2g_problem *p = prob[i];
        if (check_problem(p) != G2G_OK) continue;
        est += side_bytes(p->a) + side_bytes(p->b) + 8 * (size_t) (p->simmtx ? p->simdim * p->simrows : 0) + 64;
    }
    return est;
}

// the intron-position bonus table of a DP, with the strip kernels' per-row index behind bon_m's entries
static void pack_bonus(Blob &bl, const g2g_problem *p, DevProb &d)
{
    std::vector<BonusCell> bc;
    intron_bonus_table(p, bc);
    if (bc.empty()) return;
    std::vector<int> bm, bn; std::vector<double> bh, bx;
    for (const BonusCell &c : bc) { bm.push_back(c.m); bn.push_back(c.n); bh.push_back(c.h); bx.push_back(c.mx); }
    d.nbonus = (int) bc.size();
    // first entry of row a.left + r, r = 0 .. rows (the table is row-major with n ascending within a row; g2g_forward_kernel
    // reads the first nbonus entries only)
    const int rows = p->a.right - p->a.left;
    size_t k = 0;
    for (int r = 0; r <= rows; ++r) {
        while (k < bc.size() && bc[k].m < p->a.left + r) ++k;
        bm.push_back((int) k);
    }
    // (put_now: the four vectors are gone by the time flush() makes put()'s deferred copies)
    d.bon_m = OFF<const int>(bl.put_now(bm.data(), sizeof(int) * bm.size()));
    d.bon_n = OFF<const int>(bl.put_now(bn.data(), sizeof(int) * bn.size()));
    d.bon_h = OFF<const double>(bl.put_now(bh.data(), sizeof(double) * bh.size()));
    d.bon_mx = OFF<const double>(bl.put_now(bx.data(), sizeof(double) * bx.size()));
}

// 1. check a problem and pack its inputs into the host image; returns its status (d.kind -1: not run)
static int pack_problem(Blob &bl, const g2g_problem *p, DevProb &d, std::vector<DevPatch> &patches)
{
    memset(&d, 0, sizeof d);
    const int rc = check_problem(p);
    if (rc) { d.kind = -1; return rc; }
    d.kind = kind_of(p->alnmode);
    d.noll = p->noll; d.sim2_kind = p->sim2_kind; d.crg2_kind = p->crg2_kind; d.codonk1 = p->codonk1;
    d.rect = is_rect(p->alnmode) ? 1 : 0;
    d.lw = p->lw; d.up = p->up;
    if (d.rect) { d.lw = p->b.left - p->a.right; d.up = p->b.right - p->a.left; }     // every cell and every boundary corner inside
    d.width = d.up - d.lw + 3;
    d.basic_gop = p->basic_gop; d.weighted_gop = p->weighted_gop; d.u = p->u;
    d.u2divu1 = p->u2divu1; d.v2divv1 = p->v2divv1;
    d.simdim = p->simdim;
    if (p->simmtx) d.simmtx = OFF<const double>(bl.put(p->simmtx, sizeof(double) * (size_t) p->simdim * p->simrows));
    pack_side(bl, p->a, d.a, d.kind, d.kind == 1 || d.kind == 2, patches);
    pack_side(bl, p->b, d.b, d.kind, d.kind == 2, patches);
    d.spb_fact = p->spb_fact; d.dvsp = p->dvsp;
    pack_bonus(bl, p, d);
    return G2G_OK;
}

// 2. what the decisions need of a packed DP (and the capacity of its dynamic lists, which is one of those things)
static DpFacts dp_facts(DevProb &d, const g2g_problem *p)
{
    DpFacts f;
    memset(&f, 0, sizeof f);
    f.kind = d.kind;
    if (d.kind < 0) return f;
    if (d.kind == 1) { d.capa = p->a.gfq.hetero + 1; d.capb = 0; }
    else if (d.kind == 2) { d.capa = p->a.gfq.hetero + 1; d.capb = p->b.gfq.hetero + 1; }
    else if (d.kind == 3) { d.capa = p->a.many; d.capb = p->b.many; }
    f.rect = d.rect; f.noll = d.noll; f.capa = d.capa; f.capb = d.capb; f.nbonus = d.nbonus;
    f.crg2_kind = d.crg2_kind; f.sim2_kind = d.sim2_kind; f.lw = d.lw; f.up = d.up;
    auto side = [](const g2g_side &s, const DevSide &ds) {
        SideFacts x = {s.len, s.many, s.left, s.right, ds.nelm, ds.felm, ds.maxlist, ds.r_from_t, s.gapdens != 0, s.postgapdens != 0, s.weight != 0, {0, 0, 0}};
        if (s.has_gfq) for (int v = 0; v < 3; ++v) x.off[v] = s.gfq.off[v];
        return x;
    };
    f.a = side(p->a, d.a); f.b = side(p->b, d.b);
    return f;
}

// 5. the device-only part of the arena: state, trace, then the outputs of all problems in ONE contiguous region (a single
// device-to-host copy fetches a whole sweep).  Offsets go into the pointer fields (OFF) and are rebased after allocation.
struct Arena {
    size_t off;
    size_t take(size_t bytes) { const size_t o = off; off = (off + bytes + 15) & ~(size_t) 15; return o; }
};
static void layout_v1_state(Arena &A, DevProb &d)      // the diagonal-indexed row buffers of g2g_forward_kernel (v1): only for DPs it runs
{
    const size_t W = d.width;
    for (int x = 0; x < NX; ++x) {
        if (d.noll != 3 && (x == XG2 || x == XF2)) continue;
        d.val[x] = OFF<double>(A.take(sizeof(double) * W));
        d.dir[x] = OFF<uint8_t>(A.take(W));
        if (d.kind == 1 || d.kind == 2) d.dla[x] = OFF<int2>(A.take(sizeof(int2) * W * d.capa));
        if (d.kind == 2) d.dlb[x] = OFF<int2>(A.take(sizeof(int2) * W * d.capb));
        if (d.kind == 1) d.glb[x] = OFF<int>(A.take(sizeof(int) * W));
        if (d.kind == 3) d.glb[x] = OFF<int>(A.take(sizeof(int) * W * (d.capa + d.capb)));
    }
    d.spw = (int) W;
}
// boundary records of a DP on strips; returns whether its kernel reads a column-score matrix (strips in sweep mode make their
// own scores, block by block)
static bool layout_strip_state(Arena &A, DevProb &d, int blen, const BatchShape &s, const PrepOptions &o)
{
    const size_t rows = (size_t) (d.a.right - d.a.left);
    d.spw = 1;                                  // g2g_spscore_kernel keeps its two dynamic lists in dla/dlb[XH] (stride spw)
    d.dla[XH] = OFF<int2>(A.take(sizeof(int2) * (size_t) (d.capa + 1)));
    if (d.kind == 2) d.dlb[XH] = OFF<int2>(A.take(sizeof(int2) * (size_t) (d.capb + 1)));
    const size_t recsz = strip_record_bytes(d.v2_ok, d.kind, d.capa, d.capb);
    d.v2_rowstride = blen + 3;
    d.v2_rowH = OFF<void>(A.take(3 * recsz * (size_t) d.v2_rowstride));
    d.v2_rowG = OFF<void>(A.take(3 * recsz * (size_t) d.v2_rowstride));
    if (d.noll == 3) d.v2_rowG2 = OFF<void>(A.take(3 * recsz * (size_t) d.v2_rowstride));
    d.v2_colH = OFF<void>(A.take(recsz * (rows + 3)));
    d.v2_cbH = OFF<void>(A.take(recsz * (rows + 3)));
    d.v2_cbF = OFF<void>(A.take(recsz * (rows + 3)));
    if (d.noll == 3) d.v2_cbF2 = OFF<void>(A.take(recsz * (rows + 3)));
    d.v2_rowoff = OFF<long long>(A.take(sizeof(long long) * (rows + 2)));
    const bool own_sim = !o.no_simblk && (d.v2_ok >= 6 || (d.v2_ok == 1 && s.v2_sweep) || ((d.v2_ok == 2 || d.v2_ok == 3) && d.kind == 1 && s.v3_sweep));
    if (!own_sim) d.v2_sim = OFF<double>(A.take(sizeof(double) * (size_t) d.cells + 64));
    return !own_sim;
}
static void layout_arena(g2g_batch *b, const BatchShape &s, const PrepOptions &o)
{
    Arena A = {b->in_bytes};
    for (int i = 0; i < b->n; ++i) {
        DevProb &d = b->dp[i];
        if (d.kind < 0) continue;
        const int al = d.a.left, ar = d.a.right, bl = d.b.left, br = d.b.right;
        const BandCells bc = band_cells(al, ar, bl, br, d.lw, d.up);
        d.d0 = al + bl; d.d1 = (ar - 1) + (br - 1);
        b->cells[i] = d.cells = bc.cells;
        d.tstride = bc.tstride;
        d.trace = OFF<uint8_t>(A.take((size_t) (d.d1 - d.d0 + 1) * d.tstride));
        if (!d.v2_ok) layout_v1_state(A, d);
        else if (layout_strip_state(A, d, b->src[i]->b.len, s, o)) ++b->nsimmat;
        b->rr1[i] = (long long) (bl - al) + (br - ar);
        b->tcap[i] = d.tcap = (ar - al) + (br - bl) + 4;
    }
    b->out_lo = A.off;
    for (int i = 0; i < b->n; ++i) {
        DevProb &d = b->dp[i];
        if (d.kind < 0) continue;
        b->out_off[i] = A.take(sizeof(double) + sizeof(int) * 2 + sizeof(int2) * (size_t) d.tcap);
        d.score = OFF<double>(b->out_off[i]);
        d.ntrace = OFF<int>(b->out_off[i] + sizeof(double));
        d.otrace = OFF<int2>(b->out_off[i] + sizeof(double) + 2 * sizeof(int));
    }
    b->out_hi = A.off;
    b->arena_bytes = A.off + 256;
}

// 6. the offsets of a descriptor become addresses
static void rebase_problem(DevProb &d, char *base)
{
    rebase(d.simmtx, base);
    rebase(d.bon_m, base); rebase(d.bon_n, base); rebase(d.bon_h, base); rebase(d.bon_mx, base);
    rebase_side(d.a, base); rebase_side(d.b, base);
    for (int x = 0; x < NX; ++x) { rebase(d.val[x], base); rebase(d.dir[x], base); rebase(d.dla[x], base); rebase(d.dlb[x], base); rebase(d.glb[x], base); }
    rebase(d.v2_rowH, base); rebase(d.v2_rowG, base); rebase(d.v2_rowG2, base); rebase(d.v2_colH, base);
    rebase(d.v2_cbH, base); rebase(d.v2_cbF, base); rebase(d.v2_cbF2, base);
    rebase(d.v2_rowoff, base); rebase(d.v2_sim, base);
    rebase(d.trace, base); rebase(d.score, base); rebase(d.ntrace, base); rebase(d.otrace, base);
}

// 7. index lists of the DPs on g2g_forward_kernel (i1) and on strips (i2), and the dynamic LDS of the v2 launch
static void fill_index_lists(g2g_batch *b, int *i1, int *i2)
{
    b->n1 = b->n2 = 0; b->lds2 = 0;
    for (int i = 0; i < b->n; ++i) {
        const DevProb &d = b->dp[i];
        if (d.kind < 0) continue;
        if (d.v2_ok) { i2[b->n2++] = i; if (d.v2_ok == 1) b->lds2 = std::max(b->lds2, v2_lds_bytes(d.kind, d.noll, d.capa, d.capb, d.a.maxlist, d.b.maxlist, b->v2_threads)); }
        else i1[b->n1++] = i;
    }
}

// 8. a queue plan becomes the batch's: two pool blocks (tiles + prologue list, flags), three copies, and option V6_RING_PLAN,
// which reads back what the v6 launches of the batch were given (g2g_get_option)
// (g2g_batch_free has taken the batch when this fails)
static int upload_queues(g2g_ctx *ctx, g2g_batch *b, const QueuePlan &Q)
{
    if (Q.bad >= 0) { g2g_set_error("%s", "g2g_batch_prepare: a DP was given a kernel that has no variant slot"); g2g_batch_free(b); return G2G_ERR_DEVICE; }
    memcpy(b->var_off, Q.var_off, sizeof b->var_off); memcpy(b->var_cells, Q.var_cells, sizeof b->var_cells);
    memcpy(b->v3lds, Q.v3lds, sizeof b->v3lds); memcpy(b->v6lds, Q.v6lds, sizeof b->v6lds);
    b->lds2p = Q.lds2p; b->simtile_lds = Q.simtile_lds; b->v2_maxrows = Q.v2_maxrows; b->v2_maxcols = Q.v2_maxcols;
    b->fail_off = Q.fail_off; b->dump_off = Q.dump_off; b->xq_off = Q.xq_off;
    b->ntiles = (long long) Q.tiles.size(); b->nflags = (int) Q.flags.size(); b->flags0 = Q.flags; b->np = 0;
    ctx->opt["V6_RING_PLAN"] = std::make_pair(true, Q.v6_ring_plan);
    if (Q.tiles.empty()) return G2G_OK;
    const std::vector<V2Tile> &all = Q.tiles;
    hipError_t e2 = hipSuccess;
    b->d_tiles = (V2Tile *) pool_take(ctx, sizeof(V2Tile) * all.size() + sizeof(int) * (Q.ip.size() + 1), &b->tiles_cap);
    if (!b->d_tiles) e2 = hipErrorOutOfMemory;
    if (e2 == hipSuccess) e2 = hipMemcpy(b->d_tiles, all.data(), sizeof(V2Tile) * all.size(), hipMemcpyHostToDevice);
    b->d_idxp = (int *) (b->d_tiles + all.size()); b->np = (int) Q.ip.size();
    if (e2 == hipSuccess && b->np) e2 = hipMemcpy(b->d_idxp, Q.ip.data(), sizeof(int) * Q.ip.size(), hipMemcpyHostToDevice);
    if (e2 == hipSuccess) { b->d_flags = (int *) pool_take(ctx, sizeof(int) * Q.flags.size(), &b->flags_cap); if (!b->d_flags) e2 = hipErrorOutOfMemory; }
    if (e2 == hipSuccess) e2 = hipMemcpy(b->d_flags, Q.flags.data(), sizeof(int) * Q.flags.size(), hipMemcpyHostToDevice);
    if (e2 != hipSuccess) { g2g_set_error("tiles: %s", hipGetErrorString(e2)); (void) hipGetLastError(); g2g_batch_free(b); return G2G_ERR_NOMEM; }
    return G2G_OK;
}

static int batch_prepare_impl(g2g_ctx *ctx, int n, const g2g_problem *const *prob, g2g_batch **out, bool force_v1);
extern "C" int g2g_batch_prepare(g2g_ctx *ctx, int n, const g2g_problem *const *prob, g2g_batch **out)
{
    return batch_prepare_impl(ctx, n, prob, out, false);
}
static int batch_prepare_impl(g2g_ctx *ctx, int n, const g2g_problem *const *prob, g2g_batch **out, bool force_v1)
{
    if (!ctx || n < 0 || !out) return G2G_ERR_ARG;
    if (n > G2G_MAX_BATCH) { g2g_set_error("%s", "g2g_batch_prepare: more than 32768 problems in one batch (use g2g_forward_batch, which cuts chunks)"); return G2G_ERR_ARG; }
    if (!ctx->ok) return G2G_ERR_NODEVICE;
    HIPCHK(hipSetDevice(ctx->device));
    const bool prep_dbg = g2g_opt(ctx, "DEBUG_PREP") != 0;
    auto prep_t0 = std::chrono::steady_clock::now();
    auto prep_lap = [&](const char *what) {
        if (!prep_dbg) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[g2g prepare] %-28s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(t - prep_t0).count());
        prep_t0 = t;
    };
    const PrepOptions opts = prep_options(ctx);
    g2g_batch *b = new_batch(ctx, n, prob, force_v1, opts);
    const size_t n1 = (size_t) (n > 0 ? n : 1);
    Blob bl(ctx);
    if (const char *e = g2g_opt(ctx, "PACK_THREADS")) bl.pack_threads = atoi(e);
    bl.grow(staging_estimate(ctx, n, prob));
    const size_t probs_off = bl.put(0, 0);
    bl.extend(probs_off + sizeof(DevProb) * n1);
    std::vector<DevPatch> patches;            // descriptor fields that point at device-resident inputs (b->dp is never resized)
    std::vector<DpFacts> facts(n);
    for (int i = 0; i < n; ++i) {
        b->status[i] = pack_problem(bl, prob[i], b->dp[i], patches);
        facts[i] = dp_facts(b->dp[i], prob[i]);
    }
    const BatchShape shape = batch_shape(facts.data(), n, opts);
    b->v3_cols = shape.v3_cols; b->v2_threads = shape.v2_threads; b->v2_cols = shape.v2_cols; b->v6_on = shape.v6_on;
    b->v3_sweep = shape.v3_sweep; b->v2_sweep = shape.v2_sweep;
    std::vector<KernelChoice> choice(n);
    for (int i = 0; i < n; ++i) {
        if (b->dp[i].kind < 0) { const KernelChoice none = {0, 0, 0, {{0, 0, 0}, 0, {0, 0, 0}}}; choice[i] = none; continue; }
        choice[i] = choose_kernel(facts[i], shape, opts, force_v1);
        b->dp[i].v2_ok = choice[i].generation; b->ib[i] = choice[i].ib;
    }
    // index lists for the two forward kernels (filled below, once the arena has its address)
    const size_t idx_off = bl.put(0, 0);
    bl.extend(idx_off + sizeof(int) * 2 * n1);
    b->in_bytes = (bl.size() + 255) & ~(size_t) 255;
    layout_arena(b, shape, opts);
    bl.flush();
    if (bl.oom) { g2g_set_error("%s", "host staging buffer: out of (pinned) memory"); delete b; return G2G_ERR_NOMEM; }
    prep_lap("host image of the inputs");
    b->d_arena = (char *) pool_take(ctx, b->arena_bytes, &b->arena_cap);
    prep_lap("hipMalloc(arena)");
    if (!b->d_arena) {
        g2g_set_error("hipMalloc(arena): %s", hipGetErrorString(hipErrorOutOfMemory));
        (void) hipGetLastError();              // a failed allocation must not poison the next launch check of this thread
        delete b; return G2G_ERR_NOMEM;
    }
    for (int i = 0; i < n; ++i) if (b->dp[i].kind >= 0) rebase_problem(b->dp[i], b->d_arena);
    for (const DevPatch &pt : patches) *pt.field = pt.value;
    fill_index_lists(b, (int *) (bl.data() + idx_off), (int *) (bl.data() + idx_off) + n1);
    b->d_idx1 = (int *) (b->d_arena + idx_off);
    b->d_idx2 = b->d_idx1 + n1;
    if (int rc = upload_queues(ctx, b, queue_plan(facts.data(), choice.data(), b->cells.data(), shape, opts, n))) return rc;
    prep_lap("descriptors, tiles, flags");
    if (n) memcpy(bl.data() + probs_off, b->dp.data(), sizeof(DevProb) * (size_t) n);
    b->d_probs = (DevProb *) (b->d_arena + probs_off);
    hipError_t e = hipMemcpyAsync(b->d_arena, bl.data(), bl.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { g2g_set_error("upload: %s", hipGetErrorString(e)); g2g_batch_free(b); return G2G_ERR_DEVICE; }
    prep_lap("upload");
    *out = b;
    return G2G_OK;
}


// ---- CU shares ---------------------------------------------------------------------------------------------------
// The persistent launches of a sweep used to share every CU: whichever workgroup the dispatcher picked next took the LDS
// and the wave slots that had just become free, so strips of up to four kernels sat side by side on a CU.  A run that
// fills the machine now gives each launch a SHARE of the CUs of its own (hipExtStreamCreateWithCUMask): the chip is cut
// into 32 units -- unit u = CU slot u of every XCD, which is how the mask bits map on this part (bit i -> XCD i % 8,
// CU slot i / 8: tools/probes/cumask_probe.hip) -- and a launch gets a contiguous range of units in proportion to its
// estimated work, capped by what its strips can occupy.  No CU ever holds workgroups of two launches, every launch
// still spreads over all eight XCDs (L2s), and a grid is sized for ITS CUs.  Small runs (a refinement window) keep the
// whole chip for every launch: there a DP's critical path is what counts.
static size_t mstream_cap(const g2g_ctx *c)
{
    size_t cap = 8;
    if (const char *e = g2g_opt(c, "MSTREAM_MAX")) { const int v = atoi(e); if (v >= 2 && v <= 64) cap = (size_t) v; }
    return cap;
}
static hipStream_t cu_share_stream(g2g_ctx *c, int lo, int n)
{
    for (auto &m : c->mstream) if (m.lo == lo && m.n == n) { m.used = ++c->mstamp; return m.s; }
    // Every share is a hardware queue of its own, on top of the launch streams' (GPU_MAX_HW_QUEUES).  Somewhere above twenty queues the
    // hardware scheduler starts to take queues off the machine in turn -- persistent launches then stand still for tens to hundreds of
    // ms at a time (seen as gaps by the waiting waves: g2g_ctx_wait_gaps) -- so the shares in use are kept few.
    const size_t cap = mstream_cap(c);
    if (c->mstream.size() >= cap) {                         // forget the least recently used share
        size_t k = 0;
        for (size_t i = 1; i < c->mstream.size(); ++i) if (c->mstream[i].used < c->mstream[k].used) k = i;
        hipStreamSynchronize(c->mstream[k].s); hipStreamDestroy(c->mstream[k].s);
        c->mstream.erase(c->mstream.begin() + k);
    }
    uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int bit = 8 * lo; bit < 8 * (lo + n) && bit < 256; ++bit) mask[bit >> 5] |= 1u << (bit & 31);
    g2g_ctx::MStream m; m.lo = lo; m.n = n; m.s = 0; m.used = ++c->mstamp;
    if (hipExtStreamCreateWithCUMask(&m.s, 8, mask) != hipSuccess || !m.s) { (void) hipGetLastError(); return 0; }
    c->mstream.push_back(m);
    ++c->n_mstreams;
    return m.s;
}
static int batch_path(const g2g_batch *b, int i)
{
    if (b->status[i]) return 0;
    if (b->was_recovered[i]) return b->path_rec[i];
    return family_path(b->dp[i].v2_ok);
}

// ---- a run: plan (g2g_plan.h), then execute ------------------------------------------------------------------------
// the typed kernel of every variant slot (four signatures: the family says which member is set)
typedef void (*v2k_t)(const DevProb *, const V2Tile *, int, int *, int *, int, int, int, int, int, double *);
typedef void (*v3k_t)(const DevProb *, const V2Tile *, int, int *, int *, int, V3Lds, int, int, int, double *);
typedef void (*v6k_t)(const DevProb *, const V2Tile *, int, int *, int *, int, V6Lds, int, int, double *, unsigned *, int);
typedef void (*v7k_t)(const DevProb *, const V2Tile *, int, int *, int *, int, int, double *);
struct VariantKernel { v2k_t v2; v3k_t v3; v6k_t v6; v7k_t v7; };
#define K2(f) {f, 0, 0, 0}
#define K3(f) {0, f, 0, 0}
#define K6(f) {0, 0, f, 0}
#define K7(f) {0, 0, 0, f}
static const VariantKernel G2G_KERNEL[G2G_NVAR] = {
    K2(g2g_v2_hf2), K2(g2g_v2_hf3), K2(g2g_v2_pf2), K2(g2g_v2_pf3), K3(g2g_v3_hf2), K3(g2g_v3_hf3), K2(0), K2(0),
    K3(g2g_v3r_hf2), K3(g2g_v3r_hf3), K2(0), K2(0), K6(g2g_v6_pf2), K6(g2g_v6_pf3), K6(g2g_v6_pf2), K6(g2g_v6_pf3),
    K7(g2g_v7_ngp2), K7(g2g_v7_ngp3), K7(g2g_v8_ntv2), K7(g2g_v8_ntv3), K6(g2g_v6_pf2), K6(g2g_v6_pf3), K2(0), K2(0),
    K7(g2g_v7_ngp2_ib), K7(g2g_v7_ngp3_ib), K2(g2g_v2_hf2_ib), K2(g2g_v2_hf3_ib), K2(g2g_v2_pf2_ib), K2(g2g_v2_pf3_ib), K7(g2g_v8_ntv2_ib), K7(g2g_v8_ntv3_ib),
};
#undef K2
#undef K3
#undef K6
#undef K7

static RunFacts run_facts(const g2g_ctx *ctx, const g2g_batch *b)
{
    RunFacts f;
    for (int v = 0; v < G2G_NVAR; ++v) { f.cnt[v] = b->var_off[v + 1] - b->var_off[v]; f.cells[v] = b->var_cells[v]; }
    f.ncu = ctx->ncu;
    f.lds2 = b->lds2; f.lds2p = b->lds2p;
    f.v2_threads = b->v2_threads; f.v2_sweep = b->v2_sweep; f.v3_sweep = b->v3_sweep; f.v2_cols = b->v2_cols; f.v3_cols = b->v3_cols;
    for (int k = 0; k < 8; ++k) { const V3Lds &L = b->v3lds[k]; const LdsFacts x = {L.total, L.svals, L.rows, L.black}; f.v3[k] = x; }
    for (int k = 0; k < 6; ++k) { const V6Lds &L = b->v6lds[k]; const LdsFacts x = {L.total, L.svals, L.rows, L.black}; f.v6[k] = x; }
    auto wpc_opt = [&](const char *name) { const char *e = g2g_opt(ctx, name); const int w = e ? atoi(e) : 0; return (w >= 1 && w <= 32) ? w : 0; };
    f.v2_wpc = wpc_opt("V2_WPC"); f.v3_wpc = wpc_opt("V3_WPC"); f.v6_wpc = wpc_opt("V6_WPC");
    const char *only = g2g_opt(ctx, "ONLY_VAR");
    f.only_var_set = only != 0; f.only_var = only ? atoi(only) : 0;
    f.no_simblk = g2g_opt(ctx, "NO_SIMBLK") != 0; f.no_prostage = g2g_opt(ctx, "NO_PROSTAGE") != 0; f.parallel_hf = g2g_opt(ctx, "PARALLEL_HF") != 0;
    f.pro_lds_bytes = PRO_LDS_BYTES;
    f.simblk_bytes = (size_t) G2G_SIMBLK_STRIDE * sizeof(double);
    return f;
}

// Tile-mode DPs (test configurations; sweep mode, the default, needs none of this) read a column-score matrix and take
// their boundary chains from a prologue kernel: row offsets first (tiny), then the chains (single-lane, latency-bound) on
// a side stream while the score kernels (fully parallel) fill the GPU on the main one
static int run_tile_prologue(g2g_ctx *ctx, g2g_batch *b, int pro_off)
{
    if (b->nsimmat || b->np) {
        if (b->nsimmat) {
            hipLaunchKernelGGL(g2g_v2_rowoff_kernel, dim3((b->n2 + 63) / 64), dim3(64), 0, ctx->stream,
                               (const DevProb *) b->d_probs, (const int *) b->d_idx2, b->n2);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(ctx->vev[G2G_NVS], ctx->stream));
        HIPCHK(hipStreamWaitEvent(ctx->vstream[G2G_NVS - 1], ctx->vev[G2G_NVS], 0));
        if (b->np) {
            hipLaunchKernelGGL(g2g_v2_prologue_kernel, dim3(b->np), dim3(128), pro_off ? pro_off + 2 * PRO_LDS_BYTES : b->lds2p, ctx->vstream[G2G_NVS - 1],
                               (const DevProb *) b->d_probs, (const int *) b->d_idxp, pro_off);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(ctx->vev[G2G_NVS - 1], ctx->vstream[G2G_NVS - 1]));
        if (b->nsimmat) {
            const int simtiled = (!g2g_opt(ctx, "NO_SIMTILE") && b->simtile_lds && b->simtile_lds <= 64 * 1024) ? 1 : 0;
            if (simtiled) {
                hipLaunchKernelGGL(g2g_v2_sim_tile_kernel, dim3((b->v2_maxcols + SIM_TC - 1) / SIM_TC, (b->v2_maxrows + SIM_TR - 1) / SIM_TR, b->n2), dim3(256),
                                   b->simtile_lds, ctx->stream, (const DevProb *) b->d_probs, (const int *) b->d_idx2);
                HIPCHK(hipGetLastError());
            }
            hipLaunchKernelGGL(g2g_v2_sim_kernel, dim3(b->v2_maxrows, b->n2), dim3(256), 0, ctx->stream,
                               (const DevProb *) b->d_probs, (const int *) b->d_idx2, simtiled);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->vev[G2G_NVS - 1], 0));
    }
    if (g2g_opt(ctx, "DEBUG")) { hipError_t e3 = hipStreamSynchronize(ctx->stream); fprintf(stderr, "[g2g] prologue+sim done: %s\n", hipGetErrorString(e3)); fflush(stderr); }
    return G2G_OK;
}

// The next generation of the progress counters, the queue heads, and the header of the waits (g2g_wait_ge): time-outs, first
// slot, offset of the fail flags, wall-clock limit; then the fork event every persistent launch waits for.
static int write_wait_header(g2g_ctx *ctx, g2g_batch *b)
{
    ++b->gen;
    if ((b->gen & 0x7FF) == 0 && b->d_flags) {             // sweep-mode progress counters carry gen & 0x7FF: start over
        HIPCHK(hipMemcpyAsync(b->d_flags, b->flags0.data(), sizeof(int) * b->flags0.size(), hipMemcpyHostToDevice, ctx->stream));
        ++b->gen;
    }
    // (the image lives in the batch: an asynchronous copy from pageable memory may read its source after the call returns)
    int *hdr = b->hdr_img;
    memset(hdr, 0, sizeof b->hdr_img);
    // a legitimate wait lasts as long as the strip above needs for one publish interval, or a boundary chain for its
    // sequential walk: milliseconds, tens of ms for a strip pulled long before its producer gets going (under 180 ms in every
    // ordinary sweep observed).  Half a second of wall clock means the producer is not running; a false alarm only costs a re-run.
    double limit_ms = 500.;
    if (const char *e = g2g_opt(ctx, "WAIT_LIMIT_MS")) { const double v = atof(e); if (v > 0) limit_ms = v; }
    hdr[G2G_HDR + 2] = b->fail_off;
    hdr[G2G_HDR + 82] = b->dump_off;
    hdr[G2G_HDR + 3] = (int) std::min(2.0e9, limit_ms * ctx->rt_ticks_per_ms / 65536.) + 1;
    HIPCHK(hipMemcpyAsync(b->d_flags, hdr, sizeof b->hdr_img, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(b->d_flags + b->fail_off, 0, sizeof(int) * (size_t) (b->n > 0 ? b->n : 1), ctx->stream));
    HIPCHK(hipMemsetAsync(b->d_flags + b->xq_off, 0, sizeof(int) * (G2G_NVAR - G2G_HDR), ctx->stream));
    HIPCHK(hipEventRecord(ctx->vev[G2G_NVS], ctx->stream));
    return G2G_OK;
}

// CU shares of this run's persistent launches: the plan, then the stream of every share (looked up or created here, once: a
// launch never creates or evicts a queue while others are resident).  A stream that cannot be had turns the shares off.
static void resolve_shares(g2g_ctx *ctx, const RunFacts &f, ShareOut &sh, hipStream_t sh_stream[G2G_NVAR])
{
    ShareIn in;
    for (int v = 0; v < G2G_NVAR; ++v) { in.cnt[v] = f.cnt[v]; in.cells[v] = f.cells[v]; in.wpc[v] = f.cnt[v] ? share_wpc(f, v) : 1; sh_stream[v] = 0; }
    in.ncu = f.ncu;
    const char *opt = g2g_opt(ctx, "CU_SHARES");
    in.mode_set = opt != 0; in.mode = opt ? atoi(opt) : 0;
    in.debug = g2g_opt(ctx, "DEBUG") != 0; in.no_share_gap = g2g_opt(ctx, "NO_SHARE_GAP") != 0;
    in.mstream_cap = mstream_cap(ctx);
    for (const auto &m : ctx->mstream) in.alive.push_back(std::make_pair(m.lo, m.n));
    cu_share_plan(in, sh);
    if (sh.shares)
        for (int v = 0; v < G2G_NVAR; ++v) if (sh.n[v]) { sh_stream[v] = cu_share_stream(ctx, sh.lo[v], sh.n[v]); if (!sh_stream[v]) sh.shares = false; }
    if (g2g_opt(ctx, "WARN") && sh.shares) {
        fprintf(stderr, "[g2g] CU shares (units of 8 CUs, one per XCD):");
        for (int v = 0; v < G2G_NVAR; ++v) if (sh.n[v]) fprintf(stderr, " slot %d: %d..%d", v, sh.lo[v], sh.lo[v] + sh.n[v] - 1);
        fprintf(stderr, "\n");
    }
}

// Every buffer the launches of a run need (column-score scratch, list twins) is taken from the context's pool BEFORE the first of
// them starts.  Between the first and the last persistent launch of a run the host makes no memory-management call at all: a
// launch that is already resident never sees the device's page tables change under it (VERDICT r03, weak 2 iv).
static bool pool_regrow(g2g_ctx *ctx, void **p, size_t *cap, size_t need)
{
    if (*cap >= need) return true;
    pool_give(ctx, *p, *cap);
    *p = 0; *cap = 0;
    *p = pool_take(ctx, need, cap);
    if (!*p) *cap = 0;
    return *p != 0;
}
static int take_launch_buffers(g2g_ctx *ctx, g2g_batch *b, const std::vector<Launch> &plan)
{
    for (const Launch &l : plan) {
        if (l.scratch_bytes && !pool_regrow(ctx, (void **) &b->simscr[l.slot], &b->simscr_cap[l.slot], l.scratch_bytes)) { g2g_set_error("%s", "hipMalloc(column-score scratch)"); return G2G_ERR_NOMEM; }
        if (l.twin_bytes && !pool_regrow(ctx, (void **) &batch_twin(b, l.slot), &batch_twin_cap(b, l.slot), l.twin_bytes)) { g2g_set_error("%s", "hipMalloc(list twin image)"); return G2G_ERR_NOMEM; }
    }
    return G2G_OK;
}

// one persistent launch on stream vs; under DEBUG it says what it launches and waits for it
static int launch_variant(g2g_ctx *ctx, g2g_batch *b, const Launch &l, hipStream_t vs, bool dbg)
{
    const G2GVariant &var = G2G_VARIANT[l.slot];
    const int slot = l.slot, cnt = l.cnt;
    const DevProb *probs = b->d_probs;
    const V2Tile *tiles = b->d_tiles + b->var_off[slot];
    double *scr = l.scratch_bytes ? b->simscr[slot] : 0;
    const char *const vname = var.fam == G2G_V7 ? (var.ib ? "v7 (bonus)" : "v7") : (var.ib ? "v8 (bonus)" : "v8");
    char done[48];                  // how the "done" line of DEBUG names this launch
    switch (var.fam) {
    case G2G_V2:
        if (dbg) { fprintf(stderr, "[g2g] variant %d: %d tiles, grid %d x %d threads, lds %zu, cols %d, gen %d\n", slot, cnt, l.grid, l.block, b->lds2, b->v2_cols, b->gen); fflush(stderr); }
        snprintf(done, sizeof done, "variant %d", slot);
        hipLaunchKernelGGL(G2G_KERNEL[slot].v2, dim3(l.grid), dim3(l.block), l.lds, vs, probs, tiles, cnt,
                           batch_qhead(b, slot), b->d_flags, b->gen, (int) b->lds2, l.cols, l.pint, l.pro_off, scr);
        break;
    case G2G_V3_LDS: case G2G_V3R: {
        const V3Lds &LO = batch_v3lds(b, slot);
        const int v = variant_v3_index(slot);
        if (dbg) { fprintf(stderr, "[g2g] v3 variant %d: %d tiles, grid %d, lds %d (rows %d, apool@%d, bpool@%d), cols %d, gen %d\n", v, cnt, l.grid, LO.total, LO.black, LO.aglen, LO.bglen, b->v3_cols, b->gen); fflush(stderr); }
        snprintf(done, sizeof done, "v3 variant %d", v);
        hipLaunchKernelGGL(G2G_KERNEL[slot].v3, dim3(l.grid), dim3(l.block), l.lds, vs, probs, tiles, cnt,
                           batch_qhead(b, slot), b->d_flags, b->gen, LO, l.cols, l.pint, l.pro_off, scr);
        break; }
    case G2G_V6: {
        const V6Lds &LO = batch_v6lds(b, slot);
        const int v = variant_v6_index(slot);
        if (dbg) { fprintf(stderr, "[g2g] v6 variant %d: %d strips, grid %d, lds %d (rings %d / %d entries + tail %d), publish every %d, gen %d\n", v, cnt, l.grid, LO.total, LO.rs[0], LO.rs[1], LO.rtail, l.pint, b->gen); fflush(stderr); }
        snprintf(done, sizeof done, "v6 variant %d", v);
        hipLaunchKernelGGL(G2G_KERNEL[slot].v6, dim3(l.grid), dim3(l.block), l.lds, vs, probs, tiles, cnt,
                           batch_qhead(b, slot), b->d_flags, b->gen, LO, l.pint, l.pro_off, scr, batch_twin(b, slot), l.twin_dw);
        break; }
    case G2G_V7: case G2G_V8:
        if (dbg) { fprintf(stderr, "[g2g] %s variant %d: %d strips, grid %d, publish every %d, gen %d\n", vname, var.noll3 ? 1 : 0, cnt, l.grid, l.pint, b->gen); fflush(stderr); }
        snprintf(done, sizeof done, "%s variant %d", vname, var.noll3 ? 1 : 0);
        hipLaunchKernelGGL(G2G_KERNEL[slot].v7, dim3(l.grid), dim3(l.block), l.lds, vs, probs, tiles, cnt,
                           batch_qhead(b, slot), b->d_flags, b->gen, l.pint, scr);
        break;
    default:
        g2g_set_error("%s", "launch of a variant slot that has no kernel"); return G2G_ERR_DEVICE;
    }
    HIPCHK(hipGetLastError());
    if (dbg) {
        const auto t0 = std::chrono::steady_clock::now();
        hipError_t e3 = hipStreamSynchronize(vs);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (var.fam == G2G_V2) fprintf(stderr, "[g2g] %s done: %s\n", done, hipGetErrorString(e3));
        else fprintf(stderr, "[g2g] %s done: %s, %.1f ms\n", done, hipGetErrorString(e3), ms);
        fflush(stderr);
    }
    return G2G_OK;
}

// the launches of a run, each on its own stream behind the fork event (they are independent of each other, but for the v6
// launches, which wait for the _hf launches' events); the main stream joins every one of them
static int launch_list(g2g_ctx *ctx, g2g_batch *b, const std::vector<Launch> &plan, const ShareOut &sh, const hipStream_t sh_stream[G2G_NVAR])
{
    const bool dbg = g2g_opt(ctx, "DEBUG") != 0;
    int hf_events[G2G_NVS], n_hf_events = 0;
    for (const Launch &l : plan) {
        hipStream_t vs = (sh.shares && sh_stream[l.slot]) ? sh_stream[l.slot] : ctx->vstream[l.k];
        HIPCHK(hipStreamWaitEvent(vs, ctx->vev[G2G_NVS], 0));
        if (l.after_hf) for (int q = 0; q < n_hf_events; ++q) HIPCHK(hipStreamWaitEvent(vs, ctx->vev[hf_events[q]], 0));
        if (int rc = launch_variant(ctx, b, l, vs, dbg)) return rc;
        HIPCHK(hipEventRecord(ctx->vev[l.k], vs));
        HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->vev[l.k], 0));
        if (variant_is_v3(l.slot)) hf_events[n_hf_events++] = l.k;
    }
    return G2G_OK;
}

// v1 (the DPs no strip kernel took), the traceback of all of them, and the end of the device's part of the run
static int finish_run(g2g_ctx *ctx, g2g_batch *b)
{
    if (b->n1) {
        if (g2g_opt(ctx, "DEBUG")) { fprintf(stderr, "[g2g] v1 (state in HBM): %d of %d problems\n", b->n1, b->n); fflush(stderr); }
        hipLaunchKernelGGL(g2g_forward_kernel, dim3(b->n1), dim3(G2G_FWD_THREADS), 0, ctx->stream,
                           (const DevProb *) b->d_probs, (const int *) b->d_idx1);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    hipLaunchKernelGGL(g2g_traceback_kernel, dim3(b->n), dim3(64), 0, ctx->stream, (const DevProb *) b->d_probs, b->n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return G2G_OK;
}

// option STALL_DUMP_FILE: the dumped pipeline of a time-out's DP, appended strip by strip
static void append_stall_dump(const char *fn, int gen, const std::vector<int> &dump)
{
    FILE *fd = fopen(fn, "a");
    if (!fd) return;
    const int nd = std::min(dump[0], (int) G2G_DUMP_STRIPS), ti = dump[1];
    fprintf(fd, "# gen %d, waiter strip %d, %d strips: strip word(gen:col) HW_ID taken pastleft pastfirst pub0 pub1 w0step w0place w1step w1place\n", gen, ti, nd);
    for (int k = 0; k < nd; ++k) { const int *d = dump.data() + 2 + G2G_DUMP_WORDS * k; fprintf(fd, "%d %d:%d %08x %08x %08x %08x %d %d %d %d %d %d\n", ti - 1 - k, (d[0] >> 20) & 0x7FF, d[0] & 0xFFFFF, d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10]); }
    fclose(fd);
}
// the report of a time-out: kept in the context (g2g_ctx_last_timeout: every ordinary run that meets one carries the
// evidence), printed under WARN / DEBUG
static void report_timeout(g2g_ctx *ctx, g2g_batch *b, const int *rep, const std::vector<int> &lost)
{
    TimeoutView t;
    t.x = rep + G2G_HDR; t.dump = 0; t.dump_words = G2G_DUMP_WORDS; t.dump_strips = G2G_DUMP_STRIPS;
    t.gen = b->gen; t.n = b->n; t.fail_off = b->fail_off; t.is_retry = b->is_retry; t.rt_ticks_per_ms = ctx->rt_ticks_per_ms;
    for (int i : lost) { const TimeoutView::Lost l = {i, b->dp[i].v2_ok, b->dp[i].a.right - b->dp[i].a.left, b->dp[i].b.right - b->dp[i].b.left}; t.lost.push_back(l); }
    std::vector<int> dump(2 + G2G_DUMP_WORDS * G2G_DUMP_STRIPS);
    if (b->dump_off > 0 && hipMemcpy(dump.data(), b->d_flags + b->dump_off, sizeof(int) * dump.size(), hipMemcpyDeviceToHost) == hipSuccess && dump[0] > 0) {
        t.dump = dump.data();
        if (const char *fn = g2g_opt(ctx, "STALL_DUMP_FILE")) append_stall_dump(fn, b->gen, dump);
    }
    const std::string text = timeout_report_text(t);
    if (!b->is_retry || ctx->last_timeout.empty()) ctx->last_timeout = text;
    if (!b->injected) { std::lock_guard<std::mutex> lk(g_report_mx); g_last_report = text; }
    if (g2g_opt(ctx, "DEBUG") || g2g_opt(ctx, "WARN")) { fprintf(stderr, "[g2g] s_memrealtime: %.0f ticks/ms; %s\n", ctx->rt_ticks_per_ms, text.c_str()); fflush(stderr); }
}
// A time-out is a rare accident of scheduling, not a property of the DP: the lost DPs first run again on the ordinary
// kernels (a small batch: tens of ms); only if THAT run loses a wait too do its DPs go to v1, which polls nothing.
static int recover_lost(g2g_ctx *ctx, g2g_batch *b, const std::vector<int> &lost)
{
    if (b->force_v1 || lost.empty()) { g2g_set_error("%s", "scheduler: a wait timed out and no DP could be singled out"); return G2G_ERR_DEVICE; }
    std::vector<const g2g_problem *> pp;
    for (int i : lost) pp.push_back(b->src[i]);
    g2g_batch *rb = 0;
    int rc = batch_prepare_impl(ctx, (int) pp.size(), pp.data(), &rb, b->is_retry);
    if (!rc) {
        rb->is_retry = true;
        rc = g2g_batch_run(rb);
        std::vector<g2g_result> rr(pp.size());
        if (!rc) rc = g2g_batch_fetch(rb, rr.data());
        if (!rc) for (size_t k = 0; k < lost.size(); ++k) {
            free(b->recovered[lost[k]].trace);
            b->recovered[lost[k]] = rr[k]; b->was_recovered[lost[k]] = 1;
            b->path_rec[lost[k]] = batch_path(rb, (int) k);
        }
        g2g_batch_free(rb);
    }
    if (rc) { g2g_set_error("%s", "scheduler: the re-run of timed-out DPs failed"); return rc; }
    b->n_recovered += (int) lost.size();
    return G2G_OK;
}
// Some wait ran into the wall-clock limit.  Only the DPs marked in the fail array are lost; they are re-run here, in
// the same call, on the kernel that polls nothing (one workgroup per DP, state in HBM).
static int handle_timeouts(g2g_ctx *ctx, g2g_batch *b, const int *rep)
{
    const int nto = rep[G2G_HDR];
    std::vector<int> fail(b->n);
    HIPCHK(hipMemcpy(fail.data(), b->d_flags + b->fail_off, sizeof(int) * (size_t) b->n, hipMemcpyDeviceToHost));
    std::vector<int> lost;
    for (int i = 0; i < b->n; ++i) if (fail[i] && !b->status[i]) lost.push_back(i);
    b->last_timeouts = nto; b->last_recovered = (int) lost.size();
    ctx->n_timeouts += nto; ctx->n_recovered += (long long) lost.size();
    if (b->is_retry) ctx->n_v1 += (long long) lost.size();
    g_tot[1] += nto; g_tot[2] += (long long) lost.size();
    if (b->is_retry) g_tot[3] += (long long) lost.size();
    if (b->injected) { g_tot[5] += nto; g_tot[6] += (long long) lost.size(); }
    report_timeout(ctx, b, rep, lost);
    return recover_lost(ctx, b, lost);
}

// Compact the valid problems to the front?  No: invalid ones keep kind = -1 and the kernels skip them.
extern "C" int g2g_batch_run(g2g_batch *b)
{
    if (!b) return G2G_ERR_ARG;
    g2g_ctx *ctx = b->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    if (b->n == 0) return G2G_OK;
    std::fill(b->was_recovered.begin(), b->was_recovered.end(), 0);
    b->last_timeouts = b->last_recovered = 0;
    if (!b->is_retry) { ++ctx->n_runs; ++g_tot[0]; }
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    if (b->n2) {
        // persistent tile / strip kernels: one launch per non-empty variant slot.  Everything is decided before anything starts.
        const RunFacts facts = run_facts(ctx, b);
        if (int rc = run_tile_prologue(ctx, b, plan_pro_off(facts))) return rc;
        if (int rc = write_wait_header(ctx, b)) return rc;
        ShareOut sh;
        hipStream_t sh_stream[G2G_NVAR];
        resolve_shares(ctx, facts, sh, sh_stream);
        const std::vector<Launch> plan = launch_plan(facts, sh);
        if (int rc = take_launch_buffers(ctx, b, plan)) return rc;
        if (int rc = launch_list(ctx, b, plan, sh, sh_stream)) return rc;
    }
    if (int rc = finish_run(ctx, b)) return rc;
    if (b->d_flags) {
        int rep[G2G_HDR + G2G_HDRN];
        HIPCHK(hipMemcpy(rep, b->d_flags, sizeof rep, hipMemcpyDeviceToHost));
        if (rep[G2G_HDR + 40]) {             // waves that were off the machine while they waited: evidence, not an error
            const double gap_ms = rep[G2G_HDR + 41] * 1024. / ctx->rt_ticks_per_ms;
            ctx->n_gaps += rep[G2G_HDR + 40]; g_tot[4] += rep[G2G_HDR + 40];
            if (gap_ms > ctx->max_gap_ms) ctx->max_gap_ms = gap_ms;
            if (g2g_opt(ctx, "DEBUG") || g2g_opt(ctx, "WARN")) { fprintf(stderr, "[g2g] %d waiting wave(s) were off the machine for more than 4 ms at a stretch (longest %.1f ms); batch of %d DPs, %d wait(s) lost; %zu CU-mask streams alive, %lld created\n", rep[G2G_HDR + 40], gap_ms, b->n, rep[G2G_HDR], ctx->mstream.size(), ctx->n_mstreams); fflush(stderr); }
        }
        if (rep[G2G_HDR]) if (int rc = handle_timeouts(ctx, b, rep)) return rc;
    }
    HIPCHK(hipEventElapsedTime(&b->fwd_ms, ctx->ev[0], ctx->ev[1]));
    HIPCHK(hipEventElapsedTime(&b->tb_ms, ctx->ev[1], ctx->ev[2]));
    return G2G_OK;
}

extern "C" int g2g_batch_fetch(g2g_batch *b, g2g_result *res)
{
    if (!b || !res) return G2G_ERR_ARG;
    g2g_ctx *ctx = b->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<char> all(b->out_hi - b->out_lo);
    if (!all.empty()) HIPCHK(hipMemcpy(all.data(), b->d_arena + b->out_lo, all.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < b->n; ++i) {
        res[i].status = b->status[i];
        res[i].cells = b->cells[i];
        res[i].trace = 0; res[i].ntrace = 0; res[i].score = 0;
        if (b->status[i]) continue;
        if (b->was_recovered[i]) {                      // (re-run after a time-out: a copy, the batch may be fetched again)
            res[i] = b->recovered[i];
            res[i].trace = (g2g_skl *) malloc(sizeof(g2g_skl) * (size_t) (res[i].ntrace > 0 ? res[i].ntrace : 1));
            memcpy(res[i].trace, b->recovered[i].trace, sizeof(g2g_skl) * (size_t) res[i].ntrace);
            continue;
        }
        const char *tmp = all.data() + (b->out_off[i] - b->out_lo);
        memcpy(&res[i].score, tmp, sizeof(double));
        int nt, rr0;
        memcpy(&nt, tmp + sizeof(double), sizeof(int));
        memcpy(&rr0, tmp + sizeof(double) + sizeof(int), sizeof(int));
        res[i].rr[0] = rr0;
        res[i].rr[1] = b->rr1[i];
        if (nt < 2 || nt > b->tcap[i]) { res[i].status = G2G_ERR_DEVICE; continue; }
        res[i].ntrace = nt;
        res[i].trace = (g2g_skl *) malloc(sizeof(g2g_skl) * nt);
        memcpy(res[i].trace, tmp + sizeof(double) + 2 * sizeof(int), sizeof(g2g_skl) * nt);
    }
    return G2G_OK;
}

// Which kernel generation a problem runs on (after g2g_batch_prepare) / produced the result g2g_batch_fetch returns (after
// g2g_batch_run: a DP re-run after a lost wait reports the kernel of its successful re-run).  1 g2g_forward_kernel, 2 the
// 8-lanes-per-cell strips, 3 v3 / v3r, 6, 7, 8; 0 for a problem that was refused (g2g_result::status).
extern "C" int g2g_batch_paths(const g2g_batch *b, int32_t *gen)
{
    if (!b || !gen) { g2g_set_error("g2g_batch_paths: %s", "bad argument"); return G2G_ERR_ARG; }
    for (int i = 0; i < b->n; ++i) gen[i] = batch_path(b, i);
    return G2G_OK;
}

extern "C" void g2g_batch_times(const g2g_batch *b, float *fwd_ms, float *tb_ms)
{
    if (fwd_ms) *fwd_ms = b ? b->fwd_ms : 0;
    if (tb_ms) *tb_ms = b ? b->tb_ms : 0;
}

extern "C" long long g2g_batch_cells(const g2g_batch *b)
{
    long long c = 0;
    if (b) for (int i = 0; i < b->n; ++i) if (!b->status[i]) c += b->cells[i];
    return c;
}

extern "C" size_t g2g_batch_arena_bytes(const g2g_batch *b) { return b ? b->arena_bytes : 0; }

extern "C" void g2g_batch_recovery(const g2g_batch *b, int *timeouts_last_run, int *recovered_last_run, int *recovered_total)
{
    if (timeouts_last_run) *timeouts_last_run = b ? b->last_timeouts : 0;
    if (recovered_last_run) *recovered_last_run = b ? b->last_recovered : 0;
    if (recovered_total) *recovered_total = b ? b->n_recovered : 0;
}
extern "C" const char *g2g_ctx_last_timeout(const g2g_ctx *c) { return c ? c->last_timeout.c_str() : ""; }
extern "C" void g2g_ctx_wait_gaps(const g2g_ctx *c, long long *count, double *longest_ms)
{
    if (count) *count = c ? c->n_gaps : 0;
    if (longest_ms) *longest_ms = c ? c->max_gap_ms : 0;
}
extern "C" void g2g_process_counters(long long out[8])
{
    if (out) for (int k = 0; k < 8; ++k) out[k] = g_tot[k].load();
}
extern "C" size_t g2g_process_last_timeout(char *buf, size_t cap)
{
    std::lock_guard<std::mutex> lk(g_report_mx);
    if (buf && cap) { const size_t n = std::min(cap - 1, g_last_report.size()); memcpy(buf, g_last_report.data(), n); buf[n] = 0; }
    return g_last_report.size();
}
extern "C" void g2g_ctx_counters(const g2g_ctx *c, long long out[4])
{
    if (!out) return;
    out[0] = c ? c->n_runs : 0; out[1] = c ? c->n_timeouts : 0; out[2] = c ? c->n_recovered : 0; out[3] = c ? c->n_v1 : 0;
}

extern "C" void g2g_batch_free(g2g_batch *b)
{
    if (!b) return;
    hipSetDevice(b->ctx->device);
    release_arena(b);
    pool_give(b->ctx, b->d_tiles, b->tiles_cap);
    pool_give(b->ctx, b->d_flags, b->flags_cap);
    for (int k = 0; k < G2G_NVAR; ++k) pool_give(b->ctx, b->simscr[k], b->simscr_cap[k]);
    for (int k = 0; k < 6; ++k) pool_give(b->ctx, b->twin[k], b->twin_cap[k]);
    for (size_t i = 0; i < b->recovered.size(); ++i) free(b->recovered[i].trace);
    delete b;
}

#ifdef G2G_V6_STAMP
extern "C" void g2g_v6_stamps(unsigned long long *out, int reset)
{
    hipMemcpyFromSymbol(out, HIP_SYMBOL(g2g_v6_stamp_acc), sizeof(unsigned long long) * 16);
    if (reset) { unsigned long long z[16] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(g2g_v6_stamp_acc), z, sizeof z); }
}
#endif
#ifdef G2G_V2_STAMP
extern "C" void g2g_stamps(unsigned long long *out) { hipMemcpyFromSymbol(out, HIP_SYMBOL(g2g_stamp_acc), sizeof(unsigned long long) * 16); }
extern "C" void g2g_waits(unsigned long long *out) { hipMemcpyFromSymbol(out, HIP_SYMBOL(g2g_wait_acc), sizeof(unsigned long long) * 4); }
#endif

// f1: PreSpScore::calcSpScore on the problems of a prepared batch (their inputs are resident in HBM)
// nsets skeletons per problem of the batch in ONE launch (entry e = set e / b->n of problem e % b->n): the windows of g2g_refine
// score the current and the new alignment of every division on the batch the DPs ran on, without packing the problems again
// One set of calcSpScore walks in flight: launched on a stream (spscore_launch: uploads, g2g_spprep_kernel, g2g_spscore_kernel, the
// copies back), collected later (spscore_finish).  The host images the asynchronous copies read live in the object.
struct SpRun {
    int n, nb; char *d; size_t d_cap, o_out, o_st, b_out, b_int; hipStream_t s;
    std::vector<g2g_skl> all; std::vector<int> off, cnt, colpre; std::vector<long long> goff, soff; std::vector<g2g_spparams> sp;
    std::vector<double> ho; std::vector<int> hs;
    hipError_t e;
    SpRun() : n(0), nb(0), d(0), d_cap(0), o_out(0), o_st(0), b_out(0), b_int(0), s(0), e(hipSuccess) {}
};
static int spscore_launch(g2g_batch *b, int nsets, const g2g_spparams *sp, const g2g_skl *const *skl, const int *nskl, hipStream_t stream,
                          void **slots, size_t *slots_cap, SpRun &R)
{
    g2g_ctx *ctx = b->ctx;
    const int nb = b->n;
    const int n = nsets * nb;
    R.n = n; R.nb = nb;
    std::vector<int> &off = R.off, &cnt = R.cnt;
    off.assign(n, 0); cnt.assign(n, 0);
    size_t tot = 0;
    for (int i = 0; i < n; ++i) { off[i] = (int) tot; cnt[i] = (skl[i] && nskl[i] > 0) ? nskl[i] : 0; tot += cnt[i]; }
    std::vector<g2g_skl> &all = R.all;
    all.assign(tot ? tot : 1, g2g_skl());
    for (int i = 0; i < n; ++i) if (cnt[i]) memcpy(&all[off[i]], skl[i], sizeof(g2g_skl) * cnt[i]);
    const size_t b_skl = sizeof(g2g_skl) * all.size(), b_int = sizeof(int) * n, b_sp = sizeof(g2g_spparams) * n, b_out = sizeof(double) * 6 * n;
    char *d = 0;
    R.sp.assign(sp, sp + n);
    const size_t o_skl = 0, o_off = (b_skl + 15) & ~(size_t) 15, o_cnt = o_off + ((b_int + 15) & ~(size_t) 15),
                 o_sp = o_cnt + ((b_int + 15) & ~(size_t) 15), o_out = o_sp + ((b_sp + 15) & ~(size_t) 15),
                 o_st = o_out + ((b_out + 15) & ~(size_t) 15);
    // Gep1st rings (Noll 3): (a.many + b.many) x (codonk1 + 1) ints per problem; naive units: their gap-length arrays; zeroed
    std::vector<long long> &goff = R.goff;
    goff.assign(n, -1);
    size_t gints = 0;
    for (int i = 0; i < n; ++i) {
        const DevProb &dp = b->dp[i % nb];
        const bool rings = dp.kind >= 1 && dp.noll == 3 && dp.codonk1 > 0 && dp.codonk1 < (1 << 20);
        if (rings || dp.kind == 3) {                      // kind 3 (naive units): + gla[an], glb[bn] in front of the rings
            goff[i] = (long long) gints;
            if (dp.kind == 3) gints += (size_t) dp.a.many + dp.b.many + 2;
            if (rings) gints += (size_t) (dp.a.many + dp.b.many) * ((size_t) dp.codonk1 + 1);
        }
    }
    // the streamed walk (kinds 1 and 2: g2g_spprep_kernel lays the position-only inputs of every path column out in path order):
    // colpre = path columns up to and including each skeleton segment, soff = first slot of each alignment (-1: walks unstreamed)
    std::vector<int> &colpre = R.colpre;
    colpre.assign(all.size(), 0);
    std::vector<long long> &soff = R.soff;
    soff.assign(n, -1);
    size_t nslots = 0;
    int maxcols = 0;
    const bool streamed = !g2g_opt(ctx, "NO_SPSTREAM");
    for (int i = 0; i < n && streamed; ++i) {
        const DevProb &dp = b->dp[i % nb];
        if ((dp.kind != 1 && dp.kind != 2) || cnt[i] < 2 || b->status[i % nb]) continue;
        long long cols = 0;
        bool good = true;
        for (int k = 1; k < cnt[i] && good; ++k) {
            const int mi = all[off[i] + k].m - all[off[i] + k - 1].m, ni = all[off[i] + k].n - all[off[i] + k - 1].n;
            if (mi < 0 || ni < 0) good = false;
            cols += std::max(mi, ni);
            if (cols > (1 << 28)) good = false;
            colpre[off[i] + k] = (int) cols;
        }
        if (!good || cols == 0) continue;
        soff[i] = (long long) nslots; nslots += (size_t) cols; maxcols = std::max(maxcols, (int) cols);
    }
    if (nslots * sizeof(SpSlot) > ((size_t) 4 << 30)) { std::fill(soff.begin(), soff.end(), -1LL); nslots = 0; }
    if (nslots * sizeof(SpSlot) > (*slots_cap)) {
        if ((*slots)) hipFree((*slots));
        (*slots) = 0; (*slots_cap) = 0;
        const size_t want = nslots * sizeof(SpSlot) + (nslots * sizeof(SpSlot)) / 4;
        if (hipMalloc(&(*slots), want) == hipSuccess) (*slots_cap) = want;
        else { (void) hipGetLastError(); std::fill(soff.begin(), soff.end(), -1LL); nslots = 0; }       // no room: the walks read in place
    }
    const size_t b_goff = sizeof(long long) * n, o_goff = (o_st + b_int + 15) & ~(size_t) 15,
                 o_gws = (o_goff + b_goff + 15) & ~(size_t) 15, o_cpre = (o_gws + sizeof(int) * (gints ? gints : 1) + 15) & ~(size_t) 15,
                 o_soff = (o_cpre + sizeof(int) * colpre.size() + 15) & ~(size_t) 15, total = o_soff + b_goff;
    size_t d_cap = 0;
    d = (char *) pool_take(ctx, total, &d_cap);
    R.d = d; R.d_cap = d_cap; R.o_out = o_out; R.o_st = o_st; R.b_out = b_out; R.b_int = b_int; R.s = stream;
    if (!d) { g2g_set_error("%s", "spscore: out of device memory"); return G2G_ERR_NOMEM; }
    hipError_t e = hipMemcpyAsync(d + o_skl, all.data(), b_skl, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_off, off.data(), b_int, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_cnt, cnt.data(), b_int, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_sp, R.sp.data(), b_sp, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_goff, goff.data(), b_goff, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && gints) e = hipMemsetAsync(d + o_gws, 0, sizeof(int) * gints, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_cpre, colpre.data(), sizeof(int) * colpre.size(), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_soff, soff.data(), b_goff, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && nslots) {
        hipLaunchKernelGGL(g2g_spprep_kernel, dim3((unsigned) std::min(64, (maxcols + 255) / 256), (unsigned) n), dim3(256), 0, stream,
                           (const DevProb *) b->d_probs, n, nb, (const int2 *) (d + o_skl), (const int *) (d + o_off), (const int *) (d + o_cnt),
                           (const int *) (d + o_cpre), (const long long *) (d + o_soff), (SpSlot *) (*slots));
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(g2g_spscore_kernel, dim3(n), dim3(64), 0, stream, (const DevProb *) b->d_probs, n, nb,
                           (const SpParamsDev *) (d + o_sp), (const int2 *) (d + o_skl), (const int *) (d + o_off),
                           (const int *) (d + o_cnt), (double *) (d + o_out), (int *) (d + o_st),
                           gints ? (int *) (d + o_gws) : (int *) 0, (const long long *) (d + o_goff),
                           (const int *) (d + o_cpre), (const long long *) (d + o_soff), nslots ? (const SpSlot *) (*slots) : (const SpSlot *) 0,
                           g2g_opt(ctx, "NO_SPLANES") ? 1 : 0);
        e = hipGetLastError();
    }
    R.ho.assign(6 * (size_t) n, 0.);
    R.hs.assign(n, 0);
    if (e == hipSuccess) e = hipMemcpyAsync(R.ho.data(), d + o_out, b_out, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(R.hs.data(), d + o_st, b_int, hipMemcpyDeviceToHost, stream);
    R.e = e;
    return G2G_OK;
}
static int spscore_finish(g2g_batch *b, SpRun &R, g2g_fstat *out)
{
    g2g_ctx *ctx = b->ctx;
    hipError_t e = R.e;
    if (e == hipSuccess) e = hipStreamSynchronize(R.s);
    else (void) hipStreamSynchronize(R.s);
    pool_give(ctx, R.d, R.d_cap);
    R.d = 0;
    if (e != hipSuccess) { g2g_set_error("spscore: %s", hipGetErrorString(e)); (void) hipGetLastError(); return G2G_ERR_DEVICE; }
    const int n = R.n, nb = R.nb;
    for (int i = 0; i < n && out; ++i) {
        out[i].val = R.ho[6 * i]; out[i].gap = R.ho[6 * i + 1]; out[i].raw = R.ho[6 * i + 2]; out[i].reserved = 0;
        out[i].mch = R.ho[6 * i + 3]; out[i].mmc = R.ho[6 * i + 4]; out[i].unp = R.ho[6 * i + 5];
        out[i].status = b->status[i % nb] ? b->status[i % nb] : R.hs[i] == 0 ? G2G_OK : R.hs[i] == -2 ? G2G_ERR_MODE : G2G_ERR_ARG;
    }
    return G2G_OK;
}
static bool spscore_lists_in_state(const g2g_batch *b)
{   // the walkers keep their running lists in LDS unless the problem's capacities exceed SP_FAST_LIST entries -- then they use the problem's
    // own state arrays: two walks of one problem (and a walk beside the DP itself) must then go one after the other
    for (int i = 0; i < b->n; ++i) if (b->dp[i].capa + 1 > SP_FAST_LIST || b->dp[i].capb + 1 > SP_FAST_LIST) return true;
    return false;
}
extern "C" int g2g_batch_spscore_sets(g2g_batch *b, int nsets, const g2g_spparams *sp, const g2g_skl *const *skl, const int *nskl, g2g_fstat *out)
{
    if (!b || nsets < 1 || !sp || !skl || !nskl || !out) return G2G_ERR_ARG;
    g2g_ctx *ctx = b->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const int nb = b->n;
    if (nb == 0) return G2G_OK;
    if (nsets > 1 && spscore_lists_in_state(b)) {
        for (int k = 0; k < nsets; ++k) {
            const int rc = g2g_batch_spscore_sets(b, 1, sp + (size_t) k * nb, skl + (size_t) k * nb, nskl + (size_t) k * nb, out + (size_t) k * nb);
            if (rc) return rc;
        }
        return G2G_OK;
    }
    SpRun R;
    const int rc = spscore_launch(b, nsets, sp, skl, nskl, ctx->stream, &ctx->sp_slots, &ctx->sp_slots_cap, R);
    if (rc) return rc;
    return spscore_finish(b, R, out);
}
// One set of walks BESIDE the DP kernels of the batch (g2g_align2_score_batch: the current alignments' calcSpScore needs only the inputs,
// which are resident once the batch is prepared): launched on a stream of its own before g2g_batch_run, collected after it.  *handle
// stays NULL when the walks do not run beside the DPs (the default, see below; or their lists would live in the problems' state arrays):
// the caller then scores both sets after the run, as before.
extern "C" int g2g_batch_spscore_begin(g2g_batch *b, const g2g_spparams *sp, const g2g_skl *const *skl, const int *nskl, void **handle)
{
    if (!b || !sp || !skl || !nskl || !handle) return G2G_ERR_ARG;
    *handle = 0;
    g2g_ctx *ctx = b->ctx;
    // OFF by default: measured on the 256 x 1024 refinement the window got SLOWER with the walks beside the DPs (113.3 against 105.6 ms:
    // 16 latency-bound pipelines do not tolerate neighbours on their CUs, and the packing of the walks delays the DP launches) -- the
    // 3 ms of walks it hides cost 8.  Option SP_OVERLAP turns it on (tests keep the path alive).
    if (b->n == 0 || spscore_lists_in_state(b) || !g2g_opt(ctx, "SP_OVERLAP")) return G2G_OK;
    HIPCHK(hipSetDevice(ctx->device));
    if (!ctx->sp_stream) {
        if (hipStreamCreateWithFlags(&ctx->sp_stream, hipStreamNonBlocking) != hipSuccess) { (void) hipGetLastError(); ctx->sp_stream = 0; return G2G_OK; }
        if (hipEventCreateWithFlags(&ctx->sp_ev, hipEventDisableTiming) != hipSuccess) { (void) hipGetLastError(); hipStreamDestroy(ctx->sp_stream); ctx->sp_stream = 0; return G2G_OK; }
    }
    HIPCHK(hipEventRecord(ctx->sp_ev, ctx->stream));                 // (the batch's inputs were uploaded on the main stream)
    HIPCHK(hipStreamWaitEvent(ctx->sp_stream, ctx->sp_ev, 0));
    SpRun *R = new SpRun();
    const int rc = spscore_launch(b, 1, sp, skl, nskl, ctx->sp_stream, &ctx->sp_slots2, &ctx->sp_slots2_cap, *R);
    if (rc) { delete R; return rc; }
    *handle = R;
    return G2G_OK;
}
extern "C" int g2g_batch_spscore_end(g2g_batch *b, void *handle, g2g_fstat *out)       // out NULL: wait and drop
{
    if (!b || !handle) return G2G_ERR_ARG;
    SpRun *R = (SpRun *) handle;
    const int rc = spscore_finish(b, *R, out);
    delete R;
    return rc;
}

extern "C" int g2g_batch_spscore(g2g_batch *b, const g2g_spparams *sp, const g2g_skl *const *skl, const int *nskl, g2g_fstat *out)
{
    return g2g_batch_spscore_sets(b, 1, sp, skl, nskl, out);
}

// upper estimate of the arena bytes one problem takes in a batch (inputs + state + trace + column scores)
static size_t problem_bytes(const g2g_ctx *ctx, const g2g_problem *p)
{
    if (check_problem(p)) return 4096;
    const int al = p->a.left, ar = p->a.right, bl = p->b.left, br = p->b.right;
    const BandCells bc = band_cells(al, ar, bl, br, is_rect(p->alnmode) ? bl - ar : p->lw, is_rect(p->alnmode) ? br - al : p->up);
    const long long cells = bc.cells;
    const int tmax = bc.tstride;
    // trace (1 B per cell) + the column-score matrix (8 B per cell) where a kernel reads one: strips in sweep mode (the
    // default of every tiled kernel) make their own scores
    const bool matrix = g2g_opt(ctx, "NO_SIMBLK") || g2g_opt(ctx, "V2_SWEEP") || g2g_opt(ctx, "V3_SWEEP");   // (tile-mode test configurations)
    size_t bytes = (size_t) (ar - al + br - bl + 2) * tmax + (matrix ? 8 * (size_t) cells : 0);
    const g2g_side *sd[2] = {&p->a, &p->b};
    for (int k = 0; k < 2; ++k) {
        const size_t cols = (size_t) sd[k]->len + 2;
        bytes += cols * sd[k]->many * (kind_of(p->alnmode) == 3 ? 17 : 1) + cols * 24 + cols * 8 * (size_t) ((sd[k]->pseq && sd[k]->nelm > 0) ? sd[k]->nelm : 0);    // (nelm of a side without vectors is not defined)
        if (sd[k]->has_gfq) for (int v = 0; v < 3; ++v) bytes += 12 * (size_t) sd[k]->gfq.off[v][sd[k]->len + 1] + 4 * cols;
    }
    const size_t lists = 8 * (size_t) ((p->a.has_gfq ? p->a.gfq.hetero + 1 : p->a.many) + (p->b.has_gfq ? p->b.gfq.hetero + 1 : p->b.many));
    bytes += (size_t) ((is_rect(p->alnmode) ? (br - al) - (bl - ar) : p->up - p->lw) + 3) * 7 * (16 + lists);      // v1 state rows
    bytes += (size_t) (p->b.len + 3 + ar - al + 3) * 9 * (16 + lists / 2 + 16);                 // strip / block boundary records
    bytes += 8 * (size_t) (ar - al + 2) + 8 * (size_t) (ar - al + br - bl + 8) + 4096;
    return bytes;
}

// alignC<recd_t> for n problems.  Batches are cut so that one arena stays below a budget (default: 70 % of the free
// device memory, capped by G2G_ARENA_LIMIT_GB): a sweep over thousands of large divisions (BASELINE configs[4]:
// 4093 divisions of a 2048 x 4096 nt family) does not fit 288 GB at once.
extern "C" int g2g_forward_batch(g2g_ctx *ctx, int n, const g2g_problem *const *prob, g2g_result *res)
{
    if (!ctx || n < 0 || (n && (!prob || !res))) return G2G_ERR_ARG;
    if (!ctx->ok) return G2G_ERR_NODEVICE;
    HIPCHK(hipSetDevice(ctx->device));
    size_t budget = (size_t) 64 << 30;              // per chunk (128 GB chunks were no faster on a 3.3e10-cell DNA sweep)
    { size_t fr = 0, tot = 0; if (hipMemGetInfo(&fr, &tot) == hipSuccess && fr) budget = std::min(budget, (size_t) (0.7 * (double) fr)); }
    if (const char *e = g2g_opt(ctx, "ARENA_LIMIT_GB")) { const double g = atof(e); if (g > 0) budget = (size_t) (g * (double) ((size_t) 1 << 30)); }
    for (int i = 0; i < n; ++i) { res[i].trace = 0; res[i].ntrace = 0; }
    int lo = 0;
    while (lo < n) {
        size_t acc = 0;
        int hi = lo;
        while (hi < n) {
            const size_t pb = problem_bytes(ctx, prob[hi]);
            if (hi > lo && (acc + pb > budget || hi - lo >= G2G_MAX_BATCH)) break;
            acc += pb; ++hi;
        }
        if (g2g_opt(ctx, "DEBUG")) { fprintf(stderr, "[g2g] forward_batch: chunk [%d, %d) of %d, %.3g of %.3g bytes\n", lo, hi, n, (double) acc, (double) budget); fflush(stderr); }
        g2g_batch *b = 0;
        int rc = g2g_batch_prepare(ctx, hi - lo, prob + lo, &b);
        if (!rc) {
            rc = g2g_batch_run(b);
            if (!rc) rc = g2g_batch_fetch(b, res + lo);
            g2g_batch_free(b);
        }
        if (rc) {             // the call fails as a whole: nothing of the finished chunks is handed out
            for (int i = 0; i < hi; ++i) { free(res[i].trace); res[i].trace = 0; res[i].ntrace = 0; }
            return rc;
        }
        lo = hi;
    }
    return G2G_OK;
}

#include "g2g_dist.hip"                // f3: the guide-tree DPs (own kernels, own entry point; shares the context)
#include "g2g_pairaln.hip"             // f3: alignB_ng (pairwise alignment of single sequences with the path)
#include "g2g_pairsum.hip"             // f1: Ssrel::pairsum_ss (naive nodes on the GPU, joins through calcSpScore)
#include "g2g_ktree.hip"               // the weighting tree of an MSA: divergence kernel, UPGMA, Kirchhoff weights
#include "g2g_ktree_groups.hip"        // the weighting tree over given groups: group divergence kernels, preset leaves, phyl_pwt
#include "g2g_kmer.hip"                // k-mer composition distances of unaligned sequences: profile and pair kernels, closed forms
#include "g2g_consreg.hip"             // the conserved regions of an MSA: Ssrel::constwo / consreg (column scores and the range scan)
#include "g2g_build.hip"             // a8 / a9: thickness, vectors and gap profiles of a batch of groups on the device
