// arvx_capi.hip -- host side of libarvx.so: the C-ABI declared in
// include/arvx/arvx.h over the gfx950 kernels.  No CPU compute path exists
// here: every entry point that does work launches HIP kernels and fails with
// ARVX_ERR_HIP when no device is usable.
#include "arvx/arvx.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "arvx_ctx.h"
#include "carve_kernels.h"
#include "pixel_cache_kernels.h"
#include "rect_cache_kernels.h"
#ifdef ARVX_EXPERIMENTS
#include "carve_stream_kernels.h"  // the one-launch carve: loses by 11-24 %, experiment builds only
#endif
#include "views_kernels.h"
#include "segment_kernels.h"
#include "state_kernels.h"
#include "undistort_kernels.h"
#include "color_kernels.h"
#include "closure_kernels.h"
#include "bitplane_kernels.h"
#include "fast_carve_kernels.h"
#include "mc_kernels.h"
#include "mc_mesh_kernels.h"
#include "mc_weld_kernels.h"
#include "mc_smooth_kernels.h"
#include "mesh_relax_kernels.h"
#include "mc_decimate_kernels.h"
#include "mc_refine_kernels.h"
#include "visibility_kernels.h"
#include "photo_kernels.h"
#include "components_kernels.h"
#include "distance_kernels.h"
#include "vote_kernels.h"
#include "render_kernels.h"
#include "render_mesh_kernels.h"
#include "render_mesh_clip_kernels.h"
#include "mesh_color_kernels.h"
#include "mesh_texture_kernels.h"
#include "exchange_kernels.h"
#include <algorithm>

namespace {

thread_local std::string g_last_error;
// the grouping new contexts start with (arvx_set_projection_assoc)
std::atomic<int> g_default_assoc{ARVX_ASSOC_LEFT};

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

}  // namespace

namespace arvx {
int fail_hip(hipError_t e, const char *what, const char *file, int line) {
    return fail(ARVX_ERR_HIP, "%s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
}
int fail_msg(int code, const char *msg) { return fail(code, "%s", msg); }
}  // namespace arvx

using arvx::Ctx;
using Event = Ctx::Event;
using Form = Ctx::Form;

#define ARVX_CHECK_CTX(ctx)                                          \
    do {                                                             \
        if (!(ctx)) return fail(ARVX_ERR_INVALID, "null context");   \
        ARVX_HIP(hipSetDevice((ctx)->device));                       \
    } while (0)

#define ARVX_TRY(expr)                                    \
    do {                                                  \
        if (int arvx_rc_ = (expr)) return arvx_rc_;       \
    } while (0)

// ---- launches ---------------------------------------------------------------------------
// Every kernel of this file goes out through launch(): on the context's stream as it stands at the
// call (ExchangeStreamScope swaps that member), checked straight after the launch, a failure
// reported with the line of the stage that launched.  The arguments convert to the kernel's own
// parameter types, so a call casts only what does not convert by itself (a void pointer).
struct LaunchSite {  // the context and, through the default argument, the line of the call
    const Ctx *ctx;
    int line;
    LaunchSite(const Ctx *c, int l = __builtin_LINE()) : ctx(c), line(l) {}
};
struct Lds {  // bytes of dynamic LDS of a launch
    size_t bytes;
};
template <class... P>
[[nodiscard]] static int launch(LaunchSite at, void (*kernel)(P...), dim3 grid, dim3 block, Lds lds,
                                std::common_type_t<P>... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds.bytes, at.ctx->stream, args...);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ARVX_OK : arvx::fail_hip(e, "kernel launch", __FILE__, at.line);
}
template <class... P>
[[nodiscard]] static int launch(LaunchSite at, void (*kernel)(P...), dim3 grid, dim3 block,
                                std::common_type_t<P>... args) {
    return launch(at, kernel, grid, block, Lds{0}, args...);
}

// workgroups of `per` for n entries
static unsigned blocks_for(size_t n, size_t per = 256) { return (unsigned)((n + per - 1) / per); }

// The entry points of the occupancy hand-off (pack / compress / expand) launch on the
// context's exchange stream when the caller has set one: everything they launch inside goes
// there, and the caller orders the two streams with events.
struct ExchangeStreamScope {
    Ctx *ctx;
    hipStream_t saved;
    explicit ExchangeStreamScope(Ctx *c) : ctx(c), saved(c->stream) {
        if (c->xstream) c->stream = c->xstream;
    }
    ~ExchangeStreamScope() { ctx->stream = saved; }
};

// ---- streams ----------------------------------------------------------------------------
// hipStreamCreate / hipStreamDestroy cost 1.4 - 2.2 ms each on this stack (rocprofv3
// --hip-trace of tools/cpp/arvx_bench6: more than the whole carve of its largest model), and a
// drop-in caller makes a context per Model (src/main.cpp:306-440 builds eight in a row): the
// streams of destroyed contexts are kept per device and handed to the next context.
// A/B switches of the launch path.  The shipped library reads NO environment variable: its
// behaviour never depends on the caller's environment.  An experiment build
// (make EXTRA=-DARVX_EXPERIMENTS, e.g. into ab_libs/ for tools/carve_ab.py) turns the same
// names into environment switches again.
#ifdef ARVX_EXPERIMENTS
static bool experiment_flag(const char *name) { return getenv(name) != nullptr; }
static int experiment_int(const char *name) { return getenv(name) ? atoi(getenv(name)) : 0; }
#else
static constexpr bool experiment_flag(const char *) { return false; }
static constexpr int experiment_int(const char *) { return 0; }
#endif

namespace {
std::mutex g_stream_mutex;
std::vector<std::pair<int, hipStream_t>> g_idle_streams;  // (device, stream), idle and drained

hipError_t acquire_stream(int device, hipStream_t *out) {
    static const bool no_reuse = experiment_flag("ARVX_NO_STREAM_REUSE");
    if (!no_reuse) {
        std::lock_guard<std::mutex> lock(g_stream_mutex);
        for (size_t i = 0; i < g_idle_streams.size(); ++i)
            if (g_idle_streams[i].first == device) {
                *out = g_idle_streams[i].second;
                g_idle_streams.erase(g_idle_streams.begin() + i);
                return hipSuccess;
            }
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}

void release_stream(int device, hipStream_t s) {  // s: synchronised by the caller
    static const bool no_reuse = experiment_flag("ARVX_NO_STREAM_REUSE");
    std::lock_guard<std::mutex> lock(g_stream_mutex);
    if (!no_reuse && g_idle_streams.size() < 64) {
        g_idle_streams.emplace_back(device, s);
        return;
    }
    (void)hipStreamDestroy(s);
}
}  // namespace

// ---- bit-plane helpers (bitplane_kernels.h) ----------------------------------------------

// After a synchronisation of ctx->stream: did a kernel that waits for other workgroups give up
// (arvx_ctx.h, h_fault)?  The results of that launch are then undefined.
static int check_fault(Ctx *ctx) {
    if (!ctx->h_fault || !*ctx->h_fault) return ARVX_OK;
    const unsigned what = *ctx->h_fault;
    *ctx->h_fault = 0u;
    ctx->vstrip_key = 0;   // the ticket counters no longer match the launches: start over
    ctx->carve_layout = 0;
    ctx->stream_layout = 0;
    // (the scans' tickets and status granules too: a chunk that gave up published a prefix under a
    // valid tag -- the control block is zeroed again at its next use)
    ctx->pool_compact.release();
    ctx->compact_tickets = 0;
    ctx->compact_epoch = 0;
    ctx->counts_clean[0] = ctx->counts_clean[1] = false;
    ctx->packets_seq = 0;
    return fail(ARVX_ERR_HIP, "a kernel gave up waiting for another workgroup (mark %u): the "
                "results of the calls since the last synchronisation are undefined", what);
}

#define ARVX_SYNC(ctx)                                        \
    do {                                                      \
        ARVX_HIP(hipStreamSynchronize((ctx)->stream));        \
        if (int arvx_f_ = check_fault(ctx)) return arvx_f_;   \
    } while (0)

static int need_rec(Ctx *ctx, bool lazy_ok = false);
static arvx::CarveParams record_params(const Ctx *ctx);

// the paint plane where it takes part (null: nobody is painted)
static const unsigned long long *paint_plane(const Ctx *ctx) {
    return ctx->paint_valid ? (const unsigned long long *)ctx->pool_paint.p : nullptr;
}

// one context holds every plane of the grid: what the stages with global connectivity ask for
static bool whole_grid(const Ctx *ctx) { return ctx->stripe_world <= 1 && ctx->z0 == 0 && ctx->z1 == ctx->Z; }

// the bit planes (bitplane_kernels.h) of `planes` planes of the grid (default: the owned ones), and
// their words
static arvx::BitGrid bit_grid(const Ctx *ctx, int planes) {
    return arvx::BitGrid{ctx->X, ctx->Y, planes, (ctx->X + 63) / 64};
}
static arvx::BitGrid bit_grid(const Ctx *ctx) { return bit_grid(ctx, ctx->z1 - ctx->z0); }
static size_t bit_words(const arvx::BitGrid &g) { return (size_t)g.XW * g.Y * g.Z; }

// compute units of the context's device (cached)
static int compute_units(Ctx *ctx) {
    if (ctx->ncu <= 0) {
        ctx->ncu = 256;
        (void)hipDeviceGetAttribute(&ctx->ncu, hipDeviceAttributeMultiprocessorCount, ctx->device);
        if (ctx->ncu <= 0) ctx->ncu = 256;
        ctx->ncu_device = ctx->ncu;
    }
    return ctx->ncu;
}

// The context's planes ze0 .. ze0 + g.Z - 1 as bit planes (bitplane_kernels.h) from the
// records: `occ` = occupied, or what the closure calls occupied; `unseen` (may be null) = the
// voxels whose colour is UNSEEN_COLOR.
static int launch_bit_pack(Ctx *ctx, const arvx::BitGrid &g, int closure_occupied, int apply_unseen,
                           unsigned long long *occ, unsigned long long *unseen) {
    if (int rc = need_rec(ctx, true)) return rc;  // (bitgrid_from_rec_kernel reads lazy tiles)
    return launch(ctx, arvx::bitgrid_from_rec_kernel, blocks_for(bit_words(g)), 256, record_params(ctx), 0, g.Z,
                  closure_occupied, apply_unseen, closure_occupied ? paint_plane(ctx) : nullptr, occ, unseen);
}

// counts the set bits per block and scans the counts; *total = number of set bits
static int bit_compact_count(Ctx *ctx, const unsigned long long *bits, size_t nwords, int *d_cnt,
                             long long *d_off, long long *total) {
    const int nblk = (int)((nwords + arvx::kBitBlock - 1) / arvx::kBitBlock);
    ARVX_TRY(launch(ctx, arvx::bit_count_kernel, nblk, 256, bits, nwords, d_cnt));
    ARVX_TRY(launch(ctx, arvx::surface_scan_kernel, 1, 256, d_cnt, nblk, d_off));
    ARVX_HIP(hipMemcpyAsync(total, d_off + nblk, sizeof *total, hipMemcpyDeviceToHost,
                            ctx->stream));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

// the control block of the one-launch compaction / scan kernels: ticket counter, device totals,
// `nchunks` status words; *status (may be null): where they start
static constexpr size_t kCompactStatus = 128;  // [0] ticket counter, [8 + 8 k] device totals, then the status words
static int compact_control(Ctx *ctx, size_t nchunks, unsigned long long **status) {
    // (room for the longest array a context ever compacts or scans -- one entry per voxel, a chunk per
    // 4096 of them --, so that the block never moves between the launches of a call: the kernels of
    // a call read each other's totals from it)
    const size_t most = ctx->nvox_ext / 4096 + 4096;
    const size_t need = kCompactStatus + std::max(nchunks, most) * sizeof(unsigned long long) + 64;
    if (ctx->pool_compact.cap < need) {
        ARVX_HIP(ctx->pool_compact.reserve(need));
        ARVX_HIP(hipMemsetAsync(ctx->pool_compact.p, 0, ctx->pool_compact.cap, ctx->stream));
        ctx->compact_tickets = 0;
        ctx->compact_epoch = 0;
    }
    if (++ctx->compact_epoch == 0u) {  // (2^32 launches: start the tags over on clean memory)
        ARVX_HIP(hipMemsetAsync(ctx->pool_compact.p, 0, ctx->pool_compact.cap, ctx->stream));
        ctx->compact_tickets = 0;
        ctx->compact_epoch = 1u;
    }
    if (status) *status = (unsigned long long *)((uint8_t *)ctx->pool_compact.p + kCompactStatus);
    return ARVX_OK;
}

// the device's copy of a list length in that control block (words below Ctx::kDeviceTotals)
static long long *device_total(const Ctx *ctx, Ctx::Word w) {
    static_assert(8 + 8 * Ctx::kDeviceTotals <= kCompactStatus, "the device totals end before the status words");
    return (long long *)((uint8_t *)ctx->pool_compact.p + 8 + 8 * (int)w);
}

// Exclusive scan of n counts in ONE launch (scan_lookback_kernel): offsets[i]; the sum goes to device
// word *d_total_out and to the count word w.  cells: the counts are the triangles of the
// marching-cubes cells of that list (n: its capacity, *n_dev: its length), not an array.
static int scan_counts(Ctx *ctx, const int *counts, const int4 *cells, long long n, const long long *n_dev,
                       int *d_offsets, Ctx::Word w, const long long **d_total_out) {
    const size_t nchunks = (size_t)((n + arvx::kScanChunk - 1) / arvx::kScanChunk);
    unsigned long long *status = nullptr;
    if (int rc = compact_control(ctx, nchunks, &status)) return rc;
    unsigned *tickets = (unsigned *)ctx->pool_compact.p;
    long long *d_total = device_total(ctx, w);
    ctx->word(w) = -1;
    if (cells) {
        const int8_t *table = nullptr;  // (the triangle counts of Bourke's table, on the device)
        ARVX_HIP(hipGetSymbolAddress((void **)&table, HIP_SYMBOL(arvx::kMcTri)));
        table += offsetof(arvx::McTriTable, n);
        ARVX_TRY(launch(ctx, arvx::scan_lookback_kernel<true>, (unsigned)nchunks, 256, (const int *)cells, table,
                        n, n_dev, d_offsets, tickets, (unsigned)ctx->compact_tickets, status,
                        ctx->compact_epoch, d_total, ctx->word_dev(w), ctx->d_fault));
    } else {
        ARVX_TRY(launch(ctx, arvx::scan_lookback_kernel<false>, (unsigned)nchunks, 256, counts, nullptr, n,
                        nullptr, d_offsets, tickets, (unsigned)ctx->compact_tickets, status,
                        ctx->compact_epoch, d_total, ctx->word_dev(w), ctx->d_fault));
    }
    ctx->compact_tickets += nchunks;
    if (d_total_out) *d_total_out = d_total;
    return ARVX_OK;
}

// The ordered compaction in ONE launch (bit_compact_counted_kernel) of a plane whose producer left the
// set bits of every chunk of kBitChunk words in `counts`: up to `cap` entries of the list go to d_index,
// every word's SparseWord to d_words; the list's true length is left in device word *d_total_out (for
// the kernels that follow) and in the count word w, which the caller reads after its synchronisation.
static int bit_compact(Ctx *ctx, const unsigned long long *bits, size_t nwords, const arvx::BitGrid &g,
                       long long cap, int *d_index, arvx::SparseWord *d_words, Ctx::Word w,
                       const long long **d_total_out) {
    const size_t nchunks = (nwords + arvx::kBitChunk - 1) / arvx::kBitChunk;
    if (int rc = compact_control(ctx, 0, nullptr)) return rc;  // (the device totals live there)
    long long *d_total = device_total(ctx, w);
    ctx->word(w) = -1;
    // the counts the producer has just left in buffer `counts_cur`; the other buffer is cleared for
    // the next producer on the way
    int *cur = (int *)ctx->pool_chunk_counts.p + (size_t)ctx->counts_cur * ctx->counts_stride;
    int *other = (int *)ctx->pool_chunk_counts.p + (size_t)(ctx->counts_cur ^ 1) * ctx->counts_stride;
    ARVX_TRY(launch(ctx, arvx::bit_compact_counted_kernel, (unsigned)nchunks, 256, bits, nwords, g, cur,
                    other, cap, d_index, d_words, d_total, ctx->word_dev(w)));
    // (it clears one entry per chunk of THIS plane: a buffer that a longer plane's producer added into
    // -- the refined mesh's edge plane has three bits per lattice point -- stays marked for a fill)
    ctx->counts_clean[ctx->counts_cur ^ 1] = ctx->counts_used[ctx->counts_cur ^ 1] <= nchunks;
    if (d_total_out) *d_total_out = d_total;
    return ARVX_OK;
}
// The count buffer the NEXT plane's producer adds into (zeroed): the two buffers take turns -- the
// compaction that reads one clears the other --, so a call costs no fill launch of its own.
static int chunk_counts(Ctx *ctx, size_t nwords, int **counts) {
    const size_t n = (nwords + arvx::kBitChunk - 1) / arvx::kBitChunk;
    if (ctx->counts_stride < n || !ctx->pool_chunk_counts.p) {
        ARVX_HIP(ctx->pool_chunk_counts.reserve(2 * n * sizeof(int)));
        ctx->counts_stride = n;
        ctx->counts_clean[0] = ctx->counts_clean[1] = false;
    }
    const int k = ctx->counts_cur ^ 1;
    int *buf = (int *)ctx->pool_chunk_counts.p + (size_t)k * ctx->counts_stride;
    if (!ctx->counts_clean[k])  // (first use, or a call that failed between producer and compaction)
        ARVX_HIP(hipMemsetAsync(buf, 0, ctx->counts_stride * sizeof(int), ctx->stream));
    ctx->counts_clean[k] = false;  // the producer is about to add into it
    ctx->counts_used[k] = n;
    ctx->counts_cur = k;
    *counts = buf;
    return ARVX_OK;
}

// The total a one-launch compaction / scan left for the host (after the call's synchronisation).  The
// kernel stores it into the page-locked word; should the host not see that store, the device's own
// copy of the word is fetched instead (-1: neither holds a count).
static long long host_total(Ctx *ctx, Ctx::Word w) {
    const long long t = ctx->word(w);
    if (t >= 0 || !ctx->pool_compact.p) return t;
    // never expected since the word is allocated coherent (EXPERIMENTS.md round 4): counted, so that
    // a recurrence shows (arvx_get_stats: host_total_fallbacks; the list tests assert 0)
    ++ctx->host_total_fallbacks;
    long long dev = -1;
    if (hipMemcpy(&dev, device_total(ctx, w), sizeof dev, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    return dev;
}

// ---- lists of unknown length: sized, launched, read, retried once -----------------------------

// Room for a list of `entry`-byte entries before its length is known: what its pool held for the
// last call, or -- the first call -- `first`: for the lists of surface voxels, a surface's share of
// v voxels and never more than `most` entries.
static long long list_cap(const arvx::DevPool &pool, size_t entry, long long first) {
    return pool.cap >= entry ? (long long)(pool.cap / entry) : first;
}
static long long first_list_cap(double v, double most) {
    return (long long)std::min<double>(most, 8.0 * std::cbrt(v) * std::cbrt(v) + 4096.0);
}

// Room for the large footprints of a splat over n entries, of which `all` exist at most: what the
// last call wanted to list and an eighth more, at least a quarter of the entries and 64 Ki more.
// What does not fit is swept by the splat's own waves: the room changes the time, never the result.
static unsigned large_list_cap(long long n, long long need, long long all) {
    const long long want = std::max((1ll << 16) + n / 4, need + need / 8);
    return (unsigned)std::min<long long>({all, want, (long long)UINT32_MAX});
}

// One list of such a call: the count word its length comes back in, its room, its length.
struct ListRoom {
    Ctx::Word word;
    long long cap, total;
};
struct NoSettle {
    int operator()() const { return ARVX_OK; }
};

// The protocol: enqueue() reserves and launches everything at the lists' capacities; ONE
// synchronisation; every list's length is read; settle() reads what else the kernels left; lists
// that outgrew their room get an eighth more than they need and the call's launches run once more.
// Never a third time: the second attempt had room for all.
template <size_t N, class Enqueue, class Settle = NoSettle>
static int run_lists(Ctx *ctx, ListRoom (&lists)[N], Enqueue enqueue, Settle settle = {}) {
    for (int attempt = 0;; ++attempt) {
        if (int rc = enqueue()) return rc;
        ARVX_SYNC(ctx);
        bool fits = true, counted = true;
        for (ListRoom &l : lists) {
            l.total = host_total(ctx, l.word);
            counted = counted && l.total >= 0;
            fits = fits && l.total <= l.cap;
        }
        if (!counted) return fail(ARVX_ERR_HIP, "a list's kernels left no count");
        if (int rc = settle()) return rc;
        if (fits || attempt) return ARVX_OK;
        for (ListRoom &l : lists)
            if (l.total > l.cap) l.cap = l.total + l.total / 8;
    }
}

// The mesh's lists {cells, triangles, ...}: with too few cells the triangle count is of the cells
// that fitted -- five per missing cell at most.  The meshes' settle hook: it runs before the lists grow.
static int room_for_missing_cells(const ListRoom &cells, ListRoom &tris) {
    if (cells.total > cells.cap) tris.cap = std::max(tris.cap, tris.total + 5 * (cells.total - cells.cap));
    return ARVX_OK;
}

// f(std::true_type) or f(std::false_type) by the context's grouping: the kernels take it as a
// template argument, `kernel<decltype(left)::value>`; f's return value (that of its launch) comes back
template <class F>
[[nodiscard]] static int by_assoc(const Ctx *ctx, F f) {
    return ctx->assoc == ARVX_ASSOC_LEFT ? f(std::true_type{}) : f(std::false_type{});
}

static int bit_compact_write(Ctx *ctx, const unsigned long long *bits, size_t nwords,
                             const arvx::BitGrid &g, const long long *d_off, int *d_index,
                             arvx::SparseWord *d_words) {
    const int nblk = (int)((nwords + arvx::kBitBlock - 1) / arvx::kBitBlock);
    return launch(ctx, arvx::bit_write_kernel, nblk, 256, bits, nwords, g, d_off, d_index, d_words);
}

// xyz -> device, kernel, results back: the two projection self-tests share this frame
template <class Enqueue>
static int selftest_xyz(Ctx *ctx, int64_t n, const int32_t *xyz, size_t out_floats, float *out,
                        Enqueue enqueue) {
    if (n < 1 || !xyz || !out) return fail(ARVX_ERR_INVALID, "bad argument");
    const size_t in_bytes = (size_t)n * 3 * sizeof(int32_t);
    ARVX_HIP(ctx->pool_scratch.reserve(in_bytes + out_floats * sizeof(float) + 64));
    int *d_xyz = (int *)ctx->pool_scratch.p;
    float *d_out = (float *)((uint8_t *)ctx->pool_scratch.p + ((in_bytes + 15) & ~(size_t)15));
    ARVX_HIP(hipMemcpyAsync(d_xyz, xyz, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    ARVX_TRY(enqueue(d_xyz, d_out));
    ARVX_HIP(hipMemcpyAsync(out, d_out, out_floats * sizeof(float), hipMemcpyDeviceToHost,
                            ctx->stream));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

extern "C" {

int arvx_version(void) { return ARVX_VERSION; }

const char *arvx_last_error(void) { return g_last_error.c_str(); }

int arvx_projection_assoc(void) { return g_default_assoc.load(); }

int arvx_set_projection_assoc(int assoc) {
    if (assoc != ARVX_ASSOC_RIGHT && assoc != ARVX_ASSOC_LEFT)
        return fail(ARVX_ERR_INVALID, "grouping %d (ARVX_ASSOC_RIGHT or ARVX_ASSOC_LEFT)", assoc);
    g_default_assoc.store(assoc);
    return ARVX_OK;
}

int arvx_ctx_set_projection_assoc(arvx_ctx *ctx, int assoc) {
    if (!ctx) return fail(ARVX_ERR_INVALID, "null context");
    if (assoc != ARVX_ASSOC_RIGHT && assoc != ARVX_ASSOC_LEFT)
        return fail(ARVX_ERR_INVALID, "grouping %d (ARVX_ASSOC_RIGHT or ARVX_ASSOC_LEFT)", assoc);
    if (ctx->assoc != assoc) ctx->drop(Event::ProjectionAssoc);  // (colours were voted with the other one)
    ctx->assoc = assoc;
    return ARVX_OK;
}

int arvx_ctx_projection_assoc(const arvx_ctx *ctx, int *assoc) {
    if (!ctx || !assoc) return fail(ARVX_ERR_INVALID, "null argument");
    *assoc = ctx->assoc;
    return ARVX_OK;
}

int arvx_device_count(int *count) {
    if (!count) return fail(ARVX_ERR_INVALID, "null count");
    *count = 0;
    ARVX_HIP(hipGetDeviceCount(count));
    return ARVX_OK;
}

int arvx_compose_projection(const float K[9], const float Rt[12], float M[12]) {
    if (!K || !Rt || !M) return fail(ARVX_ERR_INVALID, "null matrix");
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            // cv::gemm small-matrix branch: float, left to right, unfused
            float t = K[3 * r] * Rt[c];
            t = t + K[3 * r + 1] * Rt[4 + c];
            t = t + K[3 * r + 2] * Rt[8 + c];
            M[4 * r + c] = t;
        }
    return ARVX_OK;
}

int arvx_ctx_create_slab(arvx_ctx **out, int device, int X, int Y, int Z, float voxel_size,
                         int z_begin, int z_end) {
    return arvx_ctx_create_slab_halo(out, device, X, Y, Z, voxel_size, z_begin, z_end, 1);
}

int arvx_ctx_create_slab_halo(arvx_ctx **out, int device, int X, int Y, int Z, float voxel_size,
                              int z_begin, int z_end, int halo) {
    if (!out) return fail(ARVX_ERR_INVALID, "null out");
    if (halo < 1 || halo > 16) return fail(ARVX_ERR_INVALID, "halo %d (1..16 planes)", halo);
    *out = nullptr;
    if (X < 1 || Y < 1 || Z < 1) return fail(ARVX_ERR_INVALID, "grid dims must be >= 1");
    if ((int64_t)X * Y * Z > (int64_t)INT32_MAX)
        return fail(ARVX_ERR_INVALID, "X*Y*Z exceeds INT_MAX (Model::flatten returns int)");
    if (!(voxel_size > 0.f)) return fail(ARVX_ERR_INVALID, "voxel size must be > 0");
    if (z_begin < 0 || z_end > Z || z_begin >= z_end)
        return fail(ARVX_ERR_INVALID, "bad slab [%d,%d) of Z=%d", z_begin, z_end, Z);
    int ndev = 0;
    ARVX_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev)
        return fail(ARVX_ERR_INVALID, "device %d of %d", device, ndev);
    ARVX_HIP(hipSetDevice(device));
    arvx_ctx *c = new (std::nothrow) arvx_ctx();
    if (!c) return fail(ARVX_ERR_NOMEM, "out of host memory");
    c->device = device;
    c->X = X;
    c->Y = Y;
    c->Z = Z;
    c->z0 = z_begin;
    c->z1 = z_end;
    c->s = voxel_size;
    c->assoc = g_default_assoc.load();
    c->halo = halo;
    c->ze0 = z_begin - halo > 0 ? z_begin - halo : 0;
    c->ze1 = z_end + halo < Z ? z_end + halo : Z;
    c->nvox = (size_t)X * Y * (size_t)(z_end - z_begin);
    c->nvox_ext = (size_t)X * Y * (size_t)(c->ze1 - c->ze0);
    hipError_t e = acquire_stream(device, &c->own_stream);
    if (e != hipSuccess) {
        delete c;
        return arvx::fail_hip(e, "hipStreamCreate", __FILE__, __LINE__);
    }
    c->stream = c->own_stream;
    e = c->pool_stats.reserve(16 * sizeof(unsigned long long));  // 8 counters + flags
    if (e != hipSuccess) {
        arvx_ctx_destroy(c);
        return arvx::fail_hip(e, "hipMalloc(stats)", __FILE__, __LINE__);
    }
    // Coherent: without the flag a mapped allocation is non-coherent host memory -- the device's stores
    // to it need not be seen by a host that has the line in its cache (the totals' words are reset by
    // the host before every launch: a call then read its own -1 back, once in a few hundred calls)
    e = hipHostMalloc((void **)&c->h_fault, Ctx::kHostBlockBytes, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) {  // (the fault word, then the count words: arvx_ctx.h)
        memset(c->h_fault, 0, Ctx::kHostBlockBytes);
        e = hipHostGetDevicePointer((void **)&c->d_fault, c->h_fault, 0);
    }
    if (e != hipSuccess) {
        arvx_ctx_destroy(c);
        return arvx::fail_hip(e, "hipHostMalloc(fault word)", __FILE__, __LINE__);
    }
    e = hipMemsetAsync(c->stats(), 0, 64, c->stream);
    if (e != hipSuccess) {
        arvx_ctx_destroy(c);
        return arvx::fail_hip(e, "hipMemsetAsync", __FILE__, __LINE__);
    }
    *out = c;
    return ARVX_OK;
}

int arvx_ctx_create_striped(arvx_ctx **out, int device, int X, int Y, int Z, float voxel_size,
                            int world, int rank) {
    if (!out) return fail(ARVX_ERR_INVALID, "null out");
    *out = nullptr;
    if (world < 1 || rank < 0 || rank >= world)
        return fail(ARVX_ERR_INVALID, "rank %d of world %d", rank, world);
    if (Z < 1 || Z % 8) return fail(ARVX_ERR_INVALID, "striped slabs need Z %% 8 == 0 (Z=%d)", Z);
    const int groups = Z / 8;
    const int mine = (groups - rank + world - 1) / world;  // groups rank, rank+world, ...
    if (mine < 1) return fail(ARVX_ERR_INVALID, "rank %d owns no planes (Z=%d)", rank, Z);
    // build it as a contiguous context of mine*8 planes, then switch the z mapping
    int rc = arvx_ctx_create_slab(out, device, X, Y, Z, voxel_size, 0, mine * 8);
    if (rc) return rc;
    arvx_ctx *c = *out;
    c->ze0 = 0;  // no halo planes: neighbours in z belong to other ranks
    c->ze1 = mine * 8;
    c->nvox_ext = c->nvox;
    c->stripe_world = world;
    c->stripe_rank = rank;
    return ARVX_OK;
}

int arvx_ctx_create(arvx_ctx **out, int device, int X, int Y, int Z, float voxel_size) {
    return arvx_ctx_create_slab(out, device, X, Y, Z, voxel_size, 0, Z);
}

int arvx_ctx_destroy(arvx_ctx *ctx) {
    if (!ctx) return ARVX_OK;
    const int device = ctx->device;
    const hipStream_t own = ctx->own_stream;
    (void)hipSetDevice(device);
    if (own) (void)hipStreamSynchronize(own);
    delete ctx;  // (its members free every buffer it holds)
    if (own) {
        (void)hipStreamSynchronize(own);
        release_stream(device, own);
    }
    return ARVX_OK;
}

int arvx_ctx_set_stream(arvx_ctx *ctx, void *hip_stream) {
    ARVX_CHECK_CTX(ctx);
    ARVX_SYNC(ctx);
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    // the carve's alternating list counters are zeroed by the PREVIOUS carve in stream order:
    // on another stream they start over (launch_carve zeroes both when the layout is unset)
    ctx->carve_layout = 0;
    return ARVX_OK;
}

int arvx_ctx_set_exchange_stream(arvx_ctx *ctx, void *hip_stream) {
    ARVX_CHECK_CTX(ctx);
    ctx->xstream = (hipStream_t)hip_stream;
    return ARVX_OK;
}

#ifdef ARVX_EXPERIMENTS
// Experiment builds only (tests/test_fault_gpu.py): leave the mark a kernel leaves when it gives up
// waiting for another workgroup, as if the launches since the last synchronisation had done so.
extern "C" int arvx_experiment_mark_fault(arvx_ctx *ctx, unsigned mark) {
    if (!ctx || !ctx->h_fault) return fail(ARVX_ERR_INVALID, "null context");
    *ctx->h_fault = mark;
    return ARVX_OK;
}
#endif

int arvx_ctx_synchronize(arvx_ctx *ctx) {
    ARVX_CHECK_CTX(ctx);
    ARVX_HIP(hipStreamSynchronize(ctx->stream));
    return check_fault(ctx);
}

int arvx_ctx_voxels(const arvx_ctx *ctx, int64_t *count) {
    if (!ctx || !count) return fail(ARVX_ERR_INVALID, "null argument");
    *count = (int64_t)ctx->nvox;
    return ARVX_OK;
}

// ---- views -------------------------------------------------------------------

// The WINDOW of a view: the part of its summed-area table that a rectangle test of a box of voxels
// of the grid X x Y x Z (voxel indices 0 .. X-1, 0 .. Y-1, global z 0 .. Z-1: every slab, halo
// plane and stripe, and the coarse boxes of striped slabs that span foreign planes) can read.
// Host arithmetic in double; it depends on the matrix, the image size, the voxel size and the grid,
// not on the masks.
//
// rect_prepare (carve_kernels.h) clamps nothing: for a box it returns the pixel rectangle
//   [ceil(umin - mu - 1/2), floor(umax + mu + 1/2)] x [ceil(vmin - mv - 1/2), floor(vmax + mv + 1/2)]
// with umin .. vmax taken over the fp32 quotients at the box's eight corners, and reads the table
// (code < 0) only when that rectangle lies inside the image; it then reads the entries
// (pylo .. pyhi + 1, pxlo .. pxhi + 1).
//  (1) A sub-box's corners w = fl32(i * s) lie inside the grid's box (rounding is monotone).  The
//      rows a_r are affine in w and u = a_0 / a_2 is linear-fractional, so where a_2 keeps its sign
//      over the grid's box the REAL u at every corner of every sub-box lies between the smallest
//      and the largest real u at the grid's eight corners, [Umin, Umax].
//  (2) A sub-box's COMPUTED corner quotient differs from the real one by at most
//        errU = (eps_0 + Ua eps_2) / (cabs - 2 eps_2) + 2^-20 Ua + 2^-12
//      (the error budget written at classify_box) with eps_r = 2^-19 E_r, E_r = sum_k |M[r][k]| max
//      |w_k| over the GRID (a sub-box's is not larger), Ua = max |U| over the grid's corners and
//      cabs = min |a_2| over the grid's corners: a sub-box's computed |a_2| is at least cabs - eps_2
//      and the budget divides by that less eps_2.
//  (3) A sub-box's margin mu is the same expression in its own fp32 quantities, times 1.0001:
//      bounded by mu = 1.001 (eps_0 + Ua' eps_2) / (cabs - 2 eps_2) + 2^-20 Ua' + 2^-12 with
//      Ua' = Ua + errU.  (eps_r carries a factor 1.001 here for the fp32 roundings of E_r.)
//  (4) So every rectangle lies in [Umin - errU - mu - 1/2, Umax + errU + mu + 1/2]; one whole pixel
//      is added on each side for what fp32 does to these sums and roundings (|u| < 10^6: an fp32
//      sum is off by less than 1/8), and +1 on the high side for the table's border.
//  (5) The result is clipped to the table and rounded outwards to the tiles of views_strip_kernel:
//      strip I = (table row - 1) / 64 (row 0 is written by strip 0), tile column J = column / 64.
// The view takes the whole table when a_2 changes sign over the grid or comes within 16 eps_2 of
// zero (cameras inside or at the grid: the argument of (1) and the divisor of (2) need more), or
// when |u| or |v| reaches 10^6 at a corner.
// win: {I0, I1, J0, J1}, inclusive.  Returns whether the window is the whole table.
static bool view_window(int X, int Y, int Z, float s, const float *M, int W, int H, int win[4]) {
    const int TI = (H + 63) / 64, JL = W / 64;  // last tile column: that of table column W
    win[0] = 0;
    win[1] = TI - 1;
    win[2] = 0;
    win[3] = JL;
    // the grid's box as make_box forms it
    const double wy[2] = {0.0, (double)((float)(Y - 1) * s)};
    const double wx[2] = {0.0, (double)((float)(X - 1) * s)};
    const double wz[2] = {0.0, (double)((float)(-(Z - 1)) * s)};
    double E[3], lo[3], hi[3];
    double a[3][8];
    for (int r = 0; r < 3; ++r) {
        const double m0 = M[4 * r], m1 = M[4 * r + 1], m2 = M[4 * r + 2], m3 = M[4 * r + 3];
        E[r] = std::fabs(m0) * std::fabs(wy[1]) + std::fabs(m1) * std::fabs(wx[1]) +
               std::fabs(m2) * std::fabs(wz[1]) + std::fabs(m3);
        for (int c = 0; c < 8; ++c) a[r][c] = m0 * wy[c & 1] + m1 * wx[(c >> 1) & 1] + m2 * wz[c >> 2] + m3;
    }
    double cmin = INFINITY, cmax = -INFINITY;
    for (int c = 0; c < 8; ++c) {
        cmin = std::fmin(cmin, a[2][c]);
        cmax = std::fmax(cmax, a[2][c]);
    }
    const double k19 = 1.001 / 524288.0, k20 = 1.0 / 1048576.0, k12 = 1.0 / 4096.0;
    const double eps0 = E[0] * k19, eps1 = E[1] * k19, eps2 = E[2] * k19;
    if (!(cmin > 0.0 || cmax < 0.0)) return true;  // a_2 changes sign (also NaN)
    const double cabs = cmin > 0.0 ? cmin : -cmax;
    if (!(cabs > 16.0 * eps2 + 1e-30)) return true;
    const double D = cabs - 2.0 * eps2;
    for (int r = 0; r < 2; ++r) {
        lo[r] = INFINITY;
        hi[r] = -INFINITY;
        for (int c = 0; c < 8; ++c) {
            const double u = a[r][c] / a[2][c];
            lo[r] = std::fmin(lo[r], u);
            hi[r] = std::fmax(hi[r], u);
        }
    }
    int t0[2], t1[2];  // table columns / rows, inclusive
    for (int r = 0; r < 2; ++r) {
        const double Ua = std::fmax(std::fabs(lo[r]), std::fabs(hi[r]));
        if (!(Ua < 1.0e6)) return true;  // also NaN
        const double epsr = r == 0 ? eps0 : eps1;
        const double err = (epsr + Ua * eps2) / D + Ua * k20 + k12;
        const double Ub = Ua + err;
        const double mu = 1.001 * (epsr + Ub * eps2) / D + Ub * k20 + k12;
        const double n = r == 0 ? (double)W : (double)H;
        double l = std::floor(lo[r] - err - mu - 0.5) - 1.0;
        double h = std::ceil(hi[r] + err + mu + 0.5) + 1.0 + 1.0;  // slack, then the border
        if (!(l == l && h == h)) return true;
        l = std::fmin(std::fmax(l, 0.0), n);  // (entries 0 .. n of the table)
        h = std::fmin(std::fmax(h, l), n);
        t0[r] = (int)l;
        t1[r] = (int)h;
    }
    win[2] = t0[0] / 64;
    win[3] = t1[0] / 64;
    win[0] = t0[1] <= 1 ? 0 : (t0[1] - 1) / 64;
    win[1] = t1[1] <= 1 ? 0 : (t1[1] - 1) / 64;
    return win[0] == 0 && win[1] == TI - 1 && win[2] == 0 && win[3] == JL;
}
static uint32_t window_word(const int win[4]) {
    return (uint32_t)win[0] | ((uint32_t)win[1] << 8) | ((uint32_t)win[2] << 16) | ((uint32_t)win[3] << 24);
}
// the table rows and columns (inclusive) that the tiles of a window word cover
static void window_rect(uint32_t w, int H, int satW, int rect[4]) {
    const int I0 = (int)(w & 0xffu), I1 = (int)((w >> 8) & 0xffu), J0 = (int)((w >> 16) & 0xffu), J1 = (int)(w >> 24);
    rect[0] = I0 == 0 ? 0 : 64 * I0 + 1;
    rect[1] = std::min(H, 64 * (I1 + 1));
    rect[2] = 64 * J0;
    rect[3] = std::min(satW - 1, 64 * J1 + 63);
}

int arvx_view_window_host(int X, int Y, int Z, float voxel_size, const float M[12], int W, int H,
                          int rect[4]) {
    if (!M || !rect) return fail(ARVX_ERR_INVALID, "null argument");
    if (X < 1 || Y < 1 || Z < 1 || !(voxel_size > 0.f)) return fail(ARVX_ERR_INVALID, "bad grid");
    if (W < 1 || H < 1 || W > arvx::kMaxImageDim || H > arvx::kMaxImageDim)
        return fail(ARVX_ERR_INVALID, "image size %dx%d out of range", W, H);
    int win[4];
    view_window(X, Y, Z, voxel_size, M, W, H, win);
    window_rect(window_word(win), H, (W + 1 + 63) / 64 * 64, rect);
    return ARVX_OK;
}

// The window words of the next derivation, on the device: those of the cameras where the strip
// kernel runs with windows (strip), the whole table everywhere else.  Sent only when one differs
// from what the device holds.
static int views_windows(Ctx *ctx, bool strip) {
    const int V = ctx->V;
    if (!ctx->win_valid) {
        ctx->h_win_geo.resize(V);
        for (int v = 0; v < V; ++v) {
            int win[4];
            view_window(ctx->X, ctx->Y, ctx->Z, ctx->s, ctx->h_M.data() + 12 * (size_t)v, ctx->W, ctx->H, win);
            ctx->h_win_geo[v] = window_word(win);
        }
        ctx->win_valid = true;
    }
    const int whole[4] = {0, (ctx->H + 63) / 64 - 1, 0, ctx->W / 64};
    const uint32_t all = window_word(whole);
    const bool geo = strip && ctx->win_on;
    bool same = ctx->h_win.size() == (size_t)V && ctx->pool_win.cap >= (size_t)V * sizeof(uint32_t);
    ctx->sat_partial = false;
    for (int v = 0; v < V; ++v) {
        const uint32_t w = geo ? ctx->h_win_geo[v] : all;
        if (w != all) ctx->sat_partial = true;
        same = same && ctx->h_win[v] == w;
    }
    if (!same) {
        ARVX_HIP(ctx->pool_win.reserve((size_t)V * sizeof(uint32_t)));
        if (geo)
            ctx->h_win = ctx->h_win_geo;
        else
            ctx->h_win.assign(V, all);
        ARVX_HIP(hipMemcpyAsync(ctx->pool_win.p, ctx->h_win.data(), (size_t)V * sizeof(uint32_t),
                                hipMemcpyHostToDevice, ctx->stream));
    }
    return ARVX_OK;
}

static int views_common(Ctx *ctx, int V, const float *M, const float *campos, int W, int H,
                        int C) {
    if (V < 1 || V > 4096) return fail(ARVX_ERR_INVALID, "V=%d out of range [1,4096]", V);
    if (!M) return fail(ARVX_ERR_INVALID, "null M");
    if (W < 1 || H < 1 || W > arvx::kMaxImageDim || H > arvx::kMaxImageDim)
        return fail(ARVX_ERR_INVALID, "image size %dx%d out of range", W, H);
    if (C < 1 || C > 4) return fail(ARVX_ERR_INVALID, "channels=%d out of range [1,4]", C);
    // the same number and size of views as before: keep every buffer (a pipeline sends its
    // views once per stage, src/main.cpp:262-284)
    const bool same = ctx->M() && ctx->V == V && ctx->W == W && ctx->H == H;
    ctx->drop(Event::SetViews);  // colour results belong to the previous views
    ctx->views_ready = false;
    ctx->cameras_ready = false;
    ctx->seg_ready = false;  // (arvx_segment_views sets it again once its masks are the views)
    if (!same) {
        ctx->free_views();
        ctx->pool_images.release();
    }
    ctx->images_ready = false;
    ctx->V = V;
    ctx->W = W;
    ctx->H = H;
    // one word more than the pixels need: bit 32 * (bgWords - 1) is a background bit that is
    // always 0, which the block-mapped exact kernel reads for voxels outside the image
    // (padded to whole 128-byte lines per view: views_strip_kernel writes a view's plane as
    // aligned 8-byte words and whole lines; only the last word is ever read as "always zero")
    ctx->bgWords = (int)(((((size_t)W * H + 31) / 32 + 1) + 31) / 32 * 32);
    // summed-area table (views_kernels.h): (H + 1) rows of W + 1 entries, the rows padded to
    // whole 128-byte lines so that the table kernel's stores are line-aligned
    ctx->satW = (W + 1 + 63) / 64 * 64;  // (two-byte entries: 64 per 128-byte line)
    ctx->satH = H + 1;
    ctx->satStride = ctx->satW * ctx->satH;
    if (!same) {
        hipError_t e = ctx->pool_M.reserve((size_t)V * 12 * sizeof(float));
        if (e == hipSuccess) e = ctx->pool_campos.reserve((size_t)V * 3 * sizeof(float));
        if (e == hipSuccess) e = ctx->pool_bg.reserve((size_t)V * ctx->bgWords * sizeof(uint32_t));
        if (e == hipSuccess) e = ctx->pool_sat.reserve((size_t)V * ctx->satStride * sizeof(uint16_t));
        if (e != hipSuccess) {
            ctx->free_views();  // whatever was allocated before the failure
            return arvx::fail_hip(e, "hipMalloc(views)", __FILE__, __LINE__);
        }
    }
    // matrices and camera positions: sent only when they differ from what the device holds
    // (a pipeline re-derives its views per batch of masks with the same cameras; the two
    // small copies cost more than a kernel of the step each)
    const bool same_M = same && ctx->h_M.size() == (size_t)V * 12 &&
                        memcmp(ctx->h_M.data(), M, (size_t)V * 12 * sizeof(float)) == 0;
    if (!same_M) {
        ctx->rect_invalidate();  // (the cached rectangles are those of the matrices before)
        ctx->h_M.assign(M, M + (size_t)V * 12);
        ARVX_HIP(hipMemcpyAsync(ctx->M(), ctx->h_M.data(), (size_t)V * 12 * sizeof(float),
                                hipMemcpyHostToDevice, ctx->stream));
    }
    ctx->has_campos = campos != nullptr;
    if (campos) {
        const bool same_c = same && ctx->h_campos.size() == (size_t)V * 3 &&
                            memcmp(ctx->h_campos.data(), campos, (size_t)V * 3 * sizeof(float)) == 0;
        if (!same_c) {
            ctx->h_campos.assign(campos, campos + (size_t)V * 3);
            ARVX_HIP(hipMemcpyAsync(ctx->campos(), ctx->h_campos.data(),
                                    (size_t)V * 3 * sizeof(float), hipMemcpyHostToDevice,
                                    ctx->stream));
        }
    } else {
        ctx->h_campos.clear();
    }
    return ARVX_OK;
}

static int views_tables_from_bits(Ctx *ctx);
static int views_preprocess(Ctx *ctx, const uint8_t *d_masks, int C) {
    const int npix = ctx->W * ctx->H;
    ARVX_HIP(hipGetLastError());  // anything stale would be blamed on the launches below
    // one- or three-channel masks with rows of whole 64-pixel tiles: ONE launch, a workgroup per strip
    // of 64 rows (views_kernels.h, views_strip_kernel); every other format: the three launches below
    static const bool three_launches = experiment_flag("ARVX_VIEWS_THREE_LAUNCHES");
    if ((C == 1 || C == 3) && ctx->W % 64 == 0 && ctx->W / 64 + 1 <= arvx::kStripMaxWaves && ctx->H <= 4096 &&
        ((uintptr_t)d_masks & 15u) == 0 && !three_launches) {
        const int TIs = (ctx->H + 63) / 64;
        // ticket counters (one per view, never reset) + the strips' published column counts;
        // zeroed once per layout (the tickets count launches from there)
        const size_t G = (size_t)ctx->W / 2;
        const size_t off_gran = ((size_t)ctx->V * sizeof(unsigned long long) + 255) / 256 * 256;
        const size_t vbytes = off_gran + (size_t)ctx->V * TIs * G * sizeof(unsigned long long);
        const size_t key = ((size_t)ctx->V << 40) ^ ((size_t)TIs << 24) ^ G;
        if (ctx->vstrip_key != key || ctx->pool_vstrip.cap < vbytes) {
            ARVX_HIP(ctx->pool_vstrip.reserve(vbytes));
            ARVX_HIP(hipMemsetAsync(ctx->pool_vstrip.p, 0, vbytes, ctx->stream));
            ctx->vstrip_key = key;
        }
        unsigned long long *ctr = (unsigned long long *)ctx->pool_vstrip.p;
        unsigned long long *gran = (unsigned long long *)((uint8_t *)ctx->pool_vstrip.p + off_gran);
        // the table's tiles outside a view's window stay unwritten (view_window, above)
        if (int rc = views_windows(ctx, true)) return rc;
        const uint32_t *win = (const uint32_t *)ctx->pool_win.p;
        ARVX_TRY(launch(ctx, C == 1 ? arvx::views_strip_kernel<1> : arvx::views_strip_kernel<3>,
                        dim3(TIs, ctx->V), 64 * (ctx->W / 64 + 1), d_masks, ctx->W, ctx->H, TIs, ctx->bg(),
                        ctx->bgWords, ctx->sat(), ctx->satStride, ctx->satW, ctr, gran, ctx->d_fault, win));
        ctx->views_ready = true;
        ctx->cameras_ready = true;
        return ARVX_OK;
    }
    // (the three launches write whole tables: the windows on record are "everything")
    if (int rc = views_windows(ctx, false)) return rc;
    if (C == 1 && npix % 32 == 0 && ((uintptr_t)d_masks & 15u) == 0) {
        ARVX_TRY(launch(ctx, arvx::views_bits16_kernel, dim3((npix / 16 + 255) / 256, ctx->V), 256, d_masks,
                        npix, ctx->bg(), ctx->bgWords));
    } else if (C == 1 || C == 3) {
        const dim3 g1(((npix + 3) / 4 + 255) / 256, ctx->V);
        ARVX_TRY(launch(ctx, C == 1 ? arvx::views_bits_kernel<1> : arvx::views_bits_kernel<3>, g1, 256, d_masks,
                        npix, ctx->bg(), ctx->bgWords));
    } else {
        const dim3 g1((npix + 255) / 256, ctx->V);
        ARVX_TRY(launch(ctx, arvx::views_bits_generic_kernel, g1, 256, d_masks, C, npix, ctx->bg(),
                        ctx->bgWords));
    }
    if (int rc = views_tables_from_bits(ctx)) return rc;
    ctx->views_ready = true;
    ctx->cameras_ready = true;
    return ARVX_OK;
}

// every view's whole summed-area table from its bit plane: two launches (views_kernels.h)
static int views_tables_from_bits(Ctx *ctx) {
    const int W = ctx->W, H = ctx->H, V = ctx->V;
    // tiles of 64 table columns x 64 image rows (views_kernels.h)
    const int TJ = (W + 1 + 63) / 64, TI = (H + arvx::kTileRows - 1) / arvx::kTileRows;
    const size_t n_rs = (size_t)V * H * TJ, n_T = (size_t)V * TI * TJ * 64, n_ts = (size_t)V * TI * TJ;
    ARVX_HIP(ctx->pool_scratch.reserve((n_rs + n_T + n_ts) * sizeof(int) + 64));
    int *d_rs = (int *)ctx->pool_scratch.p, *d_T = d_rs + n_rs, *d_ts = d_T + n_T;
    const unsigned tgrid = (unsigned)(((size_t)TJ * TI * V + 3) / 4);
    ARVX_TRY(launch(ctx, arvx::views_tile_sums_kernel, tgrid, 256, ctx->bg(), ctx->bgWords, W, H, TJ, TI, V,
                    d_rs, d_T, d_ts));
    return launch(ctx, arvx::views_table_kernel, tgrid, 256, ctx->bg(), ctx->bgWords, W, H, TJ, TI, V, d_rs,
                  d_T, d_ts, ctx->sat(), ctx->satStride, ctx->satW);
}

// Who reads the table, and why a partial one (Ctx::sat_partial) serves them: the carve kernels in
// every variant (coarse, classify, dense classify, fused, the exact kernels' block tests -- computed
// or from the cached rectangles, whose entries are rect_prepare's answers for the same boxes --,
// the streaming carve) and the vote kernel read it only through rect_prepare + rect_finish /
// classify_box / classify_block_entry, for boxes of voxels of this context's grid: inside the
// window by view_window's argument.  The brute-force carve, the colour, photo, render and mesh
// stages read the bit plane or no view data at all; the plane is always complete.  Whoever wants
// the table entry by entry (arvx_selftest_view_tables) calls this first: the two launches of the
// other mask formats write every entry from the complete bit plane -- the same absolute values --
// and the mark goes.
static int complete_tables(Ctx *ctx) {
    if (!ctx->sat_partial) return ARVX_OK;
    if (int rc = views_tables_from_bits(ctx)) return rc;
    ctx->sat_partial = false;
    return ARVX_OK;
}

int arvx_ctx_set_view_window(arvx_ctx *ctx, int on) {
    ARVX_CHECK_CTX(ctx);
    ctx->win_on = on != 0;  // (takes effect at the next arvx_set_views[_device])
    return ARVX_OK;
}

int arvx_view_window(arvx_ctx *ctx, int view, int rect[4]) {
    ARVX_CHECK_CTX(ctx);
    if (!rect) return fail(ARVX_ERR_INVALID, "null rect");
    if (!ctx->views_ready || ctx->h_win.size() != (size_t)ctx->V)
        return fail(ARVX_ERR_STATE, "arvx_set_views has not been called");
    if (view < 0 || view >= ctx->V) return fail(ARVX_ERR_INVALID, "view %d outside [0,%d)", view, ctx->V);
    window_rect(ctx->h_win[view], ctx->H, ctx->satW, rect);
    return ARVX_OK;
}

int arvx_selftest_fill_view_tables(arvx_ctx *ctx, int value) {
    ARVX_CHECK_CTX(ctx);
    if (!ctx->views_ready) return fail(ARVX_ERR_STATE, "arvx_set_views has not been called");
    ARVX_HIP(hipMemsetAsync(ctx->sat(), value & 0xff, (size_t)ctx->V * ctx->satStride * sizeof(uint16_t),
                            ctx->stream));
    ctx->views_ready = false;  // (the tables are gone: the next arvx_set_views derives them)
    return ARVX_OK;
}

int arvx_set_views(arvx_ctx *ctx, int V, const float *M, const float *campos,
                   const uint8_t *const *masks, int W, int H, int C, size_t stride) {
    ARVX_CHECK_CTX(ctx);
    if (!masks) {  // cameras only: enough for arvx_color
        if (int rc0 = views_common(ctx, V, M, campos, W, H, C > 0 ? C : 1)) return rc0;
        ctx->cameras_ready = true;
        ARVX_SYNC(ctx);
        return ARVX_OK;
    }
    if (W >= 1 && C >= 1 && stride < (size_t)W * C)
        return fail(ARVX_ERR_INVALID, "stride %zu < W*C", stride);
    for (int i = 0; i < V; ++i)
        if (!masks[i]) return fail(ARVX_ERR_INVALID, "null mask %d", i);
    int rc = views_common(ctx, V, M, campos, W, H, C);
    if (rc) return rc;
    const size_t img = (size_t)W * H * C;
    ARVX_HIP(ctx->pool_raw_masks.reserve(img * V));
    uint8_t *d_raw = (uint8_t *)ctx->pool_raw_masks.p;
    bool packed = stride == (size_t)W * C;  // all views back to back in host memory: one copy
    for (int i = 1; i < V && packed; ++i) packed = masks[i] == masks[i - 1] + img;
    if (packed) {
        ARVX_HIP(hipMemcpyAsync(d_raw, masks[0], img * V, hipMemcpyHostToDevice, ctx->stream));
    } else {
        for (int i = 0; i < V; ++i)
            ARVX_HIP(hipMemcpy2DAsync(d_raw + img * i, (size_t)W * C, masks[i], stride,
                                      (size_t)W * C, H, hipMemcpyHostToDevice, ctx->stream));
    }
    rc = views_preprocess(ctx, d_raw, C);
    if (rc) return rc;
    ARVX_SYNC(ctx);  // host buffers may go away
    return ARVX_OK;
}

int arvx_set_views_device(arvx_ctx *ctx, int V, const float *M, const float *campos,
                          const void *dev_masks, int W, int H, int C) {
    ARVX_CHECK_CTX(ctx);
    if (!dev_masks) return fail(ARVX_ERR_INVALID, "null dev_masks");
    if (int rc = views_common(ctx, V, M, campos, W, H, C)) return rc;
    return views_preprocess(ctx, (const uint8_t *)dev_masks, C);
}

static int undistort_params(const double K[9], const double *dist, int ndist, int W, int H,
                            int C, arvx::UndistortParams &p) {
    if (!K || (!dist && ndist)) return fail(ARVX_ERR_INVALID, "null calibration");
    if (ndist != 0 && ndist != 4 && ndist != 5 && ndist != 8)
        return fail(ARVX_ERR_INVALID, "distortion coefficients: 4, 5 or 8 (got %d)", ndist);
    if (W < 1 || H < 1 || C < 1 || C > 4) return fail(ARVX_ERR_INVALID, "bad image format");
    if (K[0] == 0 || K[4] == 0) return fail(ARVX_ERR_INVALID, "singular camera matrix");
    memset(&p, 0, sizeof p);
    p.fx = K[0];
    p.fy = K[4];
    p.cx = K[2];
    p.cy = K[5];
    p.ir0 = 1.0 / p.fx;  // inv(A) of an upper-triangular A with a unit last row
    p.ir2 = -p.cx / p.fx;
    p.ir4 = 1.0 / p.fy;
    p.ir5 = -p.cy / p.fy;
    double k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < ndist; ++i) k[i] = dist[i];
    p.k1 = k[0];
    p.k2 = k[1];
    p.p1 = k[2];
    p.p2 = k[3];
    p.k3 = k[4];
    p.k4 = k[5];
    p.k5 = k[6];
    p.k6 = k[7];
    p.W = W;
    p.H = H;
    p.C = C;
    return ARVX_OK;
}

int arvx_undistort_device(arvx_ctx *ctx, int V, const void *dev_src, int W, int H, int C,
                          const double K[9], const double *dist, int ndist, void *dev_dst) {
    ARVX_CHECK_CTX(ctx);
    if (!dev_src || !dev_dst || dev_src == dev_dst || V < 1)
        return fail(ARVX_ERR_INVALID, "bad argument (src and dst must differ)");
    arvx::UndistortParams p;
    if (int rc = undistort_params(K, dist, ndist, W, H, C, p)) return rc;
    return launch(ctx, arvx::undistort_kernel, dim3((W + 63) / 64, (H + 3) / 4, V), 256,
                  (const uint8_t *)dev_src, (uint8_t *)dev_dst, p);
}

int arvx_undistort(arvx_ctx *ctx, int V, const uint8_t *const *src, int W, int H, int C,
                   size_t stride, const double K[9], const double *dist, int ndist,
                   uint8_t *const *dst) {
    ARVX_CHECK_CTX(ctx);
    if (!src || !dst || V < 1) return fail(ARVX_ERR_INVALID, "bad argument");
    arvx::UndistortParams p;
    if (int rc = undistort_params(K, dist, ndist, W, H, C, p)) return rc;
    const size_t rowb = (size_t)W * C, img = rowb * H;
    if (stride < rowb) return fail(ARVX_ERR_INVALID, "stride %zu < W*C", stride);
    for (int i = 0; i < V; ++i)
        if (!src[i] || !dst[i]) return fail(ARVX_ERR_INVALID, "null image %d", i);
    ARVX_HIP(ctx->pool_scratch.reserve(2 * img * V + 64));
    uint8_t *d_src = (uint8_t *)ctx->pool_scratch.p, *d_dst = d_src + img * V;
    for (int i = 0; i < V; ++i)
        ARVX_HIP(hipMemcpy2DAsync(d_src + img * i, rowb, src[i], stride, rowb, H,
                                  hipMemcpyHostToDevice, ctx->stream));
    ARVX_TRY(launch(ctx, arvx::undistort_kernel, dim3((W + 63) / 64, (H + 3) / 4, V), 256, d_src, d_dst, p));
    for (int i = 0; i < V; ++i)
        ARVX_HIP(hipMemcpy2DAsync(dst[i], stride, d_dst + img * i, rowb, rowb, H,
                                  hipMemcpyDeviceToHost, ctx->stream));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

// ---- state -------------------------------------------------------------------

// grid geometry of a context as the kernels see it (planes ze0..ze1-1: owned + halo)
static void carve_geometry(const Ctx *ctx, arvx::CarveParams &p) {
    memset(&p, 0, sizeof p);
    p.X = ctx->X;
    p.Y = ctx->Y;
    p.Z = ctx->ze1 - ctx->ze0;  // owned planes plus halo (recomputed, never exchanged)
    p.zoff = ctx->ze0;
    p.zstride = ctx->stripe_world;
    p.zphase = ctx->stripe_rank;
    p.s = ctx->s;
    p.tilesX = (p.X + arvx::kTileX - 1) / arvx::kTileX;
    p.tilesY = (p.Y + arvx::kTileY - 1) / arvx::kTileY;
    p.tilesZ = (p.Z + arvx::kTileZ - 1) / arvx::kTileZ;
    // coarse tile 64x32x32; striped slabs: 64x64x8, so that it stays inside one stripe
    p.cyShift = ctx->stripe_world > 1 ? 3 : 2;
    p.czShift = ctx->stripe_world > 1 ? 0 : 2;
    p.coarseX = (p.X + arvx::kCoarseX - 1) / arvx::kCoarseX;
    p.coarseY = (p.Y + (8 << p.cyShift) - 1) / (8 << p.cyShift);
    p.coarseZ = (p.Z + (8 << p.czShift) - 1) / (8 << p.czShift);
    p.ccode = ctx->form == Form::Lazy ? (const uint8_t *)ctx->pool_ccode.p : nullptr;
}
// that geometry over the context's own records: what the stages' kernels take
static arvx::CarveParams record_params(const Ctx *ctx) {
    arvx::CarveParams p;
    carve_geometry(ctx, p);
    p.rec = ctx->rec();
    return p;
}
// the views' matrices and tables (arvx_set_views) as the carve kernels see them
static void carve_views(const Ctx *ctx, arvx::CarveParams &p) {
    p.M = ctx->M();
    p.bg = ctx->bg();
    p.sat = ctx->sat();
    p.W = ctx->W;
    p.H = ctx->H;
    p.bgWords = ctx->bgWords;
    p.satStride = ctx->satStride;
    p.satW = ctx->satW;
}

// A bit plane over the context's first nz planes (bitplane_kernels.h) put onto the records (grow) or
// taken off them.  Both kernels write records only: the caller has ended a lazy state first.
static int records_apply(Ctx *ctx, const unsigned long long *plane, int nz, bool grow) {
    return launch(ctx, grow ? arvx::rec_or_bitgrid_kernel : arvx::rec_andnot_bitgrid_kernel,
                  blocks_for(bit_words(bit_grid(ctx, nz))), 256, record_params(ctx), 0, nz, plane);
}

// a record buffer for this context's grid, every record "finished" when it is new
static int ensure_records(Ctx *ctx, arvx::DevPool &buf) {
    arvx::CarveParams g;
    carve_geometry(ctx, g);
    const size_t need = arvx::rec_count(g) * arvx::kRecU16 * sizeof(uint16_t);
    if (buf.cap >= need) return ARVX_OK;
    ARVX_HIP(buf.reserve(need));
    return launch(ctx, arvx::rec_init_kernel, 2048, 256, (uint32_t *)buf.p, need / 4);
}

// The state as records: what every stage works on.  lazy_ok: the caller's kernels read the
// coarse tiles a fresh carve settled as a whole from their codes (CarveParams::ccode); everybody
// else gets those tiles written out first -- the fill the carve itself skipped.
static int need_rec(Ctx *ctx, bool lazy_ok) {
    if (int rc = ensure_records(ctx, ctx->pool_rec)) return rc;
    if (ctx->form == Form::Records || (ctx->form == Form::Lazy && lazy_ok)) return ARVX_OK;
    arvx::CarveParams g = record_params(ctx);
    if (ctx->form == Form::Lazy) {
        g.ccode = nullptr;
        g.coarseCarved = (uint8_t *)ctx->pool_ccode.p;
        g.flags = 4u;  // codes 2 and 3 are those of a fresh model: written as such
    } else {
        g.flags = 4u | 16u;  // a fresh model: all occupied, none seen
    }
    ARVX_TRY(launch(ctx, arvx::carve_fill_kernel, (unsigned)((size_t)g.coarseX * g.coarseY * g.coarseZ), 256,
                    g));
    ctx->form = Form::Records;
    return ARVX_OK;
}

// The state holds a closure's fills but its list -- their colours -- is gone (handleUnseen, a colour
// call, new views or images since): the reference's Model would still give them their means, which
// the context no longer has.  Calls that return colours are refused then (arvx.h, arvx_closure).
static int fills_without_colours(Ctx *ctx) {
    if (ctx->closure_fills && !ctx->closure_ready)
        return fail(ARVX_ERR_STATE, "the closure's list of filled voxels is gone (handleUnseen, a colour call, "
                                    "new views or images since): upload the state and its colours again");
    return ARVX_OK;
}
// A closure's list holds the fills of one apply_unseen: calls that read it under the other are refused.
static int closure_of_other_unseen(const Ctx *ctx, int apply_unseen) {
    if (ctx->closure_ready && (apply_unseen != 0) != (ctx->closure_unseen != 0))
        return fail(ARVX_ERR_STATE, "arvx_closure was computed with apply_unseen=%d", ctx->closure_unseen);
    return ARVX_OK;
}

// Bytes of local planes [zl0, zl0 + nz), already in the staging buffer, into the records
// (+ bit2 into the paint plane).  Ends with a host synchronisation.
static int bytes_into_records(Ctx *ctx, int zl0, int nz) {
    if (int rc = need_rec(ctx)) return rc;
    arvx::CarveParams g = record_params(ctx);
    const size_t pw = (size_t)((ctx->X + 63) / 64) * ctx->Y * (size_t)(ctx->ze1 - ctx->ze0);
    const bool had = ctx->pool_paint.cap >= pw * 8 && ctx->paint_valid;
    ARVX_HIP(ctx->pool_paint.reserve(pw * 8));
    if (!had) ARVX_HIP(hipMemsetAsync(ctx->pool_paint.p, 0, pw * 8, ctx->stream));
    int *d_any = (int *)(ctx->stats() + 8);
    ARVX_HIP(hipMemsetAsync(d_any, 0, sizeof(int), ctx->stream));
    ARVX_TRY(launch(ctx, arvx::rec_from_bytes_kernel, (unsigned)((size_t)g.tilesX * g.tilesY * g.tilesZ), 256,
                    g, (const uint8_t *)ctx->pool_state_bytes.p, zl0, nz,
                    (unsigned long long *)ctx->pool_paint.p, d_any));
    int any = 0;
    ARVX_HIP(hipMemcpyAsync(&any, d_any, sizeof any, hipMemcpyDeviceToHost, ctx->stream));
    ARVX_SYNC(ctx);  // (also: the host bytes may go away)
    ctx->paint_valid = had || any != 0;
    return ARVX_OK;
}

// the byte staging buffer holds the current state of local planes [zl0, zl0 + nz)
static int records_into_bytes(Ctx *ctx, int zl0, int nz) {
    if (int rc = need_rec(ctx, true)) return rc;  // (rec_to_bytes_kernel reads lazy tiles)
    ARVX_HIP(ctx->pool_state_bytes.reserve(ctx->nvox_ext));
    arvx::CarveParams g = record_params(ctx);
    return launch(ctx, arvx::rec_to_bytes_kernel, (unsigned)((size_t)g.tilesX * g.tilesY * g.tilesZ), 256,
                  g, (uint8_t *)ctx->pool_state_bytes.p, zl0, nz, paint_plane(ctx));
}

int arvx_state_reset(arvx_ctx *ctx) {
    ARVX_CHECK_CTX(ctx);
    ctx->drop(Event::Reset);
    ctx->form = Form::Fresh;  // written out by need_rec, or never (a carve of a fresh model writes every record)
    return ARVX_OK;
}

int arvx_state_upload(arvx_ctx *ctx, const uint8_t *state) {
    ARVX_CHECK_CTX(ctx);
    if (!state) return fail(ARVX_ERR_INVALID, "null state");
    ctx->drop(Event::UploadState);  // (paint of the owned planes is replaced; what the halo planes hold stays)
    ARVX_HIP(ctx->pool_state_bytes.reserve(ctx->nvox_ext));
    ARVX_HIP(hipMemcpyAsync(ctx->owned(), state, ctx->nvox, hipMemcpyHostToDevice, ctx->stream));
    return bytes_into_records(ctx, ctx->z0 - ctx->ze0, ctx->z1 - ctx->z0);
}

int arvx_state_upload_halo(arvx_ctx *ctx, const uint8_t *plane_below, const uint8_t *plane_above) {
    ARVX_CHECK_CTX(ctx);
    const size_t plane = (size_t)ctx->X * ctx->Y;
    if (ctx->stripe_world > 1) return fail(ARVX_ERR_STATE, "striped slabs keep no halo planes");
    ctx->drop(Event::UploadHalo);
    ARVX_HIP(ctx->pool_state_bytes.reserve(ctx->nvox_ext));
    if (plane_below && ctx->ze0 < ctx->z0) {  // plane z0 - 1
        ARVX_HIP(hipMemcpyAsync(ctx->owned() - plane, plane_below, plane, hipMemcpyHostToDevice,
                                ctx->stream));
        if (int rc = bytes_into_records(ctx, ctx->z0 - ctx->ze0 - 1, 1)) return rc;
    }
    if (plane_above && ctx->ze1 > ctx->z1) {
        ARVX_HIP(hipMemcpyAsync(ctx->owned() + ctx->nvox, plane_above, plane,
                                hipMemcpyHostToDevice, ctx->stream));
        if (int rc = bytes_into_records(ctx, ctx->z1 - ctx->ze0, 1)) return rc;
    }
    return ARVX_OK;
}

int arvx_state_download(arvx_ctx *ctx, uint8_t *state) {
    ARVX_CHECK_CTX(ctx);
    if (!state) return fail(ARVX_ERR_INVALID, "null state");
    if (int mrc = records_into_bytes(ctx, ctx->z0 - ctx->ze0, ctx->z1 - ctx->z0)) return mrc;
    ARVX_HIP(hipMemcpyAsync(state, ctx->owned(), ctx->nvox, hipMemcpyDeviceToHost, ctx->stream));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

int arvx_state_upload_planes(arvx_ctx *ctx, const uint32_t *occ, const uint32_t *seen) {
    ARVX_CHECK_CTX(ctx);
    if (!occ || !seen) return fail(ARVX_ERR_INVALID, "null plane");
    ctx->drop(Event::UploadPlanes);
    if (int mrc = need_rec(ctx)) return mrc;  // (halo planes keep what they hold)
    const int nz = ctx->z1 - ctx->z0;
    const size_t nwords = (size_t)((ctx->X + 31) / 32) * ctx->Y * nz;
    ARVX_HIP(ctx->pool_scratch.reserve(2 * nwords * sizeof(uint32_t) + 64));
    uint32_t *d_occ = (uint32_t *)ctx->pool_scratch.p, *d_seen = d_occ + nwords;
    ARVX_HIP(hipMemcpyAsync(d_occ, occ, nwords * 4, hipMemcpyHostToDevice, ctx->stream));
    ARVX_HIP(hipMemcpyAsync(d_seen, seen, nwords * 4, hipMemcpyHostToDevice, ctx->stream));
    arvx::CarveParams g = record_params(ctx);
    ARVX_TRY(launch(ctx, arvx::rec_from_planes_kernel, blocks_for(nwords), 256, g, ctx->z0 - ctx->ze0, nz, d_occ,
                    d_seen));
    ARVX_SYNC(ctx);  // the host planes may go away
    return ARVX_OK;
}

int arvx_state_download_planes(arvx_ctx *ctx, uint32_t *occ, uint32_t *seen) {
    ARVX_CHECK_CTX(ctx);
    if (!occ || !seen) return fail(ARVX_ERR_INVALID, "null plane");
    if (int mrc = need_rec(ctx, true)) return mrc;  // (planes_from_rec_kernel reads lazy tiles)
    const int nz = ctx->z1 - ctx->z0;
    const size_t nwords = (size_t)((ctx->X + 31) / 32) * ctx->Y * nz;
    ARVX_HIP(ctx->pool_scratch.reserve(2 * nwords * sizeof(uint32_t) + 64));
    uint32_t *d_occ = (uint32_t *)ctx->pool_scratch.p, *d_seen = d_occ + nwords;
    arvx::CarveParams g = record_params(ctx);
    ARVX_TRY(launch(ctx, arvx::planes_from_rec_kernel, blocks_for(nwords), 256, g, ctx->z0 - ctx->ze0, nz, d_occ,
                    d_seen));
    ARVX_HIP(hipMemcpyAsync(occ, d_occ, nwords * 4, hipMemcpyDeviceToHost, ctx->stream));
    ARVX_HIP(hipMemcpyAsync(seen, d_seen, nwords * 4, hipMemcpyDeviceToHost, ctx->stream));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

int arvx_state_packet_geometry(arvx_ctx *ctx, int64_t *words64, int64_t *header_words) {
    if (!ctx || !words64 || !header_words) return fail(ARVX_ERR_INVALID, "null argument");
    const size_t plane = (size_t)ctx->X * ctx->Y;
    if (ctx->X % 32 || plane % 64)
        return fail(ARVX_ERR_INVALID, "state packets need X %% 32 == 0 and X*Y %% 64 == 0 (X=%d, Y=%d)", ctx->X,
                    ctx->Y);
    const long long n = (long long)(plane / 64) * (ctx->z1 - ctx->z0);
    if (2 * n >= (1ll << 32)) return fail(ARVX_ERR_INVALID, "slab too large for state packets (%lld words)", n);
    *words64 = n;
    *header_words = arvx::occ_packet_header(n);
    return ARVX_OK;
}

int arvx_state_download_packets(arvx_ctx *ctx, uint64_t *occ_packet, int64_t occ_cap, uint64_t *seen_packet,
                                int64_t seen_cap, int64_t *occ_need, int64_t *seen_need) {
    ARVX_CHECK_CTX(ctx);
    if (!occ_packet || !seen_packet || !occ_need || !seen_need || occ_cap < 0 || seen_cap < 0)
        return fail(ARVX_ERR_INVALID, "bad argument");
    int64_t n64 = 0, H64 = 0;
    if (int rc = arvx_state_packet_geometry(ctx, &n64, &H64)) return rc;
    const long long n = n64, H = H64, nb = (n + 63) / 64;
    // the two packets at their worst-case size stay on the device until the state changes: a caller
    // whose buffers were too small asks again and only the copies run
    const size_t S = (size_t)(H + n);
    if (!(ctx->packets_seq == ctx->state_seq && ctx->pool_state_packets.cap >= 2 * S * 8)) {
        if (int mrc = need_rec(ctx, true)) return mrc;
        ARVX_HIP(ctx->pool_state_packets.reserve(2 * S * 8));
        arvx::CarveParams g = record_params(ctx);
        const int zl0 = ctx->z0 - ctx->ze0;
        const int nwg = (int)((nb + arvx::kOccGroupsPerWg - 1) / arvx::kOccGroupsPerWg);
        arvx::OccGeom og;
        og.wpr = arvx::fast_div((unsigned)(ctx->X / 32));
        og.Y = arvx::fast_div((unsigned)ctx->Y);
        og.P64 = arvx::fast_div((unsigned)((size_t)ctx->X * ctx->Y / 64));
        ARVX_HIP(ctx->pool_scratch.reserve(2 * (size_t)nwg * sizeof(int) + 64));
        int *d_wgsum = (int *)ctx->pool_scratch.p;
        unsigned long long *pk = (unsigned long long *)ctx->pool_state_packets.p;
        ARVX_TRY(launch(ctx, arvx::occ_pack_classify_kernel<false>, nwg, 256, g, og, zl0, n, pk, d_wgsum,
                        nullptr));
        ARVX_TRY(launch(ctx, arvx::occ_pack_classify_kernel<true>, nwg, 256, g, og, zl0, n, pk + S,
                        d_wgsum + nwg, nullptr));
        ARVX_TRY(launch(ctx, arvx::occ_pack_write_kernel<false>, blocks_for(nb, 4), 256, g, og, zl0, n, n,
                        d_wgsum, nwg, pk));
        ARVX_TRY(launch(ctx, arvx::occ_pack_write_kernel<true>, blocks_for(nb, 4), 256, g, og, zl0, n, n,
                        d_wgsum + nwg, nwg, pk + S));
        // the two counts first (16 bytes through their page-locked count words)
        ARVX_HIP(hipMemcpyAsync(&ctx->word(Ctx::kPacketOcc), pk, 8, hipMemcpyDeviceToHost, ctx->stream));
        ARVX_HIP(hipMemcpyAsync(&ctx->word(Ctx::kPacketSeen), pk + S, 8, hipMemcpyDeviceToHost, ctx->stream));
        ARVX_SYNC(ctx);
        ctx->packet_need[0] = ctx->word(Ctx::kPacketOcc);
        ctx->packet_need[1] = ctx->word(Ctx::kPacketSeen);
        ctx->packets_seq = ctx->state_seq;
    }
    const unsigned long long *pk = (const unsigned long long *)ctx->pool_state_packets.p;
    *occ_need = ctx->packet_need[0];
    *seen_need = ctx->packet_need[1];
    ARVX_HIP(hipMemcpyAsync(occ_packet, pk, (size_t)(H + std::min<long long>(*occ_need, occ_cap)) * 8,
                            hipMemcpyDeviceToHost, ctx->stream));
    ARVX_HIP(hipMemcpyAsync(seen_packet, pk + S, (size_t)(H + std::min<long long>(*seen_need, seen_cap)) * 8,
                            hipMemcpyDeviceToHost, ctx->stream));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

int arvx_handle_unseen(arvx_ctx *ctx) {
    ARVX_CHECK_CTX(ctx);
    // (coarse tiles that exist only as their code stay codes: "carved and seen", "untouched and
    // seen" and "untouched, not seen" are all unchanged by occ |= ~seen -- the records behind a
    // code are not read by anybody)
    if (int mrc = need_rec(ctx, true)) return mrc;
    // (after need_rec, which may fail: the drop hands the colour pass's planes on to the state this
    // call makes)
    ctx->drop(Event::HandleUnseen);
    arvx::CarveParams g;
    carve_geometry(ctx, g);
    const size_t nrec = arvx::rec_count(g);
    return launch(ctx, arvx::rec_handle_unseen_kernel, blocks_for(nrec * 32), 256, (uint32_t *)ctx->rec(), nrec,
                  g.ccode, g.cyShift + g.czShift + 2);
}

int arvx_host_register(void *ptr, size_t bytes) {
    if (!ptr || !bytes) return fail(ARVX_ERR_INVALID, "null host range");
    ARVX_HIP(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    return ARVX_OK;
}

int arvx_host_unregister(void *ptr) {
    if (!ptr) return fail(ARVX_ERR_INVALID, "null host pointer");
    ARVX_HIP(hipHostUnregister(ptr));
    return ARVX_OK;
}

int arvx_state_device_ptr(arvx_ctx *ctx, void **ptr, size_t *bytes) {
    if (!ctx || !ptr) return fail(ARVX_ERR_INVALID, "null argument");
    ARVX_HIP(hipSetDevice(ctx->device));
    if (int mrc = records_into_bytes(ctx, ctx->z0 - ctx->ze0, ctx->z1 - ctx->z0)) return mrc;
    *ptr = ctx->owned();
    if (bytes) *bytes = ctx->nvox;
    return ARVX_OK;
}

// X % 64 == 0 and an 8-byte aligned destination: the tile-wise pack (state_kernels.h)
static int launch_pack_tiles(Ctx *ctx, int global, void *dev_words) {
    if (int mrc = need_rec(ctx, true)) return mrc;
    arvx::CarveParams g = record_params(ctx);
    const int zl0 = ctx->z0 - ctx->ze0, nz = ctx->z1 - ctx->z0;
    const int ntz = ((zl0 + nz - 1) >> 3) - (zl0 >> 3) + 1;
    const size_t tiles = (size_t)g.tilesX * g.tilesY * ntz;
    return launch(ctx, arvx::pack_occupancy_tile_kernel, blocks_for(tiles, 4), 256, g, zl0, nz, global,
                  (unsigned long long *)dev_words);
}

int arvx_pack_occupancy(arvx_ctx *ctx, void *dev_words) {
    ARVX_CHECK_CTX(ctx);
    ExchangeStreamScope exchange_scope(ctx);
    if (!dev_words) return fail(ARVX_ERR_INVALID, "null dev_words");
    if (ctx->X % 64 == 0 && (uintptr_t)dev_words % 8 == 0) return launch_pack_tiles(ctx, 0, dev_words);
    if (ctx->X % 32 == 0 && (uintptr_t)dev_words % 4 == 0) {
        // straight from the records: 2 bits per voxel in, 1 out
        if (int mrc = need_rec(ctx, true)) return mrc;
        arvx::CarveParams g = record_params(ctx);
        const int nz = ctx->z1 - ctx->z0;
        const size_t nwords = (size_t)(ctx->X / 32) * ctx->Y * nz;
        return launch(ctx, arvx::pack_occupancy_rec_kernel, blocks_for(nwords), 256, g, ctx->z0 - ctx->ze0, nz,
                      0, (uint32_t *)dev_words);
    }
    if (ctx->X % 8 == 0 && ((size_t)ctx->X * ctx->Y) % 32 == 0 && (uintptr_t)dev_words % 4 == 0) {
        if (int mrc = need_rec(ctx, true)) return mrc;
        arvx::CarveParams g = record_params(ctx);
        const int nz = ctx->z1 - ctx->z0;
        const size_t nwords = ((size_t)ctx->X * ctx->Y * nz / 8 + 3) / 4;
        return launch(ctx, arvx::pack_occupancy_rec8_kernel, blocks_for(nwords), 256, g, ctx->z0 - ctx->ze0, nz,
                      0, (uint32_t *)dev_words);
    }
    // odd row lengths: through the byte form
    if (int mrc = records_into_bytes(ctx, ctx->z0 - ctx->ze0, ctx->z1 - ctx->z0)) return mrc;
    if (ctx->nvox % 32 == 0 && (uintptr_t)ctx->owned() % 16 == 0 && (uintptr_t)dev_words % 4 == 0) {
        const size_t nwords = ctx->nvox / 32;
        ARVX_TRY(launch(ctx, arvx::pack_occupancy32_kernel, blocks_for(nwords), 256, ctx->owned(), nwords,
                        (uint32_t *)dev_words));
    } else if (ctx->nvox % 32 == 0 && (uintptr_t)ctx->owned() % 8 == 0) {
        const size_t nbytes = ctx->nvox / 8;
        ARVX_TRY(launch(ctx, arvx::pack_occupancy8_kernel, blocks_for(nbytes), 256, ctx->owned(), nbytes,
                        (uint8_t *)dev_words));
    } else {
        const size_t nround = (ctx->nvox + 255) / 256;
        const unsigned grid = (unsigned)(nround < 8192 ? (nround ? nround : 1) : 8192);
        ARVX_TRY(launch(ctx, arvx::pack_occupancy_kernel, grid, 256, ctx->owned(), ctx->nvox,
                        (uint32_t *)dev_words));
    }
    return ARVX_OK;
}

int arvx_pack_occupancy_global(arvx_ctx *ctx, void *dev_global_words) {
    ARVX_CHECK_CTX(ctx);
    ExchangeStreamScope exchange_scope(ctx);
    if (!dev_global_words) return fail(ARVX_ERR_INVALID, "null dev_global_words");
    const size_t plane = (size_t)ctx->X * ctx->Y;
    if (plane % 64) return fail(ARVX_ERR_INVALID, "X*Y must be a multiple of 64");
    if (ctx->X % 64 == 0 && (uintptr_t)dev_global_words % 8 == 0)
        return launch_pack_tiles(ctx, 1, dev_global_words);
    if (ctx->X % 32 == 0) {
        if (int mrc = need_rec(ctx, true)) return mrc;
        arvx::CarveParams g = record_params(ctx);
        const int nz = ctx->z1 - ctx->z0;
        const size_t nwords = (size_t)(ctx->X / 32) * ctx->Y * nz;
        return launch(ctx, arvx::pack_occupancy_rec_kernel, blocks_for(nwords), 256, g, ctx->z0 - ctx->ze0, nz,
                      1, (uint32_t *)dev_global_words);
    }
    if (ctx->X % 8 == 0) {  // (X * Y % 64 == 0 above)
        if (int mrc = need_rec(ctx, true)) return mrc;
        arvx::CarveParams g = record_params(ctx);
        const int nz = ctx->z1 - ctx->z0;
        const size_t nwords = (size_t)ctx->X * ctx->Y * nz / 32;
        return launch(ctx, arvx::pack_occupancy_rec8_kernel, blocks_for(nwords), 256, g, ctx->z0 - ctx->ze0, nz,
                      1, (uint32_t *)dev_global_words);
    }
    if (int mrc = records_into_bytes(ctx, ctx->z0 - ctx->ze0, ctx->z1 - ctx->z0)) return mrc;
    // plane % 64 == 0 and an aligned allocation: every plane starts on an 8-byte boundary
    const size_t nbytes = ctx->nvox / 8;
    return launch(ctx, arvx::pack_occupancy_global8_kernel, blocks_for(nbytes), 256, ctx->owned(), plane,
                  ctx->z1 - ctx->z0, ctx->stripe_world > 1 ? 0 : ctx->z0, ctx->stripe_world,
                  ctx->stripe_rank, (uint8_t *)dev_global_words);
}

// ---- compressed occupancy exchange -----------------------------------------------------

int64_t arvx_occupancy_packet_words(int64_t n_words64, int64_t cap_words64) {
    if (n_words64 < 0 || cap_words64 < 0) return -1;
    return (int64_t)arvx::occ_packet_header(n_words64) + cap_words64;
}

int arvx_occupancy_compress(arvx_ctx *ctx, const void *dev_words, int64_t n_words64,
                            void *dev_packet, int64_t cap_words64) {
    ARVX_CHECK_CTX(ctx);
    ExchangeStreamScope exchange_scope(ctx);
    if (!dev_words || !dev_packet || n_words64 <= 0 || cap_words64 < 0)
        return fail(ARVX_ERR_INVALID, "bad argument");
    if (((uintptr_t)dev_words | (uintptr_t)dev_packet) & 7u)
        return fail(ARVX_ERR_INVALID, "buffers must be 8-byte aligned");
    const long long n = n_words64, nb = (n + 63) / 64;
    const int nwg = (int)((nb + arvx::kOccGroupsPerWg - 1) / arvx::kOccGroupsPerWg);
    // a buffer of its own: this call may run on the exchange stream beside the views / carve of
    // the next job, whose tables live in d_scratch (arvx_ctx_set_exchange_stream).  Growing it
    // frees the old one, which hipFree orders after everything the device has in flight.
    ARVX_HIP(ctx->pool_xscratch.reserve((size_t)(nwg + 1) * sizeof(long long) +
                                        (size_t)nwg * sizeof(int) + 64));
    long long *d_wgoff = (long long *)ctx->pool_xscratch.p;  // nwg + 1 offsets, last = total
    int *d_wgsum = (int *)(d_wgoff + nwg + 1);
    const unsigned long long *words = (const unsigned long long *)dev_words;
    unsigned long long *packet = (unsigned long long *)dev_packet;
    ARVX_TRY(launch(ctx, arvx::occ_classify_kernel, nwg, 256, words, n, packet, d_wgsum));
    ARVX_TRY(launch(ctx, arvx::mc_scan_blocks_kernel, 1, 256, d_wgsum, nwg, d_wgoff));
    return launch(ctx, arvx::occ_write_kernel, blocks_for(nb, 4), 256, words, n, cap_words64, d_wgoff, nwg, packet);
}

int arvx_occupancy_pack_compress(arvx_ctx *ctx, void *dev_packet, int64_t cap_words64,
                                 void *dev_full_words) {
    ARVX_CHECK_CTX(ctx);
    ExchangeStreamScope exchange_scope(ctx);
    if (!dev_packet || cap_words64 < 0) return fail(ARVX_ERR_INVALID, "bad argument");
    if (((uintptr_t)dev_packet | (uintptr_t)dev_full_words) & 7u)
        return fail(ARVX_ERR_INVALID, "buffers must be 8-byte aligned");
    const size_t plane = (size_t)ctx->X * ctx->Y;
    if (ctx->X % 32 || plane % 64)
        return fail(ARVX_ERR_INVALID, "needs X %% 32 == 0 and X*Y %% 64 == 0 (X=%d, Y=%d)", ctx->X, ctx->Y);
    if (int mrc = need_rec(ctx, true)) return mrc;
    arvx::CarveParams g = record_params(ctx);
    const int zl0 = ctx->z0 - ctx->ze0, nz = ctx->z1 - ctx->z0;
    const long long n = (long long)(plane / 64) * nz, nb = (n + 63) / 64;
    if (2 * n >= (1ll << 32)) return fail(ARVX_ERR_INVALID, "slab too large for the fused packet (%lld words)", n);
    const int nwg = (int)((nb + arvx::kOccGroupsPerWg - 1) / arvx::kOccGroupsPerWg);
    arvx::OccGeom og;
    og.wpr = arvx::fast_div((unsigned)(ctx->X / 32));
    og.Y = arvx::fast_div((unsigned)ctx->Y);
    og.P64 = arvx::fast_div((unsigned)(plane / 64));
    // (a buffer of its own: the call may run on the exchange stream beside the next job's views)
    ARVX_HIP(ctx->pool_xscratch.reserve((size_t)(nwg + 1) * sizeof(long long) +
                                        (size_t)nwg * sizeof(int) + 64));
    int *d_wgsum = (int *)((long long *)ctx->pool_xscratch.p + nwg + 1);
    unsigned long long *packet = (unsigned long long *)dev_packet;
    ARVX_TRY(launch(ctx, arvx::occ_pack_classify_kernel<false>, nwg, 256, g, og, zl0, n, packet, d_wgsum,
                    (unsigned long long *)dev_full_words));
    return launch(ctx, arvx::occ_pack_write_kernel<false>, blocks_for(nb, 4), 256, g, og, zl0, n, cap_words64,
                  d_wgsum, nwg, packet);
}

int arvx_occupancy_expand(arvx_ctx *ctx, const void *dev_packets, int world, int self_rank,
                          int64_t n_words64, int64_t cap_words64, void *dev_full_words,
                          int *dev_overflow) {
    ARVX_CHECK_CTX(ctx);
    ExchangeStreamScope exchange_scope(ctx);
    if (!dev_packets || !dev_full_words || !dev_overflow || world < 1 || self_rank < 0 ||
        self_rank >= world || n_words64 <= 0 || cap_words64 < 0)
        return fail(ARVX_ERR_INVALID, "bad argument");
    if (((uintptr_t)dev_packets & 7u) || ((uintptr_t)dev_full_words & 15u))
        return fail(ARVX_ERR_INVALID, "packets must be 8-byte, the word plane 16-byte aligned");
    const long long n = n_words64, nb = (n + 63) / 64;
    const long long S = arvx::occ_packet_header(n) + cap_words64;
    const long long per = (nb + 2 * arvx::kExpandChunks - 1) / (2 * arvx::kExpandChunks);
    return launch(ctx, arvx::occ_expand_kernel, blocks_for(per * world, 4), 256,
                  (const unsigned long long *)dev_packets, S, world, self_rank, n, cap_words64,
                  (unsigned long long *)dev_full_words, dev_overflow, 0ll);
}

int arvx_occupancy_expand_striped(arvx_ctx *ctx, const void *dev_packets, int world,
                                  int64_t n_words64, int64_t cap_words64, int64_t words_per_group,
                                  void *dev_full_words, int *dev_overflow) {
    return arvx_occupancy_expand_striped_others(ctx, dev_packets, world, -1, n_words64, cap_words64,
                                                words_per_group, dev_full_words, dev_overflow);
}

int arvx_occupancy_expand_striped_others(arvx_ctx *ctx, const void *dev_packets, int world,
                                         int self_rank, int64_t n_words64, int64_t cap_words64,
                                         int64_t words_per_group, void *dev_full_words,
                                         int *dev_overflow) {
    ARVX_CHECK_CTX(ctx);
    ExchangeStreamScope exchange_scope(ctx);
    if (self_rank < -1 || self_rank >= world) return fail(ARVX_ERR_INVALID, "self_rank %d of %d", self_rank, world);
    if (!dev_packets || !dev_full_words || !dev_overflow || world < 1 || n_words64 <= 0 ||
        cap_words64 < 0 || words_per_group < 2 || (words_per_group & 1) ||
        n_words64 % words_per_group)
        return fail(ARVX_ERR_INVALID, "bad argument (words per group must be even and divide n)");
    if (((uintptr_t)dev_packets & 7u) || ((uintptr_t)dev_full_words & 15u))
        return fail(ARVX_ERR_INVALID, "packets must be 8-byte, the word plane 16-byte aligned");
    const long long n = n_words64, nb = (n + 63) / 64;
    const long long S = arvx::occ_packet_header(n) + cap_words64;
    const long long per = (nb + 2 * arvx::kExpandChunks - 1) / (2 * arvx::kExpandChunks);
    return launch(ctx, arvx::occ_expand_kernel, blocks_for(per * world, 4), 256,
                  (const unsigned long long *)dev_packets, S, world, self_rank, n, cap_words64,
                  (unsigned long long *)dev_full_words, dev_overflow, words_per_group);
}

// ---- carve -------------------------------------------------------------------

#ifdef ARVX_TIMELINE
// the diagnostic timeline of the launch that follows: n records of `rec` bytes, zeroed
static int timeline(Ctx *ctx, size_t n, int rec, arvx::CarveParams &p) {
    ctx->pool_timeline.release();
    ctx->timeline_n = (int64_t)n;
    ctx->timeline_rec = rec;
    ARVX_HIP(ctx->pool_timeline.reserve(n * rec));
    ARVX_HIP(hipMemsetAsync(ctx->pool_timeline.p, 0, n * rec, ctx->stream));
    p.timeline = (unsigned long long *)ctx->pool_timeline.p;
    return ARVX_OK;
}
#endif

// Launches the carve over planes [ze0, ze1) (owned + halo) of the records at `rec`.
#ifdef ARVX_EXPERIMENTS
// A fresh model carved by ONE persistent launch (carve_stream_kernels.h).  p: geometry, views and
// flags filled in by launch_carve.
static int launch_carve_stream(Ctx *ctx, arvx::CarveParams p, int ncu) {
    const size_t ncoarse = (size_t)p.coarseX * p.coarseY * p.coarseZ;
    const unsigned G = (unsigned)ncu * 4u;  // resident workgroups (128 VGPRs: 4 per compute unit)
    // (the chunks of 64 views are a template parameter of the kernel: 1, or all four)
    if (p.nchunks > 1) p.nchunks = arvx::kMaxChunks;
    // a coarse unit (one wave): up to four coarse tiles, so that every wave gets one
    p.cwA = (int)std::min<size_t>(arvx::kStreamTilesA, std::max<size_t>(1, (ncoarse + 4 * G - 1) / (4 * G)));
    p.nA = (int)((ncoarse + p.cwA - 1) / p.cwA);
    // a sub-tile unit (one wave): 16 sub-tiles, a quarter of a coarse tile (half on striped slabs)
    p.splitLog2 = p.cyShift + p.czShift - 2;
    p.listStride = 1 + 2 * p.nchunks;
    p.itemStride = 2 + 4 * p.nchunks;
    // A unit u appends to list part u % 8: a part gets at most every 8th unit's tiles
    p.listCap = (p.nA / arvx::kStreamLists + 1) * p.cwA;
    // sub-tile i (of 4 per tile) goes to list i % 8 of one of eight weight classes: a list never
    // gets more than every 8th sub-tile
    p.workCap = (int)(((size_t)p.tilesX * p.tilesY * p.tilesZ * 4 + 7) / 8);
    const size_t off_list = ((size_t)arvx::kStreamLines * arvx::kCounterStride * sizeof(int) + 255) / 256 * 256;
    const size_t off_items =
        off_list + ((size_t)arvx::kStreamLists * p.listCap * p.listStride * 8 + 255) / 256 * 256;
    const size_t need = off_items + (size_t)arvx::kWorkLists * p.workCap * p.itemStride * 8 + 256;
    if (ctx->pool_stream.cap < need) {
        ctx->stream_layout = 0;
        ARVX_HIP(ctx->pool_stream.reserve(need));
        // (stale granules are told by their tag; but the memory must not hold a FUTURE tag)
        ARVX_HIP(hipMemsetAsync(ctx->pool_stream.p, 0, need, ctx->stream));
        ctx->carve_epoch = 0;
    }
    if (ctx->stream_layout != need) {  // the control block: all zero before a launch
        ARVX_HIP(hipMemsetAsync(ctx->pool_stream.p, 0, off_list, ctx->stream));
        ctx->stream_layout = need;
    }
    if (++ctx->carve_epoch == 0u) {  // (2^32 launches: start the tags over on clean memory)
        ARVX_HIP(hipMemsetAsync(ctx->pool_stream.p, 0, need, ctx->stream));
        ctx->carve_epoch = 1u;
    }
    p.sctl = (int *)ctx->pool_stream.p;
    p.poolNext = p.sctl + (size_t)arvx::kSC_Pool * arvx::kCounterStride;
    p.listG = (unsigned long long *)((uint8_t *)ctx->pool_stream.p + off_list);
    p.itemG = (unsigned long long *)((uint8_t *)ctx->pool_stream.p + off_items);
    p.epoch = ctx->carve_epoch;
    p.fault = ctx->d_fault;
    p.nwaves = (int)G * 4;
    ARVX_HIP(ctx->pool_ccode.reserve(ncoarse + 64));
    ARVX_HIP(ctx->pool_cstate.reserve(ncoarse + 64));
    p.coarseCarved = (uint8_t *)ctx->pool_ccode.p;
    p.cstate = (uint8_t *)ctx->pool_cstate.p;
    p.flags |= 128u;
    ctx->cstate_tiles = 0;
#ifdef ARVX_TIMELINE
    if (int rc = timeline(ctx, (size_t)G * 4, 128, p)) return rc;  // one record per wave
#endif
    // (the chunks of 64 views are a template parameter: up to 64 views, or up to 256)
    const bool left = ctx->assoc == ARVX_ASSOC_LEFT, one = p.nchunks == 1;
    void (*stream)(arvx::CarveParams) = left && one ? arvx::carve_stream_kernel<true, 1>
                                        : left      ? arvx::carve_stream_kernel<true, arvx::kMaxChunks>
                                        : one       ? arvx::carve_stream_kernel<false, 1>
                                                    : arvx::carve_stream_kernel<false, arvx::kMaxChunks>;
    ARVX_TRY(launch(ctx, stream, G, 256, p));
    ctx->form = Form::Lazy;
    ctx->cstate_tiles = ncoarse;
    ctx->path_bits = ARVX_PATH_STREAM | ARVX_PATH_FRESH | ARVX_PATH_LAZY_CODES;
    return ARVX_OK;
}
#endif

// ---- cached rectangles (rect_cache_kernels.h) ---------------------------------------------------

// field widths of a table entry for the context's image size
static arvx::RectBits rect_bits(const Ctx *ctx) {
    arvx::RectBits rb = {1, 1, 0};
    while ((1 << rb.xb) < ctx->W) ++rb.xb;
    while ((1 << rb.yb) < ctx->H) ++rb.yb;
    rb.db = (32 - rb.xb - rb.yb) / 2;
    return rb;
}
static size_t rect_entries(const Ctx *ctx, const arvx::CarveParams &p) {
    return (arvx::rec_count(p) << 4) * (size_t)ctx->V;
}
static void rect_params(const Ctx *ctx, arvx::CarveParams &p) {
    const arvx::RectBits rb = rect_bits(ctx);
    p.rcXB = rb.xb;
    p.rcYB = rb.yb;
    p.rcDB = rb.db;
}

// lanes of the table of cached pixels (16 bytes each), and the words of its per-view "does not fit"
// mask behind them (one more than the views need: the kernel reads the word after a chunk's)
static size_t pixel_lanes(const Ctx *ctx, const arvx::CarveParams &p) {
    return (arvx::rec_count(p) << 6) * (size_t)ctx->V;
}
static size_t pixel_miss_words(const Ctx *ctx) { return (size_t)(ctx->V + 63) / 64 + 1; }
static unsigned pixel_grid(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, (size_t)1 << 20); }

// The table of pixels, for a carve that reads the block table (p.rcBlk stands): built once per set
// of cameras and grouping, under its own limit; handed to p once it stands.  Like the block table's,
// the build ends with a synchronisation, after which the host knows which views fit.
static int pixel_cache_prepare(Ctx *ctx, arvx::CarveParams &p) {
    if (!ctx->pix_limit) return ARVX_OK;
    if (ctx->pix_state != Ctx::Rect::None && ctx->pix_assoc != ctx->assoc) ctx->pix_state = Ctx::Rect::None;
    if (ctx->pix_state == Ctx::Rect::None) {
        ctx->pix_state = Ctx::Rect::Refused;
        ctx->pix_assoc = ctx->assoc;
        const size_t n = pixel_lanes(ctx, p), nw = pixel_miss_words(ctx);
        const size_t bytes = n * sizeof(uint4) + nw * sizeof(unsigned long long);
        if (bytes > ctx->pix_limit) {
            ctx->pool_pix.release();  // (one of an earlier, smaller set of views)
            return ARVX_OK;
        }
        if (ctx->pool_pix.reserve(bytes) != hipSuccess) {  // (no room on the device: no table, no error)
            (void)hipGetLastError();
            return ARVX_OK;
        }
        uint4 *tab = (uint4 *)ctx->pool_pix.p;
        unsigned long long *miss = (unsigned long long *)(tab + n);
        ARVX_HIP(hipMemsetAsync(miss, 0, nw * sizeof *miss, ctx->stream));
        ARVX_TRY(by_assoc(ctx, [&](auto left) {
            return launch(ctx, arvx::pixel_cache_kernel<decltype(left)::value, false>, pixel_grid(n), 256, p, tab,
                          n, miss, nullptr);
        }));
        ctx->pix_miss.assign(nw, 0ull);
        ARVX_HIP(hipMemcpyAsync(ctx->pix_miss.data(), miss, nw * sizeof *miss, hipMemcpyDeviceToHost, ctx->stream));
        ARVX_SYNC(ctx);
        ctx->pix_state = Ctx::Rect::Built;
    }
    if (ctx->pix_state == Ctx::Rect::Built) {
        p.pxTab = (const uint4 *)ctx->pool_pix.p;
        p.pxMiss = (const unsigned long long *)(p.pxTab + pixel_lanes(ctx, p));
    }
    return ARVX_OK;
}

// A carve of a fresh model that runs the dense classify kernel and the unshared block-mapped exact
// kernel on the context's own records: counts it, builds the table at the second one in a row
// under the same views, and hands p the table once it stands.  The build ends with a synchronisation -- once per set of
// cameras --, after which the host knows whether every block rectangle fitted its entry.
static int rect_cache_prepare(Ctx *ctx, arvx::CarveParams &p) {
    if (!ctx->rect_limit) return ARVX_OK;
    if (ctx->rect_streak < 2) ++ctx->rect_streak;
    if (ctx->rect_streak < 2) return ARVX_OK;
    rect_params(ctx, p);
    if (ctx->rect_state == Ctx::Rect::None) {
        ctx->rect_state = Ctx::Rect::Refused;
        const size_t n = rect_entries(ctx, p), bytes = n * sizeof(uint32_t);
        if (p.rcDB < 1 || bytes > ctx->rect_limit) return ARVX_OK;
        if (ctx->pool_rect.reserve(bytes) != hipSuccess) {  // (no room on the device: no table, no error)
            (void)hipGetLastError();
            return ARVX_OK;
        }
        ctx->word(Ctx::kRectMiss) = 0;
        ARVX_TRY(launch(ctx, arvx::rect_cache_block_kernel<false>,
                        (unsigned)std::min<size_t>((n + 255) / 256, 65536), 256, p,
                        (uint32_t *)ctx->pool_rect.p, n, ctx->word_dev(Ctx::kRectMiss), nullptr));
        ARVX_SYNC(ctx);
        if (ctx->word(Ctx::kRectMiss)) {  // a rectangle too large for an entry: computed as before
            ctx->word(Ctx::kRectMiss) = 0;
            ctx->pool_rect.release();
            return ARVX_OK;
        }
        ctx->rect_state = Ctx::Rect::Built;
    }
    if (ctx->rect_state != Ctx::Rect::Built) return ARVX_OK;
    p.rcBlk = (const uint32_t *)ctx->pool_rect.p;
    return pixel_cache_prepare(ctx, p);
}

// `fresh`: the model is all-occupied/unseen and exists only as that flag: nothing is read,
// every record of the grid is written.
// `foreign_code` (records that are not the context's own, fresh): the decided coarse tiles are not
// written there either -- their codes go to that array (ncoarse bytes) and its reader takes them
// from it (arvx_fast_carve).
static int launch_carve(Ctx *ctx, uint16_t *rec, int first, int count, unsigned flags,
                        bool fresh, uint8_t *foreign_code = nullptr) {
    arvx::CarveParams p;
    carve_geometry(ctx, p);
    p.rec = rec;
    carve_views(ctx, p);
    p.stats = ctx->stats();
    p.v0 = first;
    p.v1 = first + count;
    p.flags = (flags & 3u) | (fresh ? 4u : 0u);
    p.ccode = nullptr;  // (the carve reads records only where it has written them)
    p.cstate = nullptr;
    p.nchunks = (count + 63) / 64;
    if (flags & ARVX_CARVE_STATS) ARVX_HIP(hipMemsetAsync(ctx->stats(), 0, 64, ctx->stream));
    // rows of tiles (along x) are dealt to the XCDs cyclically: see carve_fused_kernel
    const size_t rows8 = ((size_t)p.tilesY * p.tilesZ + 7) / 8 * 8;
    const unsigned grid = (unsigned)(rows8 * p.tilesX);
    const bool cull = !(flags & ARVX_CARVE_NO_CULL);
    const bool split = cull && !(flags & ARVX_CARVE_FUSED) && p.nchunks <= arvx::kMaxChunks;
    static const bool two_launches = experiment_flag("ARVX_COARSE_SPLIT");
    const size_t ncoarse = (size_t)p.coarseX * p.coarseY * p.coarseZ;
    const int ncu = compute_units(ctx);
    size_t layout_when_done = 0;
    bool lazy = false;
    ctx->path_bits = ctx->path_dense_grid = 0;  // (arvx_last_carve_path)
    ctx->path_off_listed = ctx->path_off_work = 0;
    // a fresh model, the context's own records, up to 256 views: one persistent launch where the
    // caller asks for it (carve_stream_kernels.h; EXPERIMENTS.md, round 4: its sub-tile phase is
    // slower inside a launch of 128-register waves than as a launch of its own, so the three
    // launches below stay the default)
#ifdef ARVX_EXPERIMENTS
    static const bool stream_default = experiment_flag("ARVX_STREAM_DEFAULT");
    if (fresh && split && rec == ctx->rec() && !(flags & (ARVX_CARVE_STATS | ARVX_CARVE_NO_STREAM)) &&
        ((flags & ARVX_CARVE_STREAM) || (stream_default && (size_t)p.X * p.Y * p.Z >= ((size_t)1 << 26))) &&
        arvx::rec_count(p) < ((size_t)1 << 30) && p.tilesX < 65536 && p.tilesY < 65536 && p.tilesZ < 65536)
        return launch_carve_stream(ctx, p, ncu);
#endif
    if (cull) {
        const size_t words = ncoarse * p.nchunks;
        // coarse masks | coarse codes | undecided list | two list counters
        const size_t off_list = (2 * words * sizeof(unsigned long long) + ncoarse + 255) / 256 * 256;
        const size_t off_work = off_list + ((ncoarse + 2 * 64) * sizeof(int) + 255) / 256 * 256;
        const size_t nctr = (size_t)arvx::kWorkLists * arvx::kCounterStride;
        // sub-tile i (of 4 per tile) goes to list i % 8 of one of eight weight classes: a
        // list never gets more than every 8th sub-tile
        const size_t cap = ((size_t)p.tilesX * p.tilesY * p.tilesZ * 4 + 7) / 8;
        const size_t nitems = cap * arvx::kWorkLists;
        // one persistent workgroup per workgroup slot of the chip (4 per CU at 128 VGPRs)
        static const int exact_wgs = experiment_int("ARVX_EXACT_WGS_PER_CU");  // (A/B builds)
        // (the small grids' instantiation -- items shared between waves -- holds 149 registers, 3 per CU;
        // launched 4 per CU all the same: the fourth takes over as the first ends, C1 / C2 3 / 9 %
        // faster than with 3, EXPERIMENTS.md round 5)
        const unsigned pgrid = (unsigned)ncu * (exact_wgs > 0 ? (unsigned)exact_wgs : (unsigned)ARVX_EXACT_WAVES_PER_SIMD);
        const size_t nwaves = (size_t)pgrid * 4;
        const size_t nctr_pool = (size_t)arvx::kPoolCounters * arvx::kCounterStride;
        const size_t ints = nctr + nctr_pool;  // list fill counters, pool ticket counters
        const size_t off_items = off_work + (ints * sizeof(int) + 255) / 256 * 256;
        const size_t need =
            off_items + nitems * (1 + 2 * (size_t)p.nchunks) * sizeof(unsigned long long) + 64;
        ARVX_HIP(ctx->pool_coarse.reserve(need));
        p.coarseMixed = (unsigned long long *)ctx->pool_coarse.p;
        p.coarseFg = p.coarseMixed + words;
        p.coarseCarved = (uint8_t *)(p.coarseFg + words);
        // Lazy state: a fresh model carved by the split launch into the context's own records
        // does not write the coarse tiles it settles as a whole -- their code, kept in the
        // context, is their state (arvx_device.h; need_rec writes them out for the stages that
        // want records).
#ifndef ARVX_NO_LAZY  // (A/B builds: always write the decided tiles)
        lazy = fresh && split && (rec == ctx->rec() || foreign_code);
#endif
        if (lazy && rec == ctx->rec()) {
            ARVX_HIP(ctx->pool_ccode.reserve(ncoarse + 64));
            p.coarseCarved = (uint8_t *)ctx->pool_ccode.p;
            p.flags |= 128u;
        } else if (lazy) {
            p.coarseCarved = foreign_code;
            p.flags |= 128u;
        }
        // the model's own records: what this and earlier carves settle for whole coarse tiles
        // is remembered (CarveParams::cstate); a fresh carve rewrites every entry
        if (split && rec == ctx->rec()) {
            ARVX_HIP(ctx->pool_cstate.reserve(ncoarse + 64));
            if (!fresh && ctx->cstate_tiles != ncoarse)
                ARVX_HIP(hipMemsetAsync(ctx->pool_cstate.p, 0, ncoarse, ctx->stream));
            p.cstate = (uint8_t *)ctx->pool_cstate.p;
            ctx->cstate_tiles = 0;  // (valid again once the launches are out)
        }
        if (split) {
            int *lst = (int *)((uint8_t *)ctx->pool_coarse.p + off_list);
            // two counters, 64 ints apart, used alternately (carve_coarse_kernel): both zero
            // before the first carve that uses this layout
            if (ctx->carve_layout != need) {
                ARVX_HIP(hipMemsetAsync(lst, 0, 2 * 64 * sizeof(int), ctx->stream));
                ctx->carve_layout = need;
                ctx->carve_seq = 0;
            }
            p.undecidedCount = lst + 64 * (ctx->carve_seq & 1);
            p.undecidedCountNext = lst + 64 * ((ctx->carve_seq + 1) & 1);
            p.undecidedList = lst + 2 * 64;
            // (carve_seq advances once all launches of this carve are enqueued; a failure in
            // between leaves the layout unset, so that the next carve zeroes both counters)
            ctx->carve_layout = 0;
            layout_when_done = need;
            int *base = (int *)((uint8_t *)ctx->pool_coarse.p + off_work);
            p.workCount = base;
            p.poolNext = base + nctr;
            p.nwaves = (int)nwaves;
            p.workCap = (int)cap;
            p.itemInfo = (unsigned long long *)((uint8_t *)ctx->pool_coarse.p + off_items);
            p.itemMasks = p.itemInfo + nitems;
            // (carve_coarse_kernel zeroes the `ints` counters at base)
        }
        if (!split || two_launches || lazy) {
            // (lazy: one WAVE per coarse tile classifies it and lists it if it is undecided;
            // no workgroup per tile is needed when nothing is filled)
            // (16 tiles per workgroup where that still leaves a workgroup per compute unit:
            // fewer appends to the list's counter; 4 on small grids)
            if (p.nchunks > arvx::kMaxChunks) {  // (only the fused kernel takes that many views)
                ARVX_TRY(launch(ctx, arvx::carve_coarse_wave_kernel, blocks_for(ncoarse, 4), 256, p));
            } else {
                const int cw = ncoarse >= (size_t)16 * ncu ? arvx::kCoarseWaves : 4;
                p.coarsePerWg = cw;
                // (tile, view) pairs dealt to the lanes densely: as many waves as the pairs need
                const size_t pairs = (size_t)cw * (size_t)(p.v1 - p.v0);
                const unsigned threads =
                    (unsigned)std::min<size_t>(64 * arvx::kCoarseWaves, (pairs + 63) / 64 * 64);
                ARVX_TRY(launch(ctx, arvx::carve_coarse_kernel, (unsigned)((ncoarse + cw - 1) / cw),
                                std::max(threads, 64u), p));
            }
        }
    }
    // the statistics counters live in the row-mapped variant
    static const bool row_map = experiment_flag("ARVX_EXACT_ROWS");
    const bool blocks = split && !row_map && !(flags & ARVX_CARVE_STATS);
    // few sub-tiles per wave (small grids, slabs): the exact kernel may hand an item's views
    // to several waves (decided in the kernel from the length of the work lists)
    static const bool no_item_split = experiment_flag("ARVX_NO_ITEM_SPLIT");
    // (up to 2^26 voxels: above that there are more items than half the waves and the kernel
    // never splits; ARVX_ITEM_SPLIT_LOG2 in an experiment build moves the limit)
    static const int split_log2 = experiment_int("ARVX_ITEM_SPLIT_LOG2");
    if (blocks && !no_item_split && !(flags & ARVX_CARVE_WHOLE_ITEMS) &&
        (size_t)p.X * p.Y * p.Z <= ((size_t)1 << (split_log2 > 0 ? split_log2 : 26)))
        p.flags |= 8u;
    static const bool force_split = experiment_flag("ARVX_FORCE_SPLIT2");  // every item in 2 parts
    if (blocks && force_split) p.flags |= 8u | 64u;
    static const bool no_block_tests = experiment_flag("ARVX_NO_BLOCK_TESTS");
    if (no_block_tests) p.flags |= 32u;
    // (experiment builds: the block-mapped exact kernel counts its items, listed views, (item, view)
    // pairs and projected blocks into the statistics words -- read with arvx_get_stats)
    static const bool count_blocks = experiment_flag("ARVX_COUNT_BLOCKS");
    if (count_blocks && blocks) {
        p.flags |= 256u;
        ARVX_HIP(hipMemsetAsync(ctx->stats(), 0, 64, ctx->stream));
    }
    if (split) {
        // coarse tiles: classified, and the decided ones written as constant records, one
        // workgroup each
        // (lazy: carve_coarse_kernel above did everything)
        if (!lazy)
            ARVX_TRY(launch(ctx, two_launches ? arvx::carve_fill_kernel : arvx::carve_coarse_fill_kernel,
                            (unsigned)ncoarse, 256, p));
        // the others: a fixed grid walks the list (8 waves per SIMD)
        static const int cgrid_env = experiment_int("ARVX_CLASSIFY_WGS");
        const unsigned cgrid = cgrid_env > 0 ? (unsigned)cgrid_env : (unsigned)ncu * 8u;
#ifndef ARVX_CLASSIFY_SPARSE  // (A/B builds: the wave-per-sub-tile kernel everywhere)
        // (the statistics counters live in the other kernel; below 2^26 voxels there are too few
        // listed coarse tiles for a workgroup each: 256^3 +2.5 % with the dense kernel, 512^3
        // -1.5 %, 768^3 -5 %, 1024^3 -11 %)
        const bool dense = !(flags & ARVX_CARVE_STATS) &&
                           ((flags & ARVX_CARVE_DENSE_CLASSIFY) || (size_t)p.X * p.Y * p.Z >= ((size_t)1 << 26));
#else
        const bool dense = false;
#endif
        // the exact kernel's block rectangles from the context's table, once it stands: for the
        // carves that run the instantiation that reads it (a fresh model, items not shared)
        if (dense && blocks && fresh && !(p.flags & 8u) && rec == ctx->rec()) {
            if (int rc = rect_cache_prepare(ctx, p)) return rc;
        } else {
            ctx->rect_streak = 0;
        }
        if (dense)  // one workgroup per listed coarse tile and turn
            ARVX_TRY(launch(ctx, arvx::carve_classify_dense_kernel,
                            (unsigned)ncu * (unsigned)ARVX_DENSE_WGS_PER_CU, 256, p));
        else
            ARVX_TRY(launch(ctx, arvx::carve_classify_kernel, cgrid, 256, p));
        const unsigned pgrid = (unsigned)(p.nwaves / 4);
#ifdef ARVX_TIMELINE
        if (int rc = timeline(ctx, (size_t)pgrid * 4, 64, p)) return rc;  // one record per WAVE of the persistent kernel
#endif
        const bool left = ctx->assoc == ARVX_ASSOC_LEFT;
        const bool may_split = p.flags & 8u;
        // the block tests from the table: the large grids' fresh instantiations only
        bool cached = blocks && fresh && !may_split && p.rcBlk;
#ifdef ARVX_EXPERIMENTS
        if (flags & ARVX_CARVE_FILTER) cached = false;
        // the fp32 filter in front of the exact projection (carve_kernels.h, filtered_view_blocks):
        // for callers whose masks leave most blocks of an item to be projected (ARVX_CARVE_FILTER)
        const bool filter = (flags & ARVX_CARVE_FILTER) != 0;
#endif
        // ... and the pixels from theirs, where that stands too
        const bool pixels = cached && p.pxTab && !no_block_tests;
        // the exact kernel's instantiation: that of the first line whose condition holds
        void (*exact)(arvx::CarveParams) =
#ifdef ARVX_EXPERIMENTS
            blocks && filter && left && may_split ? arvx::carve_exact_blocks_kernel<true, true, false, true>
            : blocks && filter && left && fresh   ? arvx::carve_exact_blocks_kernel<true, false, true, true>
            : blocks && filter && left            ? arvx::carve_exact_blocks_kernel<true, false, false, true>
            : blocks && filter && may_split       ? arvx::carve_exact_blocks_kernel<false, true, false, true>
            : blocks && filter && fresh           ? arvx::carve_exact_blocks_kernel<false, false, true, true>
            : blocks && filter                    ? arvx::carve_exact_blocks_kernel<false, false, false, true>
            :
#endif
            pixels && left                ? arvx::carve_exact_blocks_kernel<true, false, true, false, true, true>
            : pixels                      ? arvx::carve_exact_blocks_kernel<false, false, true, false, true, true>
            : cached && left              ? arvx::carve_exact_blocks_kernel<true, false, true, false, true>
            : cached                      ? arvx::carve_exact_blocks_kernel<false, false, true, false, true>
            : blocks && left && may_split ? arvx::carve_exact_blocks_kernel<true, true>
            : blocks && left && fresh     ? arvx::carve_exact_blocks_kernel<true, false, true>
            : blocks && left              ? arvx::carve_exact_blocks_kernel<true, false>
            : blocks && may_split         ? arvx::carve_exact_blocks_kernel<false, true>
            : blocks && fresh             ? arvx::carve_exact_blocks_kernel<false, false, true>
            : blocks                      ? arvx::carve_exact_blocks_kernel<false, false>
            : left                        ? arvx::carve_exact_kernel<true>
                                          : arvx::carve_exact_kernel<false>;
        ARVX_TRY(launch(ctx, exact, pgrid, 256, p));
        ctx->carve_layout = layout_when_done;
        ++ctx->carve_seq;
        // (arvx_last_carve_path: all of it once every launch is out, or nothing)
        ctx->path_bits = (dense ? ARVX_PATH_DENSE_CLASSIFY : 0u) | (may_split ? ARVX_PATH_ITEM_SHARING : 0u) |
                         (fresh ? ARVX_PATH_FRESH : 0u) | (lazy ? ARVX_PATH_LAZY_CODES : 0u) |
                         (cached ? ARVX_PATH_RECT_BLOCKS : 0u) | (pixels ? ARVX_PATH_PIXEL_TABLE : 0u);
        ctx->path_dense_grid = dense ? (unsigned)ncu * (unsigned)ARVX_DENSE_WGS_PER_CU : 0u;
        ctx->path_off_listed = (size_t)((uint8_t *)p.undecidedCount - (uint8_t *)ctx->pool_coarse.p);
        ctx->path_off_work = (size_t)((uint8_t *)p.workCount - (uint8_t *)ctx->pool_coarse.p);
        if (lazy && rec == ctx->rec()) ctx->form = Form::Lazy;
        if (p.cstate) ctx->cstate_tiles = ncoarse;
        return ARVX_OK;
    }
#ifdef ARVX_TIMELINE
    if (int rc = timeline(ctx, grid, 32, p)) return rc;
#endif
    ARVX_TRY(launch(ctx, ctx->assoc == ARVX_ASSOC_LEFT ? arvx::carve_fused_kernel<true> : arvx::carve_fused_kernel<false>,
                    grid, 256, p));
    ctx->path_bits = (cull ? ARVX_PATH_FUSED : ARVX_PATH_BRUTE_FORCE) | (fresh ? ARVX_PATH_FRESH : 0u);
    ctx->rect_streak = 0;
    return ARVX_OK;
}

int arvx_carve_views(arvx_ctx *ctx, int first, int count, unsigned flags) {
    ARVX_CHECK_CTX(ctx);
    if (!ctx->views_ready) return fail(ARVX_ERR_STATE, "arvx_set_views has not been called");
    if (first < 0 || count < 0 || first + count > ctx->V)
        return fail(ARVX_ERR_INVALID, "view range [%d,%d) outside [0,%d)", first, first + count,
                    ctx->V);
    if (count == 0) return ARVX_OK;
#ifndef ARVX_EXPERIMENTS
    if (flags & ARVX_CARVE_STREAM)  // (refused before anything about the context changes)
        return fail(ARVX_ERR_INVALID, "ARVX_CARVE_STREAM: the one-launch carve is only in -DARVX_EXPERIMENTS "
                                      "builds (libarvx_experiments.so)");
    if (flags & ARVX_CARVE_FILTER)
        return fail(ARVX_ERR_INVALID, "ARVX_CARVE_FILTER: the fp32 projection filter is only in "
                                      "-DARVX_EXPERIMENTS builds (libarvx_experiments.so)");
#endif
    ctx->drop(Event::Carve);
    const bool fresh = ctx->form == Form::Fresh;
    if (fresh) {  // the kernels write every record of the grid; nothing is read
        if (int rc = ensure_records(ctx, ctx->pool_rec)) return rc;
    } else if (int rc = need_rec(ctx)) {
        return rc;
    }
    ctx->form = Form::Records;  // (Lazy once the launches are out, where the carve leaves codes)
    return launch_carve(ctx, ctx->rec(), first, count, flags, fresh);
}

int arvx_carve(arvx_ctx *ctx, unsigned flags) {
    if (!ctx) return fail(ARVX_ERR_INVALID, "null context");
    return arvx_carve_views(ctx, 0, ctx->V, flags);
}

int arvx_last_carve_path(arvx_ctx *ctx, uint32_t out[4]) {
    ARVX_CHECK_CTX(ctx);
    if (!out) return fail(ARVX_ERR_INVALID, "null out");
    out[0] = ctx->path_bits;
    out[1] = out[3] = 0;
    out[2] = ctx->path_dense_grid;
    ARVX_SYNC(ctx);
    if (!ctx->path_off_listed) return ARVX_OK;  // no list, no queues (or no carve yet)
    int listed = 0;
    int counts[arvx::kWorkLists];  // (one padded counter per list: gathered by a strided copy)
    const uint8_t *base = (const uint8_t *)ctx->pool_coarse.p;
    ARVX_HIP(hipMemcpy(&listed, base + ctx->path_off_listed, sizeof listed, hipMemcpyDeviceToHost));
    ARVX_HIP(hipMemcpy2D(counts, sizeof(int), base + ctx->path_off_work, arvx::kCounterStride * sizeof(int),
                         sizeof(int), arvx::kWorkLists, hipMemcpyDeviceToHost));
    uint64_t items = 0;
    for (int l = 0; l < arvx::kWorkLists; ++l) items += (uint64_t)counts[l];
    out[1] = (uint32_t)listed;
    out[3] = (uint32_t)items;
    return ARVX_OK;
}

// ---- vote carve (vote_kernels.h) ----------------------------------------------------------------

int arvx_carve_votes(arvx_ctx *ctx, int max_misses, unsigned flags) {
    ARVX_CHECK_CTX(ctx);
    if (!ctx->views_ready) return fail(ARVX_ERR_STATE, "arvx_set_views (with masks) has not been called");
    if (!whole_grid(ctx)) return fail(ARVX_ERR_STATE, "arvx_carve_votes needs a whole-grid context");
    if (max_misses < 0 || max_misses > 65535)
        return fail(ARVX_ERR_INVALID, "max_misses %d: must be in [0, 65535]", max_misses);
    if (ctx->V > 65535) return fail(ARVX_ERR_INVALID, "%d views: the counts are 16 bits wide", ctx->V);
    if (flags & ~(ARVX_VOTES_COUNTS | ARVX_VOTES_NO_CULL))
        return fail(ARVX_ERR_INVALID, "unknown flag bits 0x%x", flags & ~(ARVX_VOTES_COUNTS | ARVX_VOTES_NO_CULL));
    const size_t half = (ctx->nvox * sizeof(uint16_t) + 255) / 256 * 256;
    if (flags & ARVX_VOTES_COUNTS) ARVX_HIP(ctx->pool_votes.reserve(2 * half));
    // A carve as far as the context's other results go: the call only empties voxels and sets seen
    // bits, so what earlier carves settled for whole coarse tiles (cstate: all carved and seen / all
    // seen) stays true and is kept, as arvx_carve keeps it.
    ctx->drop(Event::Carve);
    const bool fresh = ctx->form == Form::Fresh;
    if (fresh) {  // the kernel writes every record of the grid; nothing is read
        if (int rc = ensure_records(ctx, ctx->pool_rec)) return rc;
    } else if (int rc = need_rec(ctx)) {  // (a lazily coded state is written out first)
        return rc;
    }
    ctx->form = Form::Records;
    arvx::VoteCarveParams q;
    arvx::CarveParams &p = q.g;
    p = record_params(ctx);
    p.ccode = nullptr;
    carve_views(ctx, p);
    p.v0 = 0;
    p.v1 = ctx->V;
    p.flags = fresh ? 4u : 0u;
    q.bg = (flags & ARVX_VOTES_COUNTS) ? (uint16_t *)ctx->pool_votes.p : nullptr;
    q.in = (flags & ARVX_VOTES_COUNTS) ? (uint16_t *)((uint8_t *)ctx->pool_votes.p + half) : nullptr;
    q.max_misses = max_misses;
    q.cull = (flags & ARVX_VOTES_NO_CULL) ? 0 : 1;
    const size_t rows8 = ((size_t)p.tilesY * p.tilesZ + 7) / 8 * 8;
    const unsigned grid = (unsigned)(rows8 * p.tilesX);
    ARVX_TRY(by_assoc(ctx, [&](auto left) {
        return launch(ctx, arvx::carve_votes_kernel<decltype(left)::value>, grid, 256, q);
    }));
    ctx->votes_ready = (flags & ARVX_VOTES_COUNTS) != 0;
    return ARVX_OK;
}

int arvx_votes_download(arvx_ctx *ctx, uint16_t *background, uint16_t *inside) {
    ARVX_CHECK_CTX(ctx);
    if (!ctx->votes_ready)
        return fail(ARVX_ERR_STATE, "no counts: arvx_carve_votes with ARVX_VOTES_COUNTS has not run since the "
                                    "state or the views were last replaced");
    const size_t bytes = ctx->nvox * sizeof(uint16_t);
    const size_t half = (bytes + 255) / 256 * 256;
    if (background)
        ARVX_HIP(hipMemcpyAsync(background, ctx->pool_votes.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (inside)
        ARVX_HIP(hipMemcpyAsync(inside, (const uint8_t *)ctx->pool_votes.p + half, bytes, hipMemcpyDeviceToHost,
                                ctx->stream));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

static int surf_host(Ctx *ctx);
static int clo_host(Ctx *ctx);
static void owned_part(const Ctx *ctx, const std::vector<int> &idx, size_t &lo, size_t &hi,
                       long long &base);
// a context without halo planes owns every entry of its lists: their lengths need no host copy
static bool owns_all_planes(const Ctx *ctx) { return ctx->z0 == ctx->ze0 && ctx->z1 == ctx->ze1; }

int arvx_get_stats(arvx_ctx *ctx, arvx_stats *out) {
    ARVX_CHECK_CTX(ctx);
    if (!out) return fail(ARVX_ERR_INVALID, "null out");
    unsigned long long h[8];
    ARVX_HIP(hipMemcpyAsync(h, ctx->stats(), sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    ARVX_SYNC(ctx);
    memset(out, 0, sizeof *out);
    out->subtiles = h[0];
    out->subtiles_carved = h[1];
    out->subtile_views_mixed = h[2];
    out->subtile_views_total = h[3];
    out->surface_voxels = 0;
    if (ctx->color_ready && owns_all_planes(ctx)) {
        out->surface_voxels = (unsigned long long)ctx->surf_count;
    } else if (ctx->color_ready) {  // the owned part of the colour pass's list (arvx_color)
        if (int rc = surf_host(ctx)) return rc;
        size_t lo, hi;
        long long base;
        owned_part(ctx, ctx->h_surf_index, lo, hi, base);
        out->surface_voxels = hi - lo;
    }
    out->reserved[0] = h[5];  // 256-voxel slices evaluated exactly
    out->reserved[1] = h[6];  // voxels among them that were not yet carved+seen
    out->reserved[2] = h[7];  // mixed pairs whose open voxels all got the same answer
    out->host_total_fallbacks = ctx->host_total_fallbacks;
    return ARVX_OK;
}

// Which planes (global z, [lo, hi)) a context's stages work on.  Colours: every plane whose two
// neighbour planes the records hold (a voxel is on the surface or not by its six neighbours).
// Closure with radius r: every plane whose 2 r neighbour planes have colours.  A whole-grid
// context and the sides of a slab that touch the grid's faces lose nothing.
static void stage_ranges(const Ctx *ctx, int radius, int &c_lo, int &c_hi, int &f_lo, int &f_hi) {
    c_lo = ctx->ze0 > 0 ? ctx->ze0 + 1 : 0;
    c_hi = ctx->ze1 < ctx->Z ? ctx->ze1 - 1 : ctx->Z;
    f_lo = c_lo > 0 ? c_lo + radius : 0;
    f_hi = c_hi < ctx->Z ? c_hi - radius : ctx->Z;
}
// the entries [lo, hi) of an ascending index list over the context's planes that lie in the
// owned planes; base = what to subtract to number them over the owned planes
static void owned_part(const Ctx *ctx, const std::vector<int> &idx, size_t &lo, size_t &hi,
                       long long &base) {
    const long long plane = (long long)ctx->X * ctx->Y;
    base = plane * (ctx->z0 - ctx->ze0);
    const long long end = plane * (ctx->z1 - ctx->ze0);
    lo = (size_t)(std::lower_bound(idx.begin(), idx.end(), base,
                                   [](int a, long long b) { return (long long)a < b; }) - idx.begin());
    hi = (size_t)(std::lower_bound(idx.begin(), idx.end(), end,
                                   [](int a, long long b) { return (long long)a < b; }) - idx.begin());
}

// ---- colour pass -----------------------------------------------------------------

// n host images of the views' size (BGR, rows of `stride` bytes), tightly packed into dst
static int images_upload(Ctx *ctx, uint8_t *dst, const uint8_t *const *images, int n, size_t stride) {
    const size_t rowb = (size_t)ctx->W * 3, img = rowb * ctx->H;
    bool packed = stride == rowb;  // all of them back to back in host memory: one copy
    for (int i = 1; i < n && packed; ++i) packed = images[i] == images[i - 1] + img;
    if (packed) {
        ARVX_HIP(hipMemcpyAsync(dst, images[0], img * n, hipMemcpyHostToDevice, ctx->stream));
    } else {
        for (int i = 0; i < n; ++i)
            ARVX_HIP(hipMemcpy2DAsync(dst + img * i, rowb, images[i], stride, rowb, ctx->H, hipMemcpyHostToDevice,
                                      ctx->stream));
    }
    return ARVX_OK;
}

int arvx_set_images(arvx_ctx *ctx, const uint8_t *const *images, size_t stride) {
    ARVX_CHECK_CTX(ctx);
    if (!ctx->cameras_ready) return fail(ARVX_ERR_STATE, "arvx_set_views must come first");
    if (!images) return fail(ARVX_ERR_INVALID, "null images");
    const size_t rowb = (size_t)ctx->W * 3;
    if (stride < rowb) return fail(ARVX_ERR_INVALID, "stride %zu < W*3", stride);
    for (int i = 0; i < ctx->V; ++i)
        if (!images[i]) return fail(ARVX_ERR_INVALID, "null image %d", i);
    const size_t img = rowb * ctx->H;
    ctx->drop(Event::SetImages);
    ARVX_HIP(ctx->pool_images.reserve(img * ctx->V));
    ARVX_TRY(images_upload(ctx, ctx->images(), images, ctx->V, stride));
    ARVX_SYNC(ctx);
    ctx->images_ready = true;
    return ARVX_OK;
}

// ---- silhouettes from the photographs (segment_kernels.h) -------------------------------------

// pixels whose labels and areas (an int32 each) one batch of views may hold: 1 GiB; a single view
// larger than that is a batch of its own (W, H <= kMaxImageDim: 2^28 pixels, int32 indices still)
static constexpr long long kSegBatchPixels = 1ll << 27;

static int segment_refusals(int V, const void *images, int W, int H, const void *plates, int plate_count,
                            const arvx_segment_params *p) {
    if (!images || !p) return fail(ARVX_ERR_INVALID, "null argument");
    // (views_common's ranges, before anything is read through V, W or H)
    if (V < 1 || V > 4096) return fail(ARVX_ERR_INVALID, "V=%d out of range [1,4096]", V);
    if (W < 1 || H < 1 || W > arvx::kMaxImageDim || H > arvx::kMaxImageDim)
        return fail(ARVX_ERR_INVALID, "image size %dx%d out of range", W, H);
    if (p->rule != ARVX_SEGMENT_RANGE && p->rule != ARVX_SEGMENT_PLATE)
        return fail(ARVX_ERR_INVALID, "unknown segmentation rule %d", p->rule);
    for (int c = 0; c < 3; ++c)
        if (p->lo[c] > p->hi[c]) return fail(ARVX_ERR_INVALID, "lo[%d] > hi[%d]", c, c);
    if (p->threshold < 0 || p->threshold > 255)
        return fail(ARVX_ERR_INVALID, "threshold %d outside [0,255]", p->threshold);
    if (p->rule == ARVX_SEGMENT_PLATE) {
        if (!plates) return fail(ARVX_ERR_INVALID, "ARVX_SEGMENT_PLATE: null plates");
        if (plate_count != 1 && plate_count != V)
            return fail(ARVX_ERR_INVALID, "plate_count %d is neither 1 nor V", plate_count);
    }
    if (p->open_radius < 0 || p->close_radius < 0) return fail(ARVX_ERR_INVALID, "negative radius");
    if (p->min_area < 0) return fail(ARVX_ERR_INVALID, "negative min_area");
    if (p->flags & ~ARVX_SEGMENT_LARGEST) return fail(ARVX_ERR_INVALID, "unknown flag bits %#x", p->flags);
    return ARVX_OK;
}

// One row or column pass of a box erosion (op_and) or dilation of radius r: *cur holds the result, *tmp
// what is left over.  Radii up to 8 combine their 2 r + 1 shifts in one launch; larger ones double a
// forward window up to r + 1 pixels, then a backward one over that -- together [-r, r], every partial
// window starting inside the image, so that "outside" never stands for pixels of the image.
static int segment_pass(Ctx *ctx, const arvx::BitGrid &g, unsigned long long **cur, unsigned long long **tmp,
                        int r, bool along_x, int op_and) {
    r = std::min(r, (along_x ? g.X : g.Y) - 1);  // (a window beyond the image adds the identity)
    if (r <= 0) return ARVX_OK;
    const unsigned grid = blocks_for(bit_words(g));
    const auto step = [&](int n, int s0, int ds) {
        const int rc = launch(ctx, arvx::seg_combine_kernel, grid, 256, *cur, *tmp, g, op_and, n, along_x ? s0 : 0,
                              along_x ? ds : 0, along_x ? 0 : s0, along_x ? 0 : ds);
        std::swap(*cur, *tmp);
        return rc;
    };
    if (r <= 8) return step(2 * r + 1, -r, 1);
    for (int dir = 1; dir >= -1; dir -= 2) {
        int len = 1;
        for (; 2 * len <= r + 1; len *= 2) ARVX_TRY(step(2, 0, dir * len));
        if (len < r + 1) ARVX_TRY(step(2, 0, dir * (r + 1 - len)));
    }
    return ARVX_OK;
}

static int segment_box(Ctx *ctx, const arvx::BitGrid &g, unsigned long long **cur, unsigned long long **tmp, int r,
                       int op_and) {
    ARVX_TRY(segment_pass(ctx, g, cur, tmp, r, true, op_and));
    return segment_pass(ctx, g, cur, tmp, r, false, op_and);
}

// The components of one kind (1 foreground, 2 background) of the views v0 .. v0 + gb.Z - 1 of `plane`:
// labels, then areas
static int segment_label(Ctx *ctx, const arvx::BitGrid &gb, const unsigned long long *plane, int which, int *L,
                         unsigned *area) {
    const size_t n = (size_t)gb.X * gb.Y * gb.Z;
    const unsigned lanes = blocks_for(bit_words(gb) * 64);
    ARVX_TRY(launch(ctx, arvx::seg_init_kernel, lanes, 256, plane, gb, which, L));
    ARVX_TRY(launch(ctx, arvx::seg_link_kernel, lanes, 256, plane, gb, which, L));
    ARVX_TRY(launch(ctx, arvx::seg_roots_kernel, blocks_for(n), 256, L, (int)n));
    ARVX_HIP(hipMemsetAsync(area, 0, n * sizeof(unsigned), ctx->stream));
    return launch(ctx, arvx::seg_area_kernel, blocks_for(n, arvx::kSegAreaBlock), arvx::kSegAreaBlock, L, (int)n, gb.X,
                  gb.Y, area);
}

// The stage behind both entry points: the images are in pool_images, views_common has run.
static int segment_run(Ctx *ctx, const uint8_t *d_plates, int plate_count, const arvx_segment_params &p) {
    const int V = ctx->V, W = ctx->W, H = ctx->H;
    const arvx::BitGrid g{W, H, V, (W + 63) / 64};
    const size_t words = bit_words(g), view_words = (size_t)g.XW * H;
    ARVX_HIP(ctx->pool_seg_planes.reserve(2 * words * sizeof(unsigned long long)));
    ARVX_HIP(ctx->pool_seg_counts.reserve((size_t)V * 8 * sizeof(unsigned long long)));
    unsigned long long *plane0 = (unsigned long long *)ctx->pool_seg_planes.p;
    unsigned long long *cur = plane0, *tmp = plane0 + words;
    unsigned long long *counts = (unsigned long long *)ctx->pool_seg_counts.p;
    ARVX_HIP(hipMemsetAsync(counts, 0, (size_t)V * 8 * sizeof(unsigned long long), ctx->stream));
    const dim3 count_grid(blocks_for(view_words), V);

    // 1. the rule
    arvx::SegRule rule{p.rule, 0u, 0u, p.threshold};
    for (int c = 0; c < 3; ++c) {
        rule.lo |= (uint32_t)p.lo[c] << (8 * c);
        rule.hi |= (uint32_t)p.hi[c] << (8 * c);
    }
    ARVX_TRY(launch(ctx, arvx::seg_rule_kernel, blocks_for(words * 16), 256, ctx->images(), d_plates,
                    plate_count == 1 ? (size_t)0 : (size_t)W * H * 3, g, rule, cur));
    ARVX_TRY(launch(ctx, arvx::seg_count_kernel, count_grid, 256, cur, g, counts, 0));
    // 2. opening, 3. closing
    ARVX_TRY(segment_box(ctx, g, &cur, &tmp, p.open_radius, 1));
    ARVX_TRY(segment_box(ctx, g, &cur, &tmp, p.open_radius, 0));
    ARVX_TRY(segment_box(ctx, g, &cur, &tmp, p.close_radius, 0));
    ARVX_TRY(segment_box(ctx, g, &cur, &tmp, p.close_radius, 1));
    ARVX_TRY(launch(ctx, arvx::seg_count_kernel, count_grid, 256, cur, g, counts, 1));

    // 4. specks and 5. holes: each labels its own kind of pixel, batch by batch -- the holes on the plane
    // the specks left, so that background a removed speck joined is one component
    const int largest = (p.flags & ARVX_SEGMENT_LARGEST) ? 1 : 0;
    const long long bound = std::max(1ll, kSegBatchPixels / ((long long)W * H));
    const int per_batch = (int)std::min<long long>(ctx->seg_batch > 0 ? std::min<long long>(ctx->seg_batch, bound) : bound, V);
    const bool specks = p.min_area > 0 || largest, holes = p.max_hole != 0;
    int *L = nullptr;
    unsigned *area = nullptr;
    unsigned long long *best = nullptr;
    if (specks || holes) {
        const size_t n = (size_t)per_batch * W * H;
        ARVX_HIP(ctx->pool_seg_label.reserve(2 * n * sizeof(int) + (size_t)per_batch * sizeof(unsigned long long)));
        best = (unsigned long long *)ctx->pool_seg_label.p;  // (first: 8-byte aligned whatever n is)
        L = (int *)(best + per_batch);
        area = (unsigned *)(L + n);
    }
    for (int step = 4; step <= 5; ++step) {
        if (step == 4 ? specks : holes)
            for (int v0 = 0; v0 < V; v0 += per_batch) {
                const arvx::BitGrid gb{W, H, std::min(per_batch, V - v0), g.XW};
                unsigned long long *plane = cur + (size_t)v0 * view_words;
                const size_t n = (size_t)W * H * gb.Z;
                const unsigned lanes = blocks_for(bit_words(gb) * 64);
                ARVX_TRY(segment_label(ctx, gb, plane, step == 4 ? 1 : 2, L, area));
                if (step == 4) {
                    if (largest) {
                        ARVX_HIP(hipMemsetAsync(best, 0, (size_t)gb.Z * sizeof(unsigned long long), ctx->stream));
                        ARVX_TRY(launch(ctx, arvx::seg_best_kernel, blocks_for(n), 256, L, area, (int)n, W * H,
                                        (long long)p.min_area, best));
                    }
                    ARVX_TRY(launch(ctx, arvx::seg_specks_kernel, lanes, 256, plane, gb, L, area,
                                    (long long)p.min_area, largest, best, counts + 8 * (size_t)v0));
                } else {
                    ARVX_TRY(launch(ctx, arvx::seg_holes_kernel, lanes, 256, plane, gb, L, area,
                                    (long long)p.max_hole, counts + 8 * (size_t)v0));
                }
            }
        ARVX_TRY(launch(ctx, arvx::seg_count_kernel, count_grid, 256, cur, g, counts, step - 2));
    }
    ctx->seg_final = cur == plane0 ? 0 : 1;

    // the views: the flat background plane, then whole tables from it
    ARVX_TRY(launch(ctx, arvx::seg_publish_kernel, dim3(blocks_for((size_t)ctx->bgWords), V), 256, cur, g,
                    ctx->bg(), ctx->bgWords));
    ARVX_TRY(views_windows(ctx, false));
    ARVX_TRY(views_tables_from_bits(ctx));
    ctx->views_ready = true;
    ctx->cameras_ready = true;
    ctx->images_ready = true;
    ctx->seg_ready = true;
    return ARVX_OK;
}

int arvx_segment_views(arvx_ctx *ctx, int V, const float *M, const float *campos, const uint8_t *const *images,
                       int W, int H, size_t stride, const uint8_t *const *plates, int plate_count,
                       const arvx_segment_params *params) {
    ARVX_CHECK_CTX(ctx);
    ARVX_TRY(segment_refusals(V, images, W, H, plates, plate_count, params));
    const bool plate = params->rule == ARVX_SEGMENT_PLATE;
    if (W >= 1 && stride < (size_t)W * 3) return fail(ARVX_ERR_INVALID, "stride %zu < W*3", stride);
    for (int i = 0; i < V; ++i)
        if (!images[i]) return fail(ARVX_ERR_INVALID, "null image %d", i);
    for (int i = 0; plate && i < plate_count; ++i)
        if (!plates[i]) return fail(ARVX_ERR_INVALID, "null plate %d", i);
    ARVX_TRY(views_common(ctx, V, M, campos, W, H, 1));
    ctx->drop(Event::SetImages);
    const size_t rowb = (size_t)W * 3, img = rowb * H;
    ARVX_HIP(ctx->pool_images.reserve(img * V));
    ARVX_TRY(images_upload(ctx, ctx->images(), images, V, stride));
    if (plate) {
        ARVX_HIP(ctx->pool_seg_plates.reserve(img * plate_count));
        ARVX_TRY(images_upload(ctx, (uint8_t *)ctx->pool_seg_plates.p, plates, plate_count, stride));
    }
    ARVX_TRY(segment_run(ctx, plate ? (const uint8_t *)ctx->pool_seg_plates.p : nullptr, plate_count, *params));
    ARVX_SYNC(ctx);  // host buffers may go away
    return ARVX_OK;
}

int arvx_segment_views_device(arvx_ctx *ctx, int V, const float *M, const float *campos, const void *dev_images,
                              int W, int H, const void *dev_plates, int plate_count,
                              const arvx_segment_params *params) {
    ARVX_CHECK_CTX(ctx);
    ARVX_TRY(segment_refusals(V, dev_images, W, H, dev_plates, plate_count, params));
    ARVX_TRY(views_common(ctx, V, M, campos, W, H, 1));
    ctx->drop(Event::SetImages);
    const size_t bytes = (size_t)W * H * 3 * V;
    ARVX_HIP(ctx->pool_images.reserve(bytes));
    ARVX_HIP(hipMemcpyAsync(ctx->images(), dev_images, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return segment_run(ctx, params->rule == ARVX_SEGMENT_PLATE ? (const uint8_t *)dev_plates : nullptr, plate_count,
                       *params);
}

static int segment_result(Ctx *ctx, int view, const void *out) {
    if (!ctx->seg_ready || !ctx->views_ready)
        return fail(ARVX_ERR_STATE, "the views are not those of an arvx_segment_views call");
    if (view < 0 || view >= ctx->V) return fail(ARVX_ERR_INVALID, "view %d outside [0,%d)", view, ctx->V);
    if (!out) return fail(ARVX_ERR_INVALID, "null argument");
    return ARVX_OK;
}

int arvx_segment_download(arvx_ctx *ctx, int view, uint8_t *mask) {
    ARVX_CHECK_CTX(ctx);
    ARVX_TRY(segment_result(ctx, view, mask));
    const arvx::BitGrid g{ctx->W, ctx->H, ctx->V, (ctx->W + 63) / 64};
    const size_t npix = (size_t)ctx->W * ctx->H;
    ARVX_HIP(ctx->pool_seg_bytes.reserve(npix));
    const unsigned long long *plane = (const unsigned long long *)ctx->pool_seg_planes.p + ctx->seg_final * bit_words(g);
    ARVX_TRY(launch(ctx, arvx::seg_bytes_kernel, blocks_for(npix), 256, plane, g, view, (uint8_t *)ctx->pool_seg_bytes.p));
    ARVX_HIP(hipMemcpyAsync(mask, ctx->pool_seg_bytes.p, npix, hipMemcpyDeviceToHost, ctx->stream));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

int arvx_segment_counts(arvx_ctx *ctx, int view, int64_t out[8]) {
    ARVX_CHECK_CTX(ctx);
    ARVX_TRY(segment_result(ctx, view, out));
    ARVX_HIP(hipMemcpyAsync(out, (const unsigned long long *)ctx->pool_seg_counts.p + 8 * (size_t)view,
                            8 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

int arvx_selftest_segment_batch(arvx_ctx *ctx, int views_per_batch) {
    ARVX_CHECK_CTX(ctx);
    if (views_per_batch < 0) return fail(ARVX_ERR_INVALID, "views_per_batch %d (0: the default bound)", views_per_batch);
    ctx->seg_batch = views_per_batch;
    return ARVX_OK;
}

// arvx_color's refusals (arvx_color_visible adds its own after them)
static int color_refusals(Ctx *ctx, int mode) {
    if (!ctx->cameras_ready) return fail(ARVX_ERR_STATE, "arvx_set_views has not been called");
    if (!ctx->images_ready) return fail(ARVX_ERR_STATE, "arvx_set_images has not been called");
    if (!ctx->has_campos) return fail(ARVX_ERR_STATE, "arvx_set_views was given no campos");
    if (mode != ARVX_COLOR_CLOSEST && mode != ARVX_COLOR_AVERAGE)
        return fail(ARVX_ERR_INVALID, "colour mode %d", mode);
    if (ctx->stripe_world > 1)
        return fail(ARVX_ERR_STATE, "the colour pass needs contiguous slabs (neighbour planes)");
    return ARVX_OK;
}

static int launch_visible_vote(Ctx *ctx, const arvx::VoteParams &vp, float tol);

// The geometry, views and images of a colour vote over indices that start at global plane zglob0;
// the list and the outputs are the caller's to fill.
static arvx::VoteParams vote_params(const Ctx *ctx, int zglob0) {
    arvx::VoteParams vp{};
    vp.X = ctx->X;
    vp.Y = ctx->Y;
    vp.zglob0 = zglob0;
    vp.s = ctx->s;
    vp.V = ctx->V;
    vp.W = ctx->W;
    vp.H = ctx->H;
    vp.M = ctx->M();
    vp.campos = ctx->campos();
    vp.images = ctx->images();
    return vp;
}

// The colour pass's list of the current state (arvx_color and arvx_photo_carve's iterations):
// surface = occupied and not inner, on bit planes over the context's planes, for the planes
// [c_lo, c_hi) (stage_ranges): the owned ones and the halo planes whose own neighbours the records
// hold; its ordered compaction goes to pool_surf_index, the plane and its ranks (SparseWord) stay in
// pool_col_bits / pool_col_rank.  The list's length is not known before the compaction has run: the
// kernels stop at the capacity the buffers were sized for, and a list that outgrew it is compacted
// and worked on again with room for all of it (run_lists).  Per attempt:
// reserve(cap) sizes the caller's buffers, enqueue(vp) launches its kernels on the list vp describes
// (length on the device, in vp.n_dev; vp.rgba / depth / has / mode are the caller's to fill), and
// settle() reads what they left after the synchronisation.
extern "C++" {  // (a template, inside the C-ABI's extern "C" block)
template <class Reserve, class Enqueue, class Settle>
static int surface_list(Ctx *ctx, Reserve reserve, Enqueue enqueue, Settle settle, long long *total_out) {
    const int Zext = ctx->ze1 - ctx->ze0;
    int c_lo, c_hi, f_lo, f_hi;
    stage_ranges(ctx, 0, c_lo, c_hi, f_lo, f_hi);
    const arvx::BitGrid gext = bit_grid(ctx, Zext);
    const size_t nw_ext = bit_words(gext);
    // the surface plane stays with the context: with its ranks it is the index of the colour
    // list (closure and mesh look colours up through it)
    ARVX_HIP(ctx->pool_col_bits.reserve(nw_ext * sizeof(unsigned long long)));
    ARVX_HIP(ctx->pool_col_rank.reserve(nw_ext * sizeof(arvx::SparseWord)));
    // ... and so do the occupancy plane and the plane of the voxels no view has seen: a closure that
    // follows -- with nothing but handleUnseen in between, src/main.cpp:282-299 -- starts from them
    // instead of converting the records again (state_planes)
    ARVX_HIP(ctx->pool_state_planes.reserve(2 * nw_ext * sizeof(unsigned long long)));  // (one allocation)
    unsigned long long *d_occ = (unsigned long long *)ctx->pool_state_planes.p;
    unsigned long long *d_surf = (unsigned long long *)ctx->pool_col_bits.p;
    ctx->planes_seq = 0;
    if (int rc = launch_bit_pack(ctx, gext, 0, 1, d_occ, d_occ + nw_ext)) return rc;
    ctx->planes_words = nw_ext;
    ctx->planes_seq = ctx->state_seq;
    ctx->planes_unseen = false;
    // the surface plane of the planes [c_lo, c_hi) (zeros elsewhere) and, per chunk of the
    // compaction, its number of set bits
    int *d_counts = nullptr;
    if (int rc = chunk_counts(ctx, nw_ext, &d_counts)) return rc;
    ARVX_TRY(launch(ctx, arvx::bit_surface_count_kernel, blocks_for(nw_ext), 256, d_occ, gext, c_lo - ctx->ze0,
                    c_hi - ctx->ze0, d_surf, d_counts));
    const double v = (double)ctx->X * ctx->Y * Zext;
    ListRoom lists[] = {{Ctx::kSurface, list_cap(ctx->pool_surf_index, sizeof(int), first_list_cap(v, v)), 0}};
    const long long &cap = lists[0].cap;
    auto attempt = [&]() -> int {
        ARVX_HIP(ctx->pool_surf_index.reserve((size_t)cap * sizeof(int)));
        ctx->d_surf_index = (int *)ctx->pool_surf_index.p;
        if (int rc = reserve(cap)) return rc;
        const long long *d_total = nullptr;
        if (int rc = bit_compact(ctx, d_surf, nw_ext, gext, cap, ctx->d_surf_index,
                                 (arvx::SparseWord *)ctx->pool_col_rank.p, Ctx::kSurface, &d_total))
            return rc;
        arvx::VoteParams vp = vote_params(ctx, ctx->ze0);  // (list indices run over the context's planes)
        vp.index = ctx->d_surf_index;
        vp.n = cap;
        vp.n_dev = d_total;
        return enqueue(vp);
    };
    if (int rc = run_lists(ctx, lists, attempt, settle)) return rc;
    *total_out = lists[0].total;
    return ARVX_OK;
}
}  // extern "C++"

// The colour pass of arvx_color (visible = false) and arvx_color_visible (visible = true: the
// depth buffers, then the visible vote, in place of color_vote_kernel).
static int color_pass(Ctx *ctx, int mode, bool visible, float tol) {
    ctx->drop(Event::Color);
    auto reserve = [&](long long cap) -> int {
        ARVX_HIP(ctx->pool_surf_rgb.reserve((size_t)cap * sizeof(float4)));
        ctx->d_surf_rgba = (float4 *)ctx->pool_surf_rgb.p;
        ARVX_HIP(ctx->pool_surf_depth.reserve((size_t)cap * sizeof(float)));
        ctx->d_surf_depth = (float *)ctx->pool_surf_depth.p;
        ARVX_HIP(ctx->pool_surf_has.reserve((size_t)cap));
        ctx->d_surf_has = (uint8_t *)ctx->pool_surf_has.p;
        if (visible) ARVX_HIP(ctx->pool_vis_views.reserve((size_t)cap * sizeof(int)));
        return ARVX_OK;
    };
    auto enqueue = [&](arvx::VoteParams vp) -> int {
        vp.mode = mode;
        vp.rgba = ctx->d_surf_rgba;
        vp.depth = ctx->d_surf_depth;
        vp.has = ctx->d_surf_has;
        if (visible) return launch_visible_vote(ctx, vp, tol);
        return by_assoc(ctx, [&](auto left) {
            return launch(ctx, arvx::color_vote_kernel<decltype(left)::value>, blocks_for(vp.n), 256, vp);
        });
    };
    auto settle = [&]() -> int {
        if (visible && ctx->word(Ctx::kVisNeed) >= 0) ctx->vis_large_need = ctx->word(Ctx::kVisNeed);
        return ARVX_OK;
    };
    long long total = 0;
    if (int rc = surface_list(ctx, reserve, enqueue, settle, &total)) return rc;
    ctx->surf_count = total;
    ctx->surf_host_count = -1;  // the host copies of the list are fetched when somebody asks
    if (total == 0) {
        ctx->d_surf_index = nullptr;
        ctx->d_surf_rgba = nullptr;
        ctx->d_surf_depth = nullptr;
        ctx->d_surf_has = nullptr;
    }
    ctx->color_ready = true;
    ctx->color_visible = visible;
    // (arvx_get_stats' surface_voxels: the owned part of the list, counted when it is asked for)
    return ARVX_OK;
}

int arvx_color(arvx_ctx *ctx, int mode) {
    ARVX_CHECK_CTX(ctx);
    if (int rc = color_refusals(ctx, mode)) return rc;
    return color_pass(ctx, mode, false, 0.f);
}

// The depth buffers of the views (clear, splat, large footprints) of the list of `cap` entries at
// `index` (its length on the device, *n_dev): no synchronisation.  The sweep leaves the number of
// large footprints it wanted in the count word kVisNeed (the caller hands it on to vis_large_need).
static int launch_depth_buffers(Ctx *ctx, const int *index, long long cap, const long long *n_dev,
                                uint32_t **zbuf_out) {
    ctx->word(Ctx::kVisNeed) = -1;
    const size_t plane = (size_t)ctx->W * ctx->H, nz = plane * ctx->V;
    ARVX_HIP(ctx->pool_vis_depth.reserve(nz * sizeof(uint32_t)));
    const unsigned large_cap = large_list_cap(cap, ctx->vis_large_need, cap * ctx->V);
    ARVX_HIP(ctx->pool_vis_large.reserve(64 + (size_t)large_cap * sizeof(arvx::SplatRect)));
    uint32_t *zbuf = (uint32_t *)ctx->pool_vis_depth.p;
    unsigned *n_large = (unsigned *)ctx->pool_vis_large.p;
    arvx::SplatRect *large = (arvx::SplatRect *)((uint8_t *)ctx->pool_vis_large.p + 64);
    const int ncu = ctx->ncu > 0 ? ctx->ncu : 256;
    ARVX_TRY(launch(ctx, arvx::vis_clear_kernel, (unsigned)std::min<size_t>((nz + 255) / 256, 8 * ncu), 256,
                    zbuf, nz, n_large));
    arvx::SplatParams sp;
    sp.index = index;
    sp.cap = cap;
    sp.n_dev = n_dev;
    sp.X = ctx->X;
    sp.Y = ctx->Y;
    sp.s = ctx->s;
    sp.V = ctx->V;
    sp.W = ctx->W;
    sp.H = ctx->H;
    sp.M = ctx->M();
    sp.zbuf = zbuf;
    sp.large = large;
    sp.n_large = n_large;
    sp.large_cap = large_cap;
    // (the x grid strides over the list: its capacity can be several times its length; 4 workgroups
    // per compute unit and view, 1024 on 256 units)
    const dim3 sgrid((unsigned)std::min<long long>((cap + 255) / 256, 4 * ncu), (unsigned)ctx->V);
    ARVX_TRY(by_assoc(ctx, [&](auto left) {
        return launch(ctx, arvx::vis_splat_kernel<decltype(left)::value>, sgrid, 256, sp);
    }));
    ARVX_TRY(launch(ctx, arvx::vis_splat_large_kernel, (unsigned)(4 * ncu), 256, large, n_large, large_cap,
                    zbuf, ctx->W, ctx->H, ctx->word_dev(Ctx::kVisNeed)));
    *zbuf_out = zbuf;
    return ARVX_OK;
}

// The depth buffers and the visible vote, on the list vp describes (its length on the device): no
// synchronisation.
static int launch_visible_vote(Ctx *ctx, const arvx::VoteParams &vp, float tol) {
    const long long cap = vp.n;
    uint32_t *zbuf = nullptr;
    if (int rc = launch_depth_buffers(ctx, vp.index, cap, vp.n_dev, &zbuf)) return rc;
    arvx::VisVoteParams q;
    q.vote = vp;
    q.zbuf = zbuf;
    q.tol = tol;
    q.views = (int *)ctx->pool_vis_views.p;
    return by_assoc(ctx, [&](auto left) {
        return launch(ctx, arvx::vis_vote_kernel<decltype(left)::value>, blocks_for(cap), 256, q);
    });
}

int arvx_color_visible(arvx_ctx *ctx, int mode, float tolerance) {
    ARVX_CHECK_CTX(ctx);
    if (int rc = color_refusals(ctx, mode)) return rc;
    if (std::isnan(tolerance) || tolerance < 0.f)
        return fail(ARVX_ERR_INVALID, "tolerance %g: must be >= 0 (finite or +inf)", (double)tolerance);
    if (!whole_grid(ctx))  // (stripes: refused above)
        return fail(ARVX_ERR_STATE, "arvx_color_visible needs a whole-grid context (the depth buffers "
                                    "need every surface voxel)");
    return color_pass(ctx, mode, true, tolerance);
}

int arvx_photo_carve(arvx_ctx *ctx, float max_std, int min_views, float tolerance, int max_iterations,
                     int *iterations, int64_t *removed) {
    ARVX_CHECK_CTX(ctx);
    if (!ctx->cameras_ready) return fail(ARVX_ERR_STATE, "arvx_set_views has not been called");
    if (!ctx->images_ready) return fail(ARVX_ERR_STATE, "arvx_set_images has not been called");
    if (!ctx->has_campos) return fail(ARVX_ERR_STATE, "arvx_set_views was given no campos");
    if (ctx->stripe_world > 1)
        return fail(ARVX_ERR_STATE, "the colour pass needs contiguous slabs (neighbour planes)");
    if (std::isnan(max_std) || max_std < 0.f)
        return fail(ARVX_ERR_INVALID, "max_std %g: must be >= 0 (finite or +inf)", (double)max_std);
    if (std::isnan(tolerance) || tolerance < 0.f)
        return fail(ARVX_ERR_INVALID, "tolerance %g: must be >= 0 (finite or +inf)", (double)tolerance);
    if (min_views < 1) return fail(ARVX_ERR_INVALID, "min_views %d: must be >= 1", min_views);
    if (max_iterations < 1) return fail(ARVX_ERR_INVALID, "max_iterations %d: must be >= 1", max_iterations);
    if (!whole_grid(ctx))  // (stripes: refused above)
        return fail(ARVX_ERR_STATE, "arvx_photo_carve needs a whole-grid context (the depth buffers "
                                    "need every surface voxel)");
    if (int frc = fills_without_colours(ctx)) return frc;
    // every record exists before a bit is cleared: a lazy state ends here (rec_andnot_bitgrid_kernel
    // writes records only, and rec_or_bitgrid_lazy_kernel relies on every call that clears
    // closure_fills ending the lazy state)
    if (int mrc = need_rec(ctx)) return mrc;
    ctx->drop(Event::PhotoCarve);
    const int Zext = ctx->ze1 - ctx->ze0;
    const size_t nw_ext = bit_words(bit_grid(ctx, Zext));
    // the removal plane, and the removal counter in front of the per-entry words
    ARVX_HIP(ctx->pool_photo_plane.reserve(nw_ext * sizeof(unsigned long long)));
    ARVX_HIP(ctx->pool_photo_rm.reserve(64 + 64 * sizeof(unsigned long long)));
    ARVX_HIP(hipMemsetAsync(ctx->pool_photo_rm.p, 0, sizeof(unsigned long long), ctx->stream));
    unsigned long long *d_plane = (unsigned long long *)ctx->pool_photo_plane.p;
    const double max_var = (double)max_std * (double)max_std;
    long long removed_k = 0, removed_all = 0;
    int it = 0;
    auto reserve = [&](long long cap) -> int {
        // (the counter stays where it is: a reallocation starts it from zero again)
        const size_t need = 64 + ((size_t)cap / 64 + 2) * sizeof(unsigned long long);
        if (ctx->pool_photo_rm.cap < need) {
            ARVX_HIP(ctx->pool_photo_rm.reserve(need));
            ARVX_HIP(hipMemsetAsync(ctx->pool_photo_rm.p, 0, sizeof(unsigned long long), ctx->stream));
        }
        return ARVX_OK;
    };
    auto enqueue = [&](const arvx::VoteParams &vp) -> int {
        ctx->word(Ctx::kPhotoRemoved) = -1;  // (photo_plane_kernel leaves the iteration's removals there)
        const long long cap = vp.n;
        uint32_t *zbuf = nullptr;
        if (int rc = launch_depth_buffers(ctx, vp.index, cap, vp.n_dev, &zbuf)) return rc;
        arvx::PhotoParams q;
        q.vote = vp;
        q.zbuf = zbuf;
        q.tol = tolerance;
        q.max_var = max_var;
        q.min_views = min_views;
        q.removed = (unsigned long long *)ctx->pool_photo_rm.p;
        q.rm = (unsigned long long *)((uint8_t *)ctx->pool_photo_rm.p + 64);
        ARVX_TRY(by_assoc(ctx, [&](auto left) {
            return launch(ctx, arvx::photo_consist_kernel<decltype(left)::value>, blocks_for(cap), 256, q);
        }));
        ARVX_TRY(launch(ctx, arvx::photo_plane_kernel, blocks_for(nw_ext), 256,
                        (const arvx::SparseWord *)ctx->pool_col_rank.p, nw_ext, q.rm, cap, vp.n_dev, d_plane,
                        q.removed, ctx->word_dev(Ctx::kPhotoRemoved)));
        return records_apply(ctx, d_plane, Zext, false);
    };
    auto settle = [&]() -> int {
        if (ctx->word(Ctx::kVisNeed) >= 0) ctx->vis_large_need = ctx->word(Ctx::kVisNeed);
        removed_k = ctx->word(Ctx::kPhotoRemoved);
        if (removed_k < 0) return fail(ARVX_ERR_HIP, "the consistency pass left no count");
        return ARVX_OK;
    };
    // one synchronisation per iteration (two when the list outgrows its buffers: the truncated
    // attempt decides and removes nothing)
    while (it < max_iterations) {
        long long total = 0;
        if (int rc = surface_list(ctx, reserve, enqueue, settle, &total)) return rc;
        ++it;
        removed_all += removed_k;
        if (removed_k == 0) break;
        ctx->planes_seq = 0;  // (the colour pass's planes are those of the state before)
    }
    ctx->d_surf_index = nullptr;  // (the list is no colour list: color_ready stays clear)
    if (iterations) *iterations = it;
    if (removed) *removed = (int64_t)removed_all;
    return ARVX_OK;
}

// ---- connected components (components_kernels.h) -------------------------------------------------

static int components_refusals(const Ctx *ctx, int connectivity) {
    if (connectivity != 6 && connectivity != 26)
        return fail(ARVX_ERR_INVALID, "connectivity %d: must be 6 or 26", connectivity);
    if (!whole_grid(ctx))
        return fail(ARVX_ERR_STATE, "the components need a whole-grid context (a component may cross "
                                    "any plane)");
    return ARVX_OK;
}

// the rule of arvx_components_keep (null: label only)
struct ComponentsRule {
    long long min_voxels;
    int largest;
};

// Labels the current state: the per-voxel labels, the table (one list, by the list stages' protocol)
// and, with a rule, the removal: the plane of the components that go, taken off the records.  An
// attempt whose table outgrew its room counts no size and removes nothing.
static int components_run(Ctx *ctx, int connectivity, const ComponentsRule *rule, long long *count,
                          long long *kept, long long *removed) {
    ctx->comp_ready = false;  // (the buffers of an earlier labelling are written over)
    const arvx::BitGrid g = bit_grid(ctx);
    const size_t nwords = bit_words(g);
    ARVX_HIP(ctx->pool_comp_planes.reserve(3 * nwords * sizeof(unsigned long long)));
    ARVX_HIP(ctx->pool_comp_label.reserve(ctx->nvox * sizeof(int)));
    ARVX_HIP(ctx->pool_comp_rank.reserve(nwords * sizeof(arvx::SparseWord)));
    ARVX_HIP(ctx->pool_comp_ctl.reserve(64));
    unsigned long long *occ = (unsigned long long *)ctx->pool_comp_planes.p, *roots = occ + nwords,
                       *gone = roots + nwords;
    int *L = (int *)ctx->pool_comp_label.p;
    arvx::SparseWord *rank = (arvx::SparseWord *)ctx->pool_comp_rank.p;
    unsigned long long *ctl = (unsigned long long *)ctx->pool_comp_ctl.p;
    constexpr size_t kEntry = 2 * sizeof(int) + 4;  // label, size, keep byte (padded)
    ListRoom lists[1] = {{Ctx::kComponents, list_cap(ctx->pool_comp_table, kEntry, 1024), 0}};
    long long cap = 0;
    auto attempt = [&]() -> int {
        cap = lists[0].cap;
        ARVX_HIP(ctx->pool_comp_table.reserve((size_t)cap * kEntry));
        int *label = (int *)ctx->pool_comp_table.p, *size = label + cap;
        uint8_t *keep = (uint8_t *)(size + cap);
        if (int rc = launch_bit_pack(ctx, g, 0, 0, occ, nullptr)) return rc;
        const unsigned gv = blocks_for(ctx->nvox), gw = blocks_for(nwords);
        ARVX_TRY(launch(ctx, arvx::comp_init_kernel, gv, 256, occ, g, L));
        ARVX_TRY(launch(ctx, connectivity == 6 ? arvx::comp_link_kernel<6> : arvx::comp_link_kernel<26>, gv, 256,
                        occ, g, L));
        int *counts = nullptr;
        if (int rc = chunk_counts(ctx, nwords, &counts)) return rc;
        ARVX_TRY(launch(ctx, arvx::comp_roots_kernel, gw, 256, occ, g, L, roots, counts));
        ARVX_HIP(hipMemsetAsync(size, 0, (size_t)cap * sizeof(int), ctx->stream));
        ARVX_HIP(hipMemsetAsync(ctl, 0, 64, ctx->stream));
        const long long *d_total = nullptr;
        if (int rc = bit_compact(ctx, roots, nwords, g, cap, label, rank, Ctx::kComponents, &d_total)) return rc;
        ARVX_TRY(launch(ctx, arvx::comp_sizes_kernel, gw, 256, occ, g, L, rank, d_total, cap, size));
        if (!rule) return ARVX_OK;
        ctx->word(Ctx::kCompKept) = ctx->word(Ctx::kCompRemoved) = -1;
        const unsigned gk = blocks_for(cap);
        if (rule->largest) ARVX_TRY(launch(ctx, arvx::comp_best_kernel, gk, 256, label, size, d_total, cap, ctl));
        ARVX_TRY(launch(ctx, arvx::comp_decide_kernel, gk, 256, label, size, d_total, cap, rule->min_voxels,
                        rule->largest, ctl, keep));
        ARVX_TRY(launch(ctx, arvx::comp_remove_kernel, gw, 256, occ, g, L, rank, keep, d_total, cap, gone));
        ARVX_TRY(records_apply(ctx, gone, g.Z, false));
        return launch(ctx, arvx::comp_publish_kernel, 1, 1, ctl, ctx->word_dev(Ctx::kCompKept),
                      ctx->word_dev(Ctx::kCompRemoved));
    };
    // one synchronisation (two when the table outgrows its room: the truncated attempt removes nothing)
    if (int rc = run_lists(ctx, lists, attempt)) return rc;
    ctx->comp_count = lists[0].total;
    ctx->comp_cap = cap;
    ctx->comp_conn = connectivity;
    if (count) *count = lists[0].total;
    if (rule) {
        const long long k = ctx->word(Ctx::kCompKept), r = ctx->word(Ctx::kCompRemoved);
        if (k < 0 || r < 0) return fail(ARVX_ERR_HIP, "the components' kernels left no count");
        if (kept) *kept = k;
        if (removed) *removed = r;
    }
    return ARVX_OK;
}

int arvx_components(arvx_ctx *ctx, int connectivity, int64_t *count) {
    ARVX_CHECK_CTX(ctx);
    if (!count) return fail(ARVX_ERR_INVALID, "null count");
    if (int rc = components_refusals(ctx, connectivity)) return rc;
    long long n = 0;
    if (int rc = components_run(ctx, connectivity, nullptr, &n, nullptr, nullptr)) return rc;
    ctx->comp_ready = true;
    *count = (int64_t)n;
    return ARVX_OK;
}

int arvx_components_download(arvx_ctx *ctx, int32_t *label, int32_t *size) {
    ARVX_CHECK_CTX(ctx);
    if (!ctx->comp_ready) return fail(ARVX_ERR_STATE, "no labelling: arvx_components has not run on this state");
    const size_t bytes = (size_t)ctx->comp_count * sizeof(int32_t);
    const int *d_label = (const int *)ctx->pool_comp_table.p;
    if (label && bytes) ARVX_HIP(hipMemcpyAsync(label, d_label, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (size && bytes)
        ARVX_HIP(hipMemcpyAsync(size, d_label + ctx->comp_cap, bytes, hipMemcpyDeviceToHost, ctx->stream));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

int arvx_components_labels_download(arvx_ctx *ctx, int32_t *voxel_label) {
    ARVX_CHECK_CTX(ctx);
    if (!voxel_label) return fail(ARVX_ERR_INVALID, "null voxel_label");
    if (!ctx->comp_ready) return fail(ARVX_ERR_STATE, "no labelling: arvx_components has not run on this state");
    ARVX_HIP(hipMemcpyAsync(voxel_label, ctx->pool_comp_label.p, ctx->nvox * sizeof(int32_t),
                            hipMemcpyDeviceToHost, ctx->stream));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

int arvx_components_keep(arvx_ctx *ctx, int connectivity, int64_t min_voxels, unsigned flags, int64_t *kept,
                         int64_t *removed) {
    ARVX_CHECK_CTX(ctx);
    if (min_voxels < 1) return fail(ARVX_ERR_INVALID, "min_voxels %lld: must be >= 1", (long long)min_voxels);
    if (flags & ~ARVX_COMPONENTS_LARGEST) return fail(ARVX_ERR_INVALID, "unknown flag bits 0x%x", flags);
    if (int rc = components_refusals(ctx, connectivity)) return rc;
    if (int frc = fills_without_colours(ctx)) return frc;
    // every record exists before a bit is cleared (rec_andnot_bitgrid_kernel writes records only): a
    // lazy state ends here, as in arvx_photo_carve
    if (int mrc = need_rec(ctx)) return mrc;
    ctx->drop(Event::ComponentsKeep);
    const ComponentsRule rule{(long long)min_voxels, (flags & ARVX_COMPONENTS_LARGEST) ? 1 : 0};
    long long k = 0, r = 0;
    if (int rc = components_run(ctx, connectivity, &rule, nullptr, &k, &r)) return rc;
    if (kept) *kept = (int64_t)k;
    if (removed) *removed = (int64_t)r;
    return ARVX_OK;
}

// ---- signed distance field and ball morphology (distance_kernels.h) -----------------------------

static int distance_refusals(const Ctx *ctx) {
    if (!whole_grid(ctx))
        return fail(ARVX_ERR_STATE, "the distance field needs a whole-grid context (the nearest site may "
                                    "lie in any plane)");
    const long long x = ctx->X + 1ll, y = ctx->Y + 1ll, z = ctx->Z + 1ll;
    if (x * x + y * y + z * z > (long long)ARVX_DISTANCE_INF - 1)
        return fail(ARVX_ERR_STATE, "the squared distances of a %d x %d x %d grid do not fit 32 bits", ctx->X,
                    ctx->Y, ctx->Z);
    return ARVX_OK;
}

// the buffers of arvx_distance and arvx_morph; planes[k]: the k-th of the three bit planes
static int distance_reserve(Ctx *ctx, const arvx::BitGrid &g, unsigned long long *planes[3], unsigned *grid_y,
                            unsigned *grid_z) {
    const size_t nwords = bit_words(g);
    // a column pass: a lane per column and sign, a workgroup per 256 lanes, at most 4 per compute unit
    // (8 are 9 % faster at 512^3 and take twice the stack memory: DESIGN.md 4.12)
    // -- the others' lanes are taken in turn --, each with a stack region of (len + 2) * 256 entries
    const size_t most = (size_t)std::max(compute_units(ctx), 1) * 4;
    *grid_y = (unsigned)std::min((2 * (size_t)g.X * g.Z + 255) / 256, most);
    *grid_z = (unsigned)std::min((2 * (size_t)g.X * g.Y + 255) / 256, most);
    const size_t stack = std::max((size_t)*grid_y * (g.Y + 2), (size_t)*grid_z * (g.Z + 2)) * 256 * sizeof(int2);
    ARVX_HIP(ctx->pool_dist_field.reserve(ctx->nvox * sizeof(int)));
    ARVX_HIP(ctx->pool_dist_planes.reserve(3 * nwords * sizeof(unsigned long long)));
    ARVX_HIP(ctx->pool_dist_stack.reserve(stack));
    ARVX_HIP(ctx->pool_dist_ctl.reserve(64));
    for (int k = 0; k < 3; ++k) planes[k] = (unsigned long long *)ctx->pool_dist_planes.p + k * nwords;
    return ARVX_OK;
}

// the three passes: the field of bit plane `occ` into pool_dist_field
static int distance_run(Ctx *ctx, const arvx::BitGrid &g, const unsigned long long *occ, int border_empty,
                        unsigned grid_y, unsigned grid_z) {
    int *S = (int *)ctx->pool_dist_field.p;
    int2 *stack = (int2 *)ctx->pool_dist_stack.p;
    const size_t per_wg = 4 * (size_t)arvx::kDistWordsPerWave;
    ARVX_TRY(launch(ctx, arvx::dist_row_kernel, blocks_for(bit_words(g), per_wg), 256, occ, g, border_empty, S));
    // along y: column (x, z) starts at z * X * Y + x, its values X apart
    ARVX_TRY(launch(ctx, arvx::dist_column_kernel, grid_y, 256, S, (long long)g.X * g.Z, g.Y, g.X, g.X,
                    (long long)g.X * g.Y, border_empty, stack));
    // along z: column (x, y) starts at y * X + x, its values X * Y apart
    return launch(ctx, arvx::dist_column_kernel, grid_z, 256, S, (long long)g.X * g.Y, g.Z,
                  (long long)g.X * g.Y, g.X, g.X, border_empty, stack);
}

int arvx_distance(arvx_ctx *ctx, unsigned flags) {
    ARVX_CHECK_CTX(ctx);
    if (flags & ~ARVX_DISTANCE_BORDER_OCCUPIED) return fail(ARVX_ERR_INVALID, "unknown flag bits 0x%x", flags);
    if (int rc = distance_refusals(ctx)) return rc;
    ctx->dist_ready = false;  // (the field of an earlier call is written over)
    const arvx::BitGrid g = bit_grid(ctx);
    unsigned long long *planes[3];
    unsigned gy = 0, gz = 0;
    if (int rc = distance_reserve(ctx, g, planes, &gy, &gz)) return rc;
    if (int rc = launch_bit_pack(ctx, g, 0, 0, planes[0], nullptr)) return rc;
    if (int rc = distance_run(ctx, g, planes[0], !(flags & ARVX_DISTANCE_BORDER_OCCUPIED), gy, gz)) return rc;
    ctx->dist_ready = true;
    return ARVX_OK;
}

int arvx_distance_download(arvx_ctx *ctx, int32_t *signed_sq) {
    ARVX_CHECK_CTX(ctx);
    if (!signed_sq) return fail(ARVX_ERR_INVALID, "null signed_sq");
    if (!ctx->dist_ready) return fail(ARVX_ERR_STATE, "no distance field: arvx_distance has not run on this state");
    ARVX_HIP(hipMemcpyAsync(signed_sq, ctx->pool_dist_field.p, ctx->nvox * sizeof(int32_t), hipMemcpyDeviceToHost,
                            ctx->stream));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

int arvx_morph(arvx_ctx *ctx, int op, int64_t radius_sq, int64_t *removed, int64_t *added) {
    ARVX_CHECK_CTX(ctx);
    if (op < ARVX_MORPH_ERODE || op > ARVX_MORPH_CLOSE) return fail(ARVX_ERR_INVALID, "op %d: must be 0..3", op);
    if (radius_sq < 0 || radius_sq >= (int64_t)ARVX_DISTANCE_INF)
        return fail(ARVX_ERR_INVALID, "radius_sq %lld: must be in [0, %d)", (long long)radius_sq, ARVX_DISTANCE_INF);
    if (int rc = distance_refusals(ctx)) return rc;
    if (int frc = fills_without_colours(ctx)) return frc;
    const bool grows = op == ARVX_MORPH_DILATE || op == ARVX_MORPH_CLOSE;
    // every record exists before a bit is cleared or set (rec_andnot_bitgrid_kernel and
    // rec_or_bitgrid_kernel write records only): a lazy state ends here, as in arvx_components_keep
    if (int mrc = need_rec(ctx)) return mrc;
    const arvx::BitGrid g = bit_grid(ctx);
    unsigned long long *planes[3];
    unsigned gy = 0, gz = 0;
    if (int rc = distance_reserve(ctx, g, planes, &gy, &gz)) return rc;
    ctx->drop(grows ? Event::MorphGrow : Event::MorphShrink);
    unsigned long long *occ = planes[0], *mid = planes[1], *change = planes[2];
    unsigned long long *d_count = (unsigned long long *)ctx->pool_dist_ctl.p;
    const int *S = (const int *)ctx->pool_dist_field.p;
    const int R = (int)radius_sq;
    const size_t per_wg = 4 * (size_t)arvx::kDistWordsPerWave;  // (words of a dist_threshold_kernel workgroup)
    const unsigned gt = blocks_for(bit_words(g), per_wg);
    ARVX_HIP(hipMemsetAsync(d_count, 0, sizeof *d_count, ctx->stream));
    if (int rc = launch_bit_pack(ctx, g, 0, 0, occ, nullptr)) return rc;
    // the field of the state; for OPEN and CLOSE the first half's set as a plane, and the field of that
    if (int rc = distance_run(ctx, g, occ, 1, gy, gz)) return rc;
    if (op == ARVX_MORPH_OPEN || op == ARVX_MORPH_CLOSE) {
        ARVX_TRY(launch(ctx, arvx::dist_threshold_kernel, gt, 256, S, g, R, grows ? 1 : 0, 0, occ, mid,
                        d_count));
        // (CLOSE: the erosion of the dilated set leaves the grid's edge alone)
        if (int rc = distance_run(ctx, g, mid, grows ? 0 : 1, gy, gz)) return rc;
    }
    // what leaves (ERODE; OPEN: after the dilation of the eroded set) or joins (DILATE; CLOSE: after
    // the erosion of the dilated set) the model, against the occupancy the call started from
    const int second_grows = op == ARVX_MORPH_DILATE || op == ARVX_MORPH_OPEN;
    ARVX_TRY(launch(ctx, arvx::dist_threshold_kernel, gt, 256, S, g, R, second_grows, grows ? 2 : 1, occ,
                    change, d_count));
    ARVX_TRY(records_apply(ctx, change, g.Z, grows));
    ctx->word(Ctx::kMorphChanged) = -1;
    ARVX_HIP(hipMemcpyAsync(&ctx->word(Ctx::kMorphChanged), d_count, sizeof(long long), hipMemcpyDeviceToHost,
                            ctx->stream));
    ARVX_SYNC(ctx);
    const long long n = ctx->word(Ctx::kMorphChanged);
    if (n < 0) return fail(ARVX_ERR_HIP, "the morphology's kernels left no count");
    if (removed) *removed = grows ? 0 : (int64_t)n;
    if (added) *added = grows ? (int64_t)n : 0;
    return ARVX_OK;
}

int arvx_color_samples(arvx_ctx *ctx, int64_t n, const int64_t *index, int views,
                       arvx_color_sample *out) {
    ARVX_CHECK_CTX(ctx);
    static_assert(sizeof(arvx_color_sample) == 8, "r, g, b, valid, depth");
    if (!ctx->cameras_ready) return fail(ARVX_ERR_STATE, "arvx_set_views has not been called");
    if (views != ctx->V)
        return fail(ARVX_ERR_INVALID, "out holds %d samples per voxel, the context has %d views", views,
                    ctx->V);
    if (!ctx->images_ready) return fail(ARVX_ERR_STATE, "arvx_set_images has not been called");
    if (!ctx->has_campos) return fail(ARVX_ERR_STATE, "arvx_set_views was given no campos");
    if (n < 0 || (n && (!index || !out))) return fail(ARVX_ERR_INVALID, "null index / out or n < 0");
    if (n == 0) return ARVX_OK;
    const int64_t nown = (int64_t)ctx->X * ctx->Y * (ctx->z1 - ctx->z0);
    for (int64_t k = 0; k < n; ++k)
        if (index[k] < 0 || index[k] >= nown)
            return fail(ARVX_ERR_INVALID, "voxel index %lld outside [0,%lld)", (long long)index[k],
                        (long long)nown);
    const size_t total = (size_t)n * ctx->V;
    ARVX_HIP(ctx->pool_scratch.reserve((size_t)n * sizeof(long long) + total * sizeof(uint2) + 64));
    uint2 *d_out = (uint2 *)ctx->pool_scratch.p;
    long long *d_idx = (long long *)(d_out + total);
    ARVX_HIP(hipMemcpyAsync(d_idx, index, (size_t)n * sizeof(long long), hipMemcpyHostToDevice,
                            ctx->stream));
    arvx::VoteParams vp = vote_params(ctx, ctx->z0);  // (indices run over the owned planes)
    vp.n = n;
    const unsigned grid = blocks_for(total);
    ARVX_TRY(by_assoc(ctx, [&](auto left) {
        return launch(ctx, arvx::color_samples_kernel<decltype(left)::value>, grid, 256, vp, d_idx, d_out);
    }));
    ARVX_HIP(hipMemcpyAsync(out, d_out, total * sizeof(uint2), hipMemcpyDeviceToHost, ctx->stream));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

// The colour list's indices and has-flags on the host: fetched when somebody asks (a pipeline
// that goes on to the closure and the mesh on the device never does).
static int surf_host(Ctx *ctx) {
    if (ctx->surf_host_count == ctx->surf_count) return ARVX_OK;
    const size_t n = (size_t)ctx->surf_count;
    ctx->h_surf_index.resize(n);
    ctx->h_surf_has.resize(n);
    if (n) {
        ARVX_HIP(hipMemcpyAsync(ctx->h_surf_index.data(), ctx->d_surf_index, n * sizeof(int),
                                hipMemcpyDeviceToHost, ctx->stream));
        ARVX_HIP(hipMemcpyAsync(ctx->h_surf_has.data(), ctx->d_surf_has, n, hipMemcpyDeviceToHost,
                                ctx->stream));
        ARVX_SYNC(ctx);
    }
    ctx->surf_host_count = ctx->surf_count;
    return ARVX_OK;
}

int arvx_surface_count(arvx_ctx *ctx, int64_t *count) {
    if (!ctx || !count) return fail(ARVX_ERR_INVALID, "null argument");
    if (!ctx->color_ready) return fail(ARVX_ERR_STATE, "no colour result (call arvx_color)");
    ARVX_HIP(hipSetDevice(ctx->device));
    if (int rc = surf_host(ctx)) return rc;
    size_t lo, hi;
    long long base;
    owned_part(ctx, ctx->h_surf_index, lo, hi, base);
    int64_t n = 0;
    for (size_t e = lo; e < hi; ++e) n += ctx->h_surf_has[e];
    *count = n;
    return ARVX_OK;
}

static int surface_fetch(Ctx *ctx, std::vector<float> &rgb, std::vector<float> &depth) {
    rgb.resize((size_t)ctx->surf_count * 4);  // (r, g, b, has) per entry
    depth.resize((size_t)ctx->surf_count);
    if (ctx->surf_count) {
        ARVX_HIP(hipMemcpyAsync(rgb.data(), ctx->d_surf_rgba, rgb.size() * sizeof(float),
                                hipMemcpyDeviceToHost, ctx->stream));
        ARVX_HIP(hipMemcpyAsync(depth.data(), ctx->d_surf_depth, depth.size() * sizeof(float),
                                hipMemcpyDeviceToHost, ctx->stream));
        ARVX_SYNC(ctx);
    }
    return ARVX_OK;
}

int arvx_surface_download(arvx_ctx *ctx, int64_t *index, float *rgb) {
    ARVX_CHECK_CTX(ctx);
    if (!index || !rgb) return fail(ARVX_ERR_INVALID, "null argument");
    if (!ctx->color_ready) return fail(ARVX_ERR_STATE, "no colour result (call arvx_color)");
    std::vector<float> hrgb, hdepth;
    int rc = surface_fetch(ctx, hrgb, hdepth);
    if (rc) return rc;
    if (int rc2 = surf_host(ctx)) return rc2;
    size_t lo, hi;
    long long base;
    owned_part(ctx, ctx->h_surf_index, lo, hi, base);
    size_t k = 0;
    for (size_t e = lo; e < hi; ++e) {
        if (!ctx->h_surf_has[e]) continue;
        index[k] = ctx->h_surf_index[e] - base;
        rgb[3 * k] = hrgb[4 * e];
        rgb[3 * k + 1] = hrgb[4 * e + 1];
        rgb[3 * k + 2] = hrgb[4 * e + 2];
        ++k;
    }
    return ARVX_OK;
}

int arvx_surface_depth_download(arvx_ctx *ctx, float *depth) {
    ARVX_CHECK_CTX(ctx);
    if (!depth) return fail(ARVX_ERR_INVALID, "null argument");
    if (!ctx->color_ready) return fail(ARVX_ERR_STATE, "no colour result (call arvx_color)");
    std::vector<float> hrgb, hdepth;
    int rc = surface_fetch(ctx, hrgb, hdepth);
    if (rc) return rc;
    if (int rc2 = surf_host(ctx)) return rc2;
    size_t lo, hi;
    long long base;
    owned_part(ctx, ctx->h_surf_index, lo, hi, base);
    size_t k = 0;
    for (size_t e = lo; e < hi; ++e)
        if (ctx->h_surf_has[e]) depth[k++] = hdepth[e];
    return ARVX_OK;
}

static int visible_ready(const Ctx *ctx) {
    if (!ctx->color_ready || !ctx->color_visible)
        return fail(ARVX_ERR_STATE, "no visible colour result (call arvx_color_visible)");
    return ARVX_OK;
}

int arvx_surface_visible_download(arvx_ctx *ctx, int32_t *views) {
    ARVX_CHECK_CTX(ctx);
    if (int rc = visible_ready(ctx)) return rc;
    if (!views) return fail(ARVX_ERR_INVALID, "null argument");
    if (int rc = surf_host(ctx)) return rc;
    std::vector<int32_t> h((size_t)ctx->surf_count);
    if (ctx->surf_count) {
        ARVX_HIP(hipMemcpyAsync(h.data(), ctx->pool_vis_views.p, h.size() * sizeof(int32_t),
                                hipMemcpyDeviceToHost, ctx->stream));
        ARVX_SYNC(ctx);
    }
    size_t lo, hi;
    long long base;
    owned_part(ctx, ctx->h_surf_index, lo, hi, base);
    size_t k = 0;
    for (size_t e = lo; e < hi; ++e)
        if (ctx->h_surf_has[e]) views[k++] = h[e];
    return ARVX_OK;
}

int arvx_view_depth_download(arvx_ctx *ctx, int view, float *depth) {
    ARVX_CHECK_CTX(ctx);
    if (int rc = visible_ready(ctx)) return rc;
    if (view < 0 || view >= ctx->V) return fail(ARVX_ERR_INVALID, "view %d outside [0,%d)", view, ctx->V);
    if (!depth) return fail(ARVX_ERR_INVALID, "null argument");
    const size_t plane = (size_t)ctx->W * ctx->H;
    ARVX_HIP(hipMemcpyAsync(depth, (const uint32_t *)ctx->pool_vis_depth.p + plane * view,
                            plane * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

// Model::voxels of the owned voxels, built on the device in chunks and copied out.
int arvx_export_model(arvx_ctx *ctx, float *rgba, int apply_unseen) {
    ARVX_CHECK_CTX(ctx);
    if (int frc = fills_without_colours(ctx)) return frc;
    if (int mrc = need_rec(ctx)) return mrc;
    if (!rgba) return fail(ARVX_ERR_INVALID, "null rgba");
    arvx::CarveParams g = record_params(ctx);
    const int zown = ctx->z0 - ctx->ze0;
    if (int crc = closure_of_other_unseen(ctx, apply_unseen)) return crc;
    const size_t chunk = (size_t)1 << 24;  // voxels per chunk: 256 MiB of float4
    const size_t nchunk = std::min(chunk, ctx->nvox);
    float4 *d_out = nullptr;
    ARVX_HIP(hipMalloc(&d_out, nchunk * sizeof(float4)));
    auto export_chunk = [&](size_t i0) -> int {  // (returns early on a failure: the caller frees d_out)
        const size_t n = std::min(chunk, ctx->nvox - i0);
        const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 16384);
        ARVX_TRY(launch(ctx, arvx::export_fill_kernel, grid, 256, g, zown, i0, n, paint_plane(ctx), d_out,
                        apply_unseen));
        // entries of an ascending list (numbered over the context's planes) in owned voxels
        // [i0, i0 + n)
        const long long own_base = (long long)ctx->X * ctx->Y * zown;
        auto list_range = [&](const std::vector<int> &idx, long long &first, long long &last) {
            auto below = [](int a, long long b) { return (long long)a < b; };
            first = std::lower_bound(idx.begin(), idx.end(), own_base + (long long)i0, below) - idx.begin();
            last = std::lower_bound(idx.begin(), idx.end(), own_base + (long long)(i0 + n), below) -
                   idx.begin();
        };
        if (ctx->color_ready && ctx->surf_count > 0) {
            if (int rc = surf_host(ctx)) return rc;
            long long first, last;
            list_range(ctx->h_surf_index, first, last);
            if (last > first)
                ARVX_TRY(launch(ctx, arvx::export_scatter_kernel, blocks_for(last - first), 256,
                                ctx->d_surf_index, ctx->d_surf_rgba, first, last, g, zown, paint_plane(ctx),
                                i0, d_out, apply_unseen));
        }
        if (ctx->closure_ready && ctx->clo_count > 0) {
            if (int rc = clo_host(ctx)) return rc;
            long long first, last;
            list_range(ctx->h_clo_index, first, last);
            if (last > first)
                ARVX_TRY(launch(ctx, arvx::export_overlay_kernel, blocks_for(last - first), 256, ctx->d_clo_index,
                                (const float4 *)ctx->d_clo_rgba, first, last, own_base, i0, d_out));
        }
        ARVX_HIP(hipMemcpyAsync(rgba + 4 * i0, d_out, n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
        ARVX_HIP(hipStreamSynchronize(ctx->stream));
        return ARVX_OK;
    };
    int rc = ARVX_OK;
    for (size_t i0 = 0; i0 < ctx->nvox && rc == ARVX_OK; i0 += chunk) rc = export_chunk(i0);
    (void)hipFree(d_out);
    return rc;
}

int arvx_selftest_divide(arvx_ctx *ctx, int64_t n, const float *a0, const float *a1,
                         const float *b, float *out) {
    ARVX_CHECK_CTX(ctx);
    if (n < 1 || !a0 || !a1 || !b || !out) return fail(ARVX_ERR_INVALID, "bad argument");
    float *d = nullptr;
    ARVX_HIP(hipMalloc(&d, (size_t)n * 7 * sizeof(float)));
    auto run = [&]() -> int {  // (returns early on a failure: d is freed below)
        ARVX_HIP(hipMemcpyAsync(d, a0, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        ARVX_HIP(hipMemcpyAsync(d + n, a1, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        ARVX_HIP(hipMemcpyAsync(d + 2 * n, b, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        ARVX_TRY(launch(ctx, arvx::selftest_divide_kernel, blocks_for(n), 256, d, d + n, d + 2 * n, n, d + 3 * n));
        ARVX_HIP(hipMemcpyAsync(out, d + 3 * n, (size_t)n * 16, hipMemcpyDeviceToHost, ctx->stream));
        ARVX_HIP(hipStreamSynchronize(ctx->stream));
        return ARVX_OK;
    };
    const int rc = run();
    (void)hipFree(d);
    return rc;
}

int arvx_selftest_project(arvx_ctx *ctx, int64_t n, const float M[12], float voxel_size,
                          const int32_t *xyz, float *rows_uv) {
    ARVX_CHECK_CTX(ctx);
    if (!M) return fail(ARVX_ERR_INVALID, "null M");
    arvx::SelftestMatrix m;
    memcpy(m.m, M, sizeof m.m);
    const unsigned grid = blocks_for(n);
    return selftest_xyz(ctx, n, xyz, (size_t)n * 5, rows_uv, [&](int *d_xyz, float *d_out) {
        return by_assoc(ctx, [&](auto left) {
            return launch(ctx, arvx::selftest_project_kernel<decltype(left)::value>, grid, 256, m, voxel_size,
                          d_xyz, n, d_out, d_out + 3 * n);
        });
    });
}

int arvx_selftest_depth(arvx_ctx *ctx, int64_t n, const float campos[3], float voxel_size,
                        const int32_t *xyz, float *depth) {
    ARVX_CHECK_CTX(ctx);
    if (!campos) return fail(ARVX_ERR_INVALID, "null campos");
    arvx::SelftestMatrix m;
    memset(&m, 0, sizeof m);
    memcpy(m.m, campos, 3 * sizeof(float));
    return selftest_xyz(ctx, n, xyz, (size_t)n, depth, [&](int *d_xyz, float *d_out) {
        return launch(ctx, arvx::selftest_depth_kernel, blocks_for(n), 256, m, voxel_size, d_xyz, n, d_out);
    });
}

int arvx_selftest_view_tables(arvx_ctx *ctx, int view, uint32_t *bg_bits, uint16_t *table, int *ld) {
    ARVX_CHECK_CTX(ctx);
    if (!ctx->views_ready) return fail(ARVX_ERR_STATE, "arvx_set_views has not been called");
    if (view < 0 || view >= ctx->V) return fail(ARVX_ERR_INVALID, "view %d outside [0,%d)", view, ctx->V);
    if (!ld) return fail(ARVX_ERR_INVALID, "null ld");
    *ld = ctx->satW;
    // (every entry is asked for: those outside the views' windows are written now)
    if (table)
        if (int rc = complete_tables(ctx)) return rc;
    const size_t words = ((size_t)ctx->W * ctx->H + 31) / 32;
    if (bg_bits)
        ARVX_HIP(hipMemcpyAsync(bg_bits, ctx->bg() + (size_t)view * ctx->bgWords, words * sizeof(uint32_t),
                                hipMemcpyDeviceToHost, ctx->stream));
    if (table)
        ARVX_HIP(hipMemcpyAsync(table, ctx->sat() + (size_t)view * ctx->satStride,
                                (size_t)ctx->satStride * sizeof(uint16_t), hipMemcpyDeviceToHost,
                                ctx->stream));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

int arvx_selftest_view_table_raw(arvx_ctx *ctx, int view, uint16_t *table) {
    ARVX_CHECK_CTX(ctx);
    if (!ctx->views_ready) return fail(ARVX_ERR_STATE, "arvx_set_views has not been called");
    if (view < 0 || view >= ctx->V) return fail(ARVX_ERR_INVALID, "view %d outside [0,%d)", view, ctx->V);
    if (!table) return fail(ARVX_ERR_INVALID, "null table");
    ARVX_HIP(hipMemcpyAsync(table, ctx->sat() + (size_t)view * ctx->satStride,
                            (size_t)ctx->satStride * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

int arvx_selftest_round(arvx_ctx *ctx, int64_t *mismatches) {
    ARVX_CHECK_CTX(ctx);
    if (!mismatches) return fail(ARVX_ERR_INVALID, "null mismatches");
    *mismatches = -1;
    ARVX_HIP(ctx->pool_scratch.reserve(64));
    unsigned long long *d_bad = (unsigned long long *)ctx->pool_scratch.p;
    ARVX_HIP(hipMemsetAsync(d_bad, 0, sizeof *d_bad, ctx->stream));
    // every float in [+0, 2^24] and in (-0.5, -0]: all quotients that can be inside an image
    const unsigned ranges[2][2] = {{0x00000000u, 0x4B800000u}, {0x80000000u, 0xBEFFFFFFu}};
    for (const auto &r : ranges) {
        const unsigned long long n = (unsigned long long)r[1] - r[0] + 1;
        ARVX_TRY(launch(ctx, arvx::selftest_round_kernel, blocks_for(n), 256, r[0], r[1], d_bad));
    }
    unsigned long long bad = 0;
    ARVX_HIP(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
    ARVX_SYNC(ctx);
    *mismatches = (int64_t)bad;
    return ARVX_OK;
}

int arvx_ctx_set_rect_cache_limit(arvx_ctx *ctx, uint64_t bytes) {
    ARVX_CHECK_CTX(ctx);
    if (bytes > (uint64_t)1 << 46) return fail(ARVX_ERR_INVALID, "limit of %llu bytes", (unsigned long long)bytes);
    if (ctx->pool_rect.p) ARVX_SYNC(ctx);  // (a kernel of the stream may still be reading the table)
    ctx->pool_rect.release();
    ctx->pool_pix.release();  // (the pixels are relative to the block table's rectangles)
    ctx->rect_state = ctx->pix_state = Ctx::Rect::None;  // (decided again under the new limit)
    ctx->rect_limit = (size_t)bytes;
    return ARVX_OK;
}

int arvx_ctx_set_pixel_cache_limit(arvx_ctx *ctx, uint64_t bytes) {
    ARVX_CHECK_CTX(ctx);
    if (bytes > (uint64_t)1 << 46) return fail(ARVX_ERR_INVALID, "limit of %llu bytes", (unsigned long long)bytes);
    if (ctx->pool_pix.p) ARVX_SYNC(ctx);  // (a kernel of the stream may still be reading the table)
    ctx->pool_pix.release();
    ctx->pix_state = Ctx::Rect::None;  // (decided again under the new limit)
    ctx->pix_limit = (size_t)bytes;
    return ARVX_OK;
}

int arvx_pixel_cache_views(arvx_ctx *ctx, uint64_t *fits, int nwords) {
    ARVX_CHECK_CTX(ctx);
    if (!fits || nwords < 0) return fail(ARVX_ERR_INVALID, "null fits or %d words", nwords);
    const bool built = ctx->pix_state == Ctx::Rect::Built && ctx->pix_assoc == ctx->assoc;
    for (int w = 0; w < nwords; ++w) {
        const int left = ctx->V - 64 * w;  // views of this word
        const uint64_t all = left >= 64 ? ~0ull : left > 0 ? (1ull << left) - 1 : 0ull;
        fits[w] = built && left > 0 ? ~(uint64_t)ctx->pix_miss[w] & all : 0ull;
    }
    return ARVX_OK;
}

int arvx_selftest_pixel_cache(arvx_ctx *ctx, int64_t *mismatches) {
    ARVX_CHECK_CTX(ctx);
    if (!mismatches) return fail(ARVX_ERR_INVALID, "null mismatches");
    *mismatches = -1;
    // (a table built under the other grouping is as good as none: the next carve that could read
    // it builds it again)
    if (ctx->pix_state != Ctx::Rect::Built || ctx->rect_state != Ctx::Rect::Built || ctx->pix_assoc != ctx->assoc)
        return ARVX_OK;
    arvx::CarveParams p;
    carve_geometry(ctx, p);
    carve_views(ctx, p);
    rect_params(ctx, p);
    p.rcBlk = (const uint32_t *)ctx->pool_rect.p;
    ARVX_HIP(ctx->pool_scratch.reserve(64));
    unsigned long long *d_bad = (unsigned long long *)ctx->pool_scratch.p;
    ARVX_HIP(hipMemsetAsync(d_bad, 0, sizeof *d_bad, ctx->stream));
    const size_t n = pixel_lanes(ctx, p);
    ARVX_TRY(by_assoc(ctx, [&](auto left) {
        return launch(ctx, arvx::pixel_cache_kernel<decltype(left)::value, true>, pixel_grid(n), 256, p,
                      (uint4 *)ctx->pool_pix.p, n, (unsigned long long *)nullptr, d_bad);
    }));
    unsigned long long bad = 0;
    ARVX_HIP(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
    ARVX_SYNC(ctx);
    *mismatches = (int64_t)bad;
    return ARVX_OK;
}

int arvx_selftest_rect_cache(arvx_ctx *ctx, int64_t *mismatches) {
    ARVX_CHECK_CTX(ctx);
    if (!mismatches) return fail(ARVX_ERR_INVALID, "null mismatches");
    *mismatches = -1;
    if (ctx->rect_state != Ctx::Rect::Built) return ARVX_OK;
    arvx::CarveParams p;
    carve_geometry(ctx, p);
    carve_views(ctx, p);
    rect_params(ctx, p);
    ARVX_HIP(ctx->pool_scratch.reserve(64));
    unsigned long long *d_bad = (unsigned long long *)ctx->pool_scratch.p;
    ARVX_HIP(hipMemsetAsync(d_bad, 0, sizeof *d_bad, ctx->stream));
    const size_t n = rect_entries(ctx, p);
    ARVX_TRY(launch(ctx, arvx::rect_cache_block_kernel<true>,
                    (unsigned)std::min<size_t>((n + 255) / 256, 65536), 256, p, (uint32_t *)ctx->pool_rect.p,
                    n, nullptr, d_bad));
    unsigned long long bad = 0;
    ARVX_HIP(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
    ARVX_SYNC(ctx);
    *mismatches = (int64_t)bad;
    return ARVX_OK;
}

#ifdef ARVX_TIMELINE
// diagnostic builds only: per-workgroup {start, end (100 MHz ticks), xcc id, 0} of the last carve
extern "C" int arvx_debug_timeline(arvx_ctx *ctx, unsigned long long *out, int64_t *n) {
    ARVX_CHECK_CTX(ctx);
    *n = ctx->timeline_n;
    if (out && ctx->pool_timeline.p) {
        ARVX_SYNC(ctx);
        ARVX_HIP(hipMemcpy(out, ctx->pool_timeline.p, (size_t)ctx->timeline_n * ctx->timeline_rec,
                           hipMemcpyDeviceToHost));
    }
    return ARVX_OK;
}
#endif

// ---- closure -------------------------------------------------------------------------

int arvx_colors_upload(arvx_ctx *ctx, int64_t n, const int64_t *index, const float *rgb) {
    ARVX_CHECK_CTX(ctx);
    if (n < 0 || (n > 0 && (!index || !rgb))) return fail(ARVX_ERR_INVALID, "bad colour list");
    ctx->drop(Event::UploadColors);  // (before the indices are checked: a refused list drops the old one too)
    std::vector<int> idx((size_t)n);
    const long long own_base = (long long)ctx->X * ctx->Y * (ctx->z0 - ctx->ze0);
    for (int64_t k = 0; k < n; ++k) {
        if (index[k] < 0 || (size_t)index[k] >= ctx->nvox || (k && index[k] <= index[k - 1]))
            return fail(ARVX_ERR_INVALID, "colour indices must be ascending and inside the grid");
        idx[(size_t)k] = (int)(index[k] + own_base);  // numbered over the context's planes
    }
    ctx->surf_count = n;
    ctx->surf_host_count = n;
    ctx->h_surf_index = idx;
    ctx->h_surf_has.assign((size_t)n, 1);
    if (n > 0) {
        ARVX_HIP(ctx->pool_surf_index.reserve((size_t)n * sizeof(int)));
        ctx->d_surf_index = (int *)ctx->pool_surf_index.p;
        ARVX_HIP(ctx->pool_surf_rgb.reserve((size_t)n * sizeof(float4)));
        ctx->d_surf_rgba = (float4 *)ctx->pool_surf_rgb.p;
        ARVX_HIP(ctx->pool_surf_depth.reserve((size_t)n * sizeof(float)));
        ctx->d_surf_depth = (float *)ctx->pool_surf_depth.p;
        ARVX_HIP(ctx->pool_surf_has.reserve((size_t)n));
        ctx->d_surf_has = (uint8_t *)ctx->pool_surf_has.p;
        ARVX_HIP(hipMemcpyAsync(ctx->d_surf_index, idx.data(), (size_t)n * sizeof(int),
                                hipMemcpyHostToDevice, ctx->stream));
        // three floats per voxel from the host, (r, g, b, has = 1) on the device
        ARVX_HIP(ctx->pool_scratch.reserve((size_t)n * 3 * sizeof(float) + 64));
        ARVX_HIP(hipMemcpyAsync(ctx->pool_scratch.p, rgb, (size_t)n * 3 * sizeof(float),
                                hipMemcpyHostToDevice, ctx->stream));
        ARVX_TRY(launch(ctx, arvx::rgb_to_rgba_kernel, blocks_for(n), 256, (const float *)ctx->pool_scratch.p, n,
                        ctx->d_surf_rgba));
        ARVX_SYNC(ctx);  // (the scratch buffer is reused below)
        ARVX_HIP(hipMemsetAsync(ctx->d_surf_depth, 0, (size_t)n * sizeof(float), ctx->stream));
        ARVX_HIP(hipMemsetAsync(ctx->d_surf_has, 1, (size_t)n, ctx->stream));
        // the list's plane + ranks (what arvx_color leaves behind)
        const arvx::BitGrid gown = bit_grid(ctx, ctx->ze1 - ctx->ze0);  // the context's planes
        const size_t nw = bit_words(gown);
        const int nblk = (int)((nw + arvx::kBitBlock - 1) / arvx::kBitBlock);
        ARVX_HIP(ctx->pool_col_bits.reserve(nw * sizeof(unsigned long long)));
        ARVX_HIP(ctx->pool_col_rank.reserve(nw * sizeof(arvx::SparseWord)));
        ARVX_HIP(ctx->pool_scratch.reserve((size_t)(nblk + 1) * sizeof(long long) +
                                           (size_t)nblk * sizeof(int) + 64));
        unsigned long long *bits = (unsigned long long *)ctx->pool_col_bits.p;
        long long *d_off = (long long *)ctx->pool_scratch.p;
        int *d_cnt = (int *)(d_off + nblk + 1);
        ARVX_HIP(hipMemsetAsync(bits, 0, nw * sizeof(unsigned long long), ctx->stream));
        ARVX_TRY(launch(ctx, arvx::bits_from_index_kernel, blocks_for(n), 256, ctx->d_surf_index, n, gown, bits));
        long long total = 0;
        if (int rc = bit_compact_count(ctx, bits, nw, d_cnt, d_off, &total)) return rc;
        if (int rc = bit_compact_write(ctx, bits, nw, gown, d_off, nullptr,
                                       (arvx::SparseWord *)ctx->pool_col_rank.p))
            return rc;
        ARVX_SYNC(ctx);
    }
    ctx->color_ready = true;
    return ARVX_OK;
}

// the context's sparse lists as plane + rank (empty: nulls)
static arvx::SparseList colour_list(const Ctx *ctx) {
    if (!ctx->color_ready || ctx->surf_count <= 0) return arvx::SparseList{nullptr};
    return arvx::SparseList{(const arvx::SparseWord *)ctx->pool_col_rank.p};
}
static arvx::SparseList closure_list(const Ctx *ctx) {
    if (!ctx->closure_ready || ctx->clo_count <= 0) return arvx::SparseList{nullptr};
    return arvx::SparseList{(const arvx::SparseWord *)ctx->pool_clo_rank.p};
}

int arvx_closure(arvx_ctx *ctx, int kernel_size, int apply_unseen) {
    ARVX_CHECK_CTX(ctx);
    if (kernel_size < 1 || kernel_size % 2 != 1 || kernel_size > 9)
        return fail(ARVX_ERR_INVALID, "kernel size %d (odd, 1..9)", kernel_size);
    if (ctx->stripe_world > 1)
        return fail(ARVX_ERR_STATE, "arvx_closure needs contiguous slabs (neighbour planes)");
    if (ctx->closure_ready || ctx->closure_fills)
        return fail(ARVX_ERR_STATE, "closure already applied to this model state (carve, upload or reset first)");
    const int radius = (kernel_size - 1) / 2;
    // the planes that get filled here: all owned ones, plus the halo planes whose box lies
    // inside the planes that carry colours (stage_ranges)
    int c_lo, c_hi, f_lo, f_hi;
    stage_ranges(ctx, radius, c_lo, c_hi, f_lo, f_hi);
    if (f_lo > ctx->z0 || f_hi < ctx->z1)
        return fail(ARVX_ERR_STATE,
                    "a slab needs %d halo planes for a closure of size %d (it has %d): "
                    "arvx_ctx_create_slab_halo", radius + 1, kernel_size, ctx->halo);
    // (the planes are built from the lazy form; the tiles that exist only as a code are written out
    // further down, just before rec_or_bitgrid_kernel needs every record to exist -- written out
    // first, their non-temporal stores had emptied the caches of the records the planes are built from)
    if (int mrc = need_rec(ctx, true)) return mrc;
    // filled = dilate(occupied, box of radius r) and not occupied, on bit planes over the
    // context's planes
    const int Zext = ctx->ze1 - ctx->ze0;
    const arvx::BitGrid g = bit_grid(ctx, Zext);
    const size_t nwords = bit_words(g);
    const bool paints = apply_unseen || ctx->paint_valid;  // somebody is UNSEEN_COLOR
    ARVX_HIP(ctx->pool_scratch.reserve(3 * nwords * sizeof(unsigned long long) + 64));
    ARVX_HIP(ctx->pool_clo_bits.reserve(nwords * sizeof(unsigned long long)));
    ARVX_HIP(ctx->pool_clo_rank.reserve(nwords * sizeof(arvx::SparseWord)));
    unsigned long long *d_occ = (unsigned long long *)ctx->pool_scratch.p;
    unsigned long long *d_unseen = d_occ + nwords, *d_b = d_unseen + nwords;
    unsigned long long *d_fill = (unsigned long long *)ctx->pool_clo_bits.p;
    const unsigned gw = blocks_for(nwords);
    if (ctx->planes_seq == ctx->state_seq && !ctx->paint_valid && ctx->planes_words == nwords &&
        ctx->pool_state_planes.cap >= 2 * nwords * 8) {
        // the colour pass's planes are the state's (nothing but handleUnseen ran since): what the
        // closure calls occupied is their occupancy, with the never-seen voxels once those are occupied
        // (handleUnseen ran, or the caller says apply_unseen); the UNSEEN_COLOR plane is the never-seen one
        const unsigned long long *p_occ = (const unsigned long long *)ctx->pool_state_planes.p;
        const unsigned long long *p_nseen = p_occ + nwords;
        const bool merge = ctx->planes_unseen || apply_unseen;
        ARVX_TRY(launch(ctx, arvx::bit_dilate_xy_kernel, gw, 256, p_occ, merge ? p_nseen : nullptr, g, radius, d_b,
                        d_occ));
        if (!merge) d_occ = const_cast<unsigned long long *>(p_occ);
        d_unseen = const_cast<unsigned long long *>(p_nseen);  // (read only where `paints`)
    } else {
        if (int rc = launch_bit_pack(ctx, g, 1, apply_unseen ? 1 : 0, d_occ, paints ? d_unseen : nullptr))
            return rc;
        ARVX_TRY(launch(ctx, arvx::bit_dilate_xy_kernel, gw, 256, d_occ, nullptr, g, radius, d_b, nullptr));
    }
    // (halo planes outside [f_lo, f_hi): their boxes reach planes this context knows nothing
    // about -- not filled here, their owners do it: zeros)
    int *d_counts = nullptr;
    if (int rc = chunk_counts(ctx, nwords, &d_counts)) return rc;
    arvx::CarveParams rp = record_params(ctx);
    // Coarse tiles that exist only as their code: the few that receive a voxel are marked by the fill
    // plane's producer and written out by rec_or_bitgrid_lazy_kernel, the others stay codes (grids
    // whose rows and planes fill whole tiles; else every tile is written out first, as in round 4)
    // (never a second closure on the lazy state: closure_fills is refused above, and
    // rec_or_bitgrid_lazy_kernel depends on that)
    const bool lazy_or = ctx->form == Form::Lazy && ctx->Y % 8 == 0 && Zext % 8 == 0;
    arvx::CoarseMark mark{lazy_or ? (uint8_t *)ctx->pool_ccode.p : nullptr, rp.coarseX, rp.coarseY, rp.cyShift,
                          rp.czShift};
    ARVX_TRY(launch(ctx, arvx::bit_dilate_z_count_kernel, gw, 256, d_b, g, radius, d_occ, f_lo - ctx->ze0,
                    f_hi - ctx->ze0, d_fill, d_counts, mark));
    // The filled voxels are occupied from now on (their w is count / count = 1; the fill kernel reads
    // the occupancy from the bit planes, not from the records).  Launched HERE, right behind the
    // producer that marked the tiles: from this launch on the marks and the records agree, whatever
    // happens to the rest of the call.
    if (!lazy_or)
        if (int mrc = need_rec(ctx)) return mrc;  // every record exists from here on
    ctx->drop(Event::Closure);  // (the state changes here: tiles an earlier carve emptied may be occupied again)
    ctx->closure_fills = true;
    if (lazy_or)
        ARVX_TRY(launch(ctx, arvx::rec_or_bitgrid_lazy_kernel, gw, 256, rp, g.Z, d_fill,
                        (const uint8_t *)ctx->pool_ccode.p));
    else
        ARVX_TRY(launch(ctx, arvx::rec_or_bitgrid_kernel, gw, 256, rp, 0, g.Z, d_fill));
    // The list of the filled voxels: compacted and coloured in buffers sized before its length is known (run_lists).
    const double v = (double)nwords * 64.0;
    ListRoom lists[] = {{Ctx::kClosure, list_cap(ctx->pool_clo_index, sizeof(int), first_list_cap(v, v)), 0}};
    const long long &cap = lists[0].cap;
    auto attempt = [&]() -> int {
        ARVX_HIP(ctx->pool_clo_index.reserve((size_t)cap * sizeof(int)));
        ctx->d_clo_index = (int *)ctx->pool_clo_index.p;
        ARVX_HIP(ctx->pool_clo_rgba.reserve((size_t)cap * sizeof(float4)));
        ctx->d_clo_rgba = (void *)ctx->pool_clo_rgba.p;
        const long long *d_total = nullptr;
        if (int rc = bit_compact(ctx, d_fill, nwords, g, cap, ctx->d_clo_index,
                                 (arvx::SparseWord *)ctx->pool_clo_rank.p, Ctx::kClosure, &d_total))
            return rc;
        arvx::ClosureParams cp;
        cp.g = g;
        cp.occ = d_occ;
        cp.unseen = paints ? d_unseen : nullptr;
        cp.radius = radius;
        cp.col = colour_list(ctx);
        cp.col_rgba = ctx->d_surf_rgba;
        return launch(ctx, radius == 1 ? arvx::closure_fill_kernel<true> : arvx::closure_fill_kernel<false>,
                      blocks_for(cap), 256, cp, ctx->d_clo_index, cap, d_total, (float4 *)ctx->d_clo_rgba);
    };
    if (int rc = run_lists(ctx, lists, attempt)) return rc;
    const long long total = lists[0].total;
    ctx->clo_count = total;
    ctx->clo_host_count = -1;  // the list's host copy is fetched when somebody asks
    if (total == 0) ctx->closure_fills = false;  // (nothing was filled: the state is as before)
    if (total == 0) {
        ctx->d_clo_index = nullptr;
        ctx->d_clo_rgba = nullptr;
    }
    ctx->closure_ready = true;
    ctx->closure_unseen = apply_unseen ? 1 : 0;
    ctx->closure_radius = radius;
    return ARVX_OK;
}

// the closure list's indices on the host: fetched when somebody asks
static int clo_host(Ctx *ctx) {
    if (ctx->clo_host_count == ctx->clo_count) return ARVX_OK;
    const size_t n = (size_t)ctx->clo_count;
    ctx->h_clo_index.resize(n);
    if (n) {
        ARVX_HIP(hipMemcpyAsync(ctx->h_clo_index.data(), ctx->d_clo_index, n * sizeof(int),
                                hipMemcpyDeviceToHost, ctx->stream));
        ARVX_SYNC(ctx);
    }
    ctx->clo_host_count = ctx->clo_count;
    return ARVX_OK;
}

int arvx_closure_count(arvx_ctx *ctx, int64_t *count) {
    if (!ctx || !count) return fail(ARVX_ERR_INVALID, "null argument");
    if (!ctx->closure_ready) return fail(ARVX_ERR_STATE, "no closure result (call arvx_closure)");
    ARVX_HIP(hipSetDevice(ctx->device));
    if (owns_all_planes(ctx)) {  // (the list itself stays on the device until somebody asks for it)
        *count = (int64_t)ctx->clo_count;
        return ARVX_OK;
    }
    if (int rc = clo_host(ctx)) return rc;
    size_t lo, hi;
    long long base;
    owned_part(ctx, ctx->h_clo_index, lo, hi, base);
    *count = (int64_t)(hi - lo);  // (the filled voxels of the owned planes)
    return ARVX_OK;
}

int arvx_closure_download(arvx_ctx *ctx, int64_t *index, float *rgba) {
    ARVX_CHECK_CTX(ctx);
    if (!index || !rgba) return fail(ARVX_ERR_INVALID, "null argument");
    if (!ctx->closure_ready) return fail(ARVX_ERR_STATE, "no closure result (call arvx_closure)");
    if (int rc_h = clo_host(ctx)) return rc_h;
    size_t lo, hi;
    long long base;
    owned_part(ctx, ctx->h_clo_index, lo, hi, base);
    for (size_t k = lo; k < hi; ++k) index[k - lo] = ctx->h_clo_index[k] - base;
    if (hi > lo) {
        ARVX_HIP(hipMemcpyAsync(rgba, (const float4 *)ctx->d_clo_rgba + lo,
                                (hi - lo) * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
        ARVX_SYNC(ctx);
    }
    return ARVX_OK;
}

// ---- marching-cubes hand-off ----------------------------------------------------------

inline Ctx::Plane *Ctx::dec_bits() const { return (Plane *)(dec_rank() + dec_words); }

// The cell list, launched without a synchronisation: up to `cap` cells into the context's buffer,
// the list's true length in device word *d_total (and the count word kCells after the next sync).
static int mc_cells_launch(Ctx *ctx, long long cap, const long long **d_total) {
    if (int mrc = need_rec(ctx, true)) return mrc;  // (mc_zpack_rec_kernel reads lazy tiles)
    arvx::McParams mp;
    mp.X = ctx->X;
    mp.Y = ctx->Y;
    mp.Z = ctx->Z;
    mp.ze0 = ctx->ze0;
    mp.ze1 = ctx->ze1;
    // a cell belongs to the slab that owns its upper plane; the last slab also takes
    // the cells whose upper plane is outside the grid
    mp.cz0 = ctx->z0 - 1;
    mp.cz1 = (ctx->z1 == ctx->Z) ? ctx->Z : ctx->z1 - 1;
    mp.ZW = (mp.cz1 - mp.cz0 + 1 + 63) / 64;
    const size_t nzw = (size_t)mp.ZW * ctx->X * ctx->Y;  // z-packed occupancy words
    const long long ncol = (long long)(ctx->X + 1) * (ctx->Y + 1);
    ARVX_HIP(ctx->pool_scratch.reserve(nzw * sizeof(unsigned long long) +
                                       2 * (size_t)(ncol + 1) * sizeof(int) + 64));
    mp.zbits = (unsigned long long *)ctx->pool_scratch.p;
    int *d_off = (int *)(mp.zbits + nzw);  // ncol column offsets
    int *d_cnt = d_off + ncol + 1;
    const arvx::CarveParams g = record_params(ctx);
    ARVX_TRY(launch(ctx, arvx::mc_zpack_rec_kernel, (unsigned)((size_t)g.tilesX * g.tilesY * mp.ZW), 256, g, mp));
    const unsigned nblk = blocks_for(ncol);
    ARVX_TRY(launch(ctx, arvx::mc_count_kernel, nblk, 256, mp, d_cnt));
    // the columns' offsets in the list: one launch
    if (int rc = scan_counts(ctx, d_cnt, nullptr, ncol, nullptr, d_off, Ctx::kCells, d_total)) return rc;
    ARVX_HIP(ctx->pool_mc_cells.reserve((size_t)cap * sizeof(int4)));
    ctx->d_mc_cells = (void *)ctx->pool_mc_cells.p;
    return launch(ctx, arvx::mc_write_kernel, nblk, 256, mp, d_off, cap, (int4 *)ctx->d_mc_cells);
}
// room for the cell list before its length is known: what the last list needed, or a surface's share
static long long mc_cells_cap(const Ctx *ctx) {
    const double v = (double)ctx->nvox_ext;
    return list_cap(ctx->pool_mc_cells, sizeof(int4), first_list_cap(v, v + 1e6));
}

// The start of every mesh's attempt: the cell list at room `cap`, what the kernels read of the state and its
// colours, the cells' triangle offsets (in a pool of their own: the scratch buffer holds mc_cells_launch's arrays).
struct MeshCells {
    arvx::McMeshParams mp;
    const int4 *cells;
    long long cap;
    const long long *d_ncells;
    int *d_off;
};
static int mesh_cells_launch(Ctx *ctx, int apply_unseen, long long cap, MeshCells *m) {
    if (int rc = mc_cells_launch(ctx, cap, &m->d_ncells)) return rc;
    m->mp.g = record_params(ctx);
    m->mp.paint = paint_plane(ctx);
    m->mp.apply_unseen = apply_unseen ? 1 : 0;
    m->mp.col = colour_list(ctx);
    m->mp.col_rgba = ctx->d_surf_rgba;
    m->mp.clo = closure_list(ctx);
    m->mp.clo_rgba = (const float4 *)ctx->d_clo_rgba;
    m->cells = (const int4 *)ctx->d_mc_cells;
    m->cap = cap;
    ARVX_HIP(ctx->pool_mesh_off.reserve((size_t)(cap + 1) * sizeof(int)));
    m->d_off = ctx->pool_mesh_off.data();
    return scan_counts(ctx, nullptr, m->cells, cap, m->d_ncells, m->d_off, Ctx::kTris, nullptr);
}

// n entries of `entry` bytes to the host, where there are any and the caller wants them
static int download(Ctx *ctx, void *dst, const void *src, size_t n, size_t entry) {
    if (n > 0 && dst) ARVX_HIP(hipMemcpyAsync(dst, src, n * entry, hipMemcpyDeviceToHost, ctx->stream));
    return ARVX_OK;
}

int arvx_mc_cells(arvx_ctx *ctx, int64_t *count) {
    ARVX_CHECK_CTX(ctx);
    if (!count) return fail(ARVX_ERR_INVALID, "null argument");
    if (ctx->stripe_world > 1)
        return fail(ARVX_ERR_STATE, "the cell walk needs contiguous slabs (neighbour planes)");
    ctx->free_mc();
    ListRoom lists[] = {{Ctx::kCells, mc_cells_cap(ctx), 0}};
    if (int rc = run_lists(ctx, lists, [&] { return mc_cells_launch(ctx, lists[0].cap, nullptr); })) return rc;
    ctx->cells_built(lists[0].total);
    *count = lists[0].total;
    return ARVX_OK;
}

int arvx_mc_cells_download(arvx_ctx *ctx, int32_t *cells) {
    ARVX_CHECK_CTX(ctx);
    if (!cells) return fail(ARVX_ERR_INVALID, "null argument");
    if (!ctx->mc_ready) return fail(ARVX_ERR_STATE, "no cell list (call arvx_mc_cells)");
    if (ctx->mc_count) {
        ARVX_HIP(hipMemcpyAsync(cells, ctx->d_mc_cells, (size_t)ctx->mc_count * sizeof(int4),
                                hipMemcpyDeviceToHost, ctx->stream));
        ARVX_SYNC(ctx);
    }
    return ARVX_OK;
}

int arvx_mc_mesh(arvx_ctx *ctx, int apply_unseen, int64_t *triangles) {
    ARVX_CHECK_CTX(ctx);
    if (int frc = fills_without_colours(ctx)) return frc;
    if (!triangles) return fail(ARVX_ERR_INVALID, "null argument");
    if (ctx->stripe_world > 1)
        return fail(ARVX_ERR_STATE, "arvx_mc_mesh needs contiguous slabs (neighbour planes)");
    if (int crc = closure_of_other_unseen(ctx, apply_unseen)) return crc;
    {
        // a slab lists the cells whose upper plane it owns: their corners lie in planes
        // z0 - 1 .. z1 - 1, and plane z0 - 1 (a halo plane) must carry whatever the owned
        // planes carry -- colours, the closure's fills -- or the cells at the slab's lower
        // face would be coloured differently from the whole-grid result
        int c_lo, c_hi, f_lo, f_hi;
        stage_ranges(ctx, ctx->closure_radius, c_lo, c_hi, f_lo, f_hi);
        const int low = ctx->z0 > 0 ? ctx->z0 - 1 : 0;
        if (ctx->color_ready && ctx->surf_count > 0 && c_lo > low)
            return fail(ARVX_ERR_STATE, "a slab's mesh needs 2 halo planes once colours exist "
                                        "(it has %d): arvx_ctx_create_slab_halo", ctx->halo);
        if (ctx->closure_ready && f_lo > low)
            return fail(ARVX_ERR_STATE, "a slab's mesh needs %d halo planes after a closure of "
                                        "radius %d (it has %d): arvx_ctx_create_slab_halo",
                        ctx->closure_radius + 2, ctx->closure_radius, ctx->halo);
    }
    // cells -> triangles per cell -> triangles, all launched before the call's ONE synchronisation;
    // the kernels stop at the room they have, and a mesh that outgrew it is built once more (run_lists).
    ctx->free_mc();
    ctx->mesh_tris = 0;
    *triangles = 0;
    const long long cells = mc_cells_cap(ctx);
    ListRoom lists[] = {{Ctx::kCells, cells, 0},
                        {Ctx::kTris, list_cap(ctx->pool_mesh_verts, 3 * Ctx::kVertexBytes, 2 * cells), 0}};
    const long long &ccap = lists[0].cap, &tcap = lists[1].cap;
    auto attempt = [&]() -> int {
        ARVX_HIP(ctx->pool_mesh_verts.reserve((size_t)tcap * 3 * Ctx::kVertexBytes));
        ARVX_HIP(ctx->pool_mesh_rgb.reserve((size_t)tcap * Ctx::kFaceBytes));
        MeshCells mc;
        if (int rc = mesh_cells_launch(ctx, apply_unseen, ccap, &mc)) return rc;
        return launch(ctx, arvx::mc_mesh_kernel, blocks_for(ccap), 256, mc.mp, mc.cells, ccap, mc.d_ncells, tcap,
                      mc.d_off, ctx->pool_mesh_verts.data(), ctx->pool_mesh_rgb.data());
    };
    ARVX_TRY(run_lists(ctx, lists, attempt, [&] { return room_for_missing_cells(lists[0], lists[1]); }));
    ctx->cells_built(lists[0].total);
    *triangles = ctx->mesh_tris = lists[1].total;
    return ARVX_OK;
}

int arvx_mc_mesh_download(arvx_ctx *ctx, float *verts, uint32_t *face_rgb) {
    ARVX_CHECK_CTX(ctx);
    if (!verts || !face_rgb) return fail(ARVX_ERR_INVALID, "null argument");
    const size_t T = (size_t)ctx->mesh_tris;
    if (T > 0) {
        ARVX_TRY(download(ctx, verts, ctx->pool_mesh_verts.data(), T, 3 * Ctx::kVertexBytes));
        // r, g, b of the face records
        const size_t rgb = Ctx::kFaceBytes - Ctx::kFaceColour;
        ARVX_HIP(hipMemcpy2DAsync(face_rgb, rgb, (const uint8_t *)ctx->pool_mesh_rgb.data() + Ctx::kFaceColour,
                                  Ctx::kFaceBytes, rgb, T, hipMemcpyDeviceToHost, ctx->stream));
        ARVX_SYNC(ctx);
    }
    return ARVX_OK;
}

int arvx_mc_mesh_download_faces(arvx_ctx *ctx, float *verts, uint32_t *faces) {
    ARVX_CHECK_CTX(ctx);
    if (!verts || !faces) return fail(ARVX_ERR_INVALID, "null argument");
    const size_t T = (size_t)ctx->mesh_tris;
    ARVX_TRY(download(ctx, verts, ctx->pool_mesh_verts.data(), T, 3 * Ctx::kVertexBytes));
    ARVX_TRY(download(ctx, faces, ctx->pool_mesh_rgb.data(), T, Ctx::kFaceBytes));
    if (T > 0) ARVX_SYNC(ctx);
    return ARVX_OK;
}

// The frame of the two indexed meshes -- welded: a vertex per surface voxel; refined: a vertex per cut
// edge.  Occupancy plane -> vertex plane with its chunk counts -> vertex list; cells -> triangles; the
// vertices: all launched before the call's ONE synchronisation, as in arvx_mc_mesh; the three lists'
// lengths come back together, and a mesh that outgrew its buffers is built once more with room for all
// of it.  What differs between the two is in here, and in two callbacks: plane(d_counts) launches the
// vertex plane's kernel, build(mc, tcap, vcap, d_nverts) the triangle and the vertex kernels.
struct IndexedMesh {
    Ctx::Plane *occ, *vtx;  // the grid's occupancy plane; the vertex plane, of grid `vg` (both reserved)
    arvx::BitGrid vg;
    arvx::DevArray<arvx::SparseWord> &rank;  // the vertex plane's ranks
    arvx::DevArray<int> &index;              // the vertex list
    arvx::DevArray<float> &verts, &rgb;
    arvx::DevArray<unsigned> &faces;
    Ctx::Word word;           // the vertex list's count word
    int per_cell;             // its first room, in cells
    arvx::DevPool *more;      // a further array of `more_entry` bytes per vertex (null: none)
    size_t more_entry;
    long long nverts, ntris;  // out: the lists' lengths
};
extern "C++" template <class PlaneKernel, class Build>  // (the entry points' block has C linkage)
static int indexed_mesh(Ctx *ctx, int apply_unseen, IndexedMesh &m, PlaneKernel plane, Build build) {
    // the occupancy the cell walk reads (the records: closure fills included), then the vertex plane
    const size_t nvw = bit_words(m.vg);
    ARVX_HIP(m.rank.reserve(nvw * sizeof(arvx::SparseWord)));
    if (int rc = launch_bit_pack(ctx, bit_grid(ctx), 0, 0, m.occ, nullptr)) return rc;
    int *d_counts = nullptr;
    if (int rc = chunk_counts(ctx, nvw, &d_counts)) return rc;
    ARVX_TRY(plane(d_counts));
    // room: what the last mesh of this kind needed, or a surface's share of the voxels
    const long long cells = mc_cells_cap(ctx);
    ListRoom lists[] = {{Ctx::kCells, cells, 0},
                        {Ctx::kTris, list_cap(m.faces, Ctx::kFaceBytes, 2 * cells), 0},
                        {m.word, list_cap(m.index, sizeof(int), m.per_cell * cells), 0}};
    const long long &ccap = lists[0].cap, &tcap = lists[1].cap, &vcap = lists[2].cap;
    auto attempt = [&]() -> int {
        ARVX_HIP(m.index.reserve((size_t)vcap * sizeof(int)));
        ARVX_HIP(m.verts.reserve((size_t)vcap * Ctx::kVertexBytes));
        ARVX_HIP(m.rgb.reserve((size_t)vcap * Ctx::kVertexBytes));
        if (m.more) ARVX_HIP(m.more->reserve((size_t)vcap * m.more_entry));
        ARVX_HIP(m.faces.reserve((size_t)tcap * Ctx::kFaceBytes));
        const long long *d_nverts = nullptr;
        ARVX_TRY(bit_compact(ctx, m.vtx, nvw, m.vg, vcap, m.index.data(), m.rank.data(), m.word, &d_nverts));
        MeshCells mc;
        if (int rc = mesh_cells_launch(ctx, apply_unseen, ccap, &mc)) return rc;
        return build(mc, tcap, vcap, d_nverts);
    };
    ARVX_TRY(run_lists(ctx, lists, attempt, [&] { return room_for_missing_cells(lists[0], lists[1]); }));
    ctx->cells_built(lists[0].total);
    m.ntris = lists[1].total, m.nverts = lists[2].total;
    return ARVX_OK;
}

// The welded mesh (mc_weld_kernels.h).
int arvx_mc_mesh_welded(arvx_ctx *ctx, int apply_unseen, int64_t *vertices, int64_t *triangles) {
    ARVX_CHECK_CTX(ctx);
    if (int frc = fills_without_colours(ctx)) return frc;
    if (!vertices || !triangles) return fail(ARVX_ERR_INVALID, "null argument");
    if (!whole_grid(ctx))
        return fail(ARVX_ERR_STATE, "arvx_mc_mesh_welded needs a whole-grid context (vertex indices "
                                    "are ranks in the whole grid)");
    if (int crc = closure_of_other_unseen(ctx, apply_unseen)) return crc;
    ctx->free_mc();
    ctx->weld_ready = false;
    ctx->smooth_ready = ctx->smooth_csr_ready = false;  // (a new mesh: new CSRs)
    ctx->dec_ready = false;                              // (... and the old one's decimation goes)
    ctx->render_ready = false;                           // (... and the old one's render goes)
    for (int src : {ARVX_MESH_WELDED, ARVX_MESH_SMOOTHED, ARVX_MESH_DECIMATED})
        ctx->mesh_color_ended(src);                      // (... and the image colours of the three)
    for (int src : {ARVX_MESH_WELDED, ARVX_MESH_SMOOTHED, ARVX_MESH_DECIMATED})
        ctx->relax_ended(src);                           // (... and a relaxed mesh made of one of them)
    ctx->weld_verts = ctx->weld_tris = 0;
    *vertices = *triangles = 0;
    const arvx::BitGrid g = bit_grid(ctx);
    ctx->weld_words = bit_words(g);
    ARVX_HIP(ctx->pool_weld_planes.reserve(2 * ctx->weld_words * sizeof(Ctx::Plane)));
    IndexedMesh m{ctx->weld_occ(), ctx->weld_vtx(), g, ctx->pool_weld_rank, ctx->pool_weld_index,
                  ctx->pool_weld_verts, ctx->pool_weld_rgb, ctx->pool_weld_faces, Ctx::kVerts, 1, nullptr, 0, 0, 0};
    // the vertex plane: occupied voxels with an empty 6-neighbour
    auto plane = [&](int *d_counts) {
        return launch(ctx, arvx::bit_surface_count_kernel, blocks_for(ctx->weld_words), 256, m.occ, g, 0, ctx->Z,
                      m.vtx, d_counts);
    };
    auto build = [&](const MeshCells &mc, long long tcap, long long vcap, const long long *d_nverts) -> int {
        ARVX_TRY(launch(ctx, arvx::mc_weld_tri_kernel, blocks_for(mc.cap), 256, mc.mp,
                        arvx::SparseList{m.rank.data()}, mc.cells, mc.cap, mc.d_ncells, tcap, mc.d_off,
                        m.faces.data()));
        return launch(ctx, arvx::mc_weld_vertex_kernel, blocks_for(vcap), 256, mc.mp, m.index.data(), vcap,
                      d_nverts, m.verts.data(), m.rgb.data());
    };
    if (int rc = indexed_mesh(ctx, apply_unseen, m, plane, build)) return rc;
    *vertices = ctx->weld_verts = m.nverts;
    *triangles = ctx->weld_tris = m.ntris;
    ctx->weld_ready = true;
    return ARVX_OK;
}

int arvx_mc_mesh_welded_download(arvx_ctx *ctx, float *verts, uint32_t *faces, float *vertex_rgb) {
    ARVX_CHECK_CTX(ctx);
    if (!ctx->weld_ready) return fail(ARVX_ERR_STATE, "no welded mesh (call arvx_mc_mesh_welded)");
    const size_t V = (size_t)ctx->weld_verts, T = (size_t)ctx->weld_tris;
    if ((V > 0 && !verts) || (T > 0 && !faces)) return fail(ARVX_ERR_INVALID, "null argument");
    ARVX_TRY(download(ctx, verts, ctx->pool_weld_verts.data(), V, Ctx::kVertexBytes));
    ARVX_TRY(download(ctx, vertex_rgb, ctx->pool_weld_rgb.data(), V, Ctx::kVertexBytes));
    ARVX_TRY(download(ctx, faces, ctx->pool_weld_faces.data(), T, Ctx::kFaceBytes));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

// Taubin smoothing and vertex normals of the welded mesh (mc_smooth_kernels.h).  V and T are
// known on the host and every buffer is sized from bounds (neighbour entries <= min(26 V, 6 T),
// incidences <= 3 T), so no count has to come back: the call only launches, and
// arvx_mc_mesh_smooth_download has the synchronisation.  The CSRs are built at the first call on
// a welded mesh and kept for the next ones.
static int smooth_csr(Ctx *ctx) {
    const long long V = ctx->weld_verts, T = ctx->weld_tris;
    const long long ncap = std::min(26 * V, 6 * T), icap = 3 * T;
    const unsigned blocks_v = blocks_for(V + 1), blocks_t = blocks_for(T);
    ARVX_HIP(ctx->pool_smooth_csr.reserve(ctx->smooth_csr_bytes()));
    ARVX_HIP(ctx->pool_smooth_nbr.reserve((size_t)std::max(ncap, 1ll) * sizeof(unsigned)));
    ARVX_HIP(ctx->pool_smooth_inc.reserve((size_t)std::max(icap, 1ll) * sizeof(unsigned)));
    unsigned *masks = ctx->smooth_masks();
    int *icount = ctx->smooth_icount(), *ncount = ctx->smooth_ncount(), *noff = ctx->smooth_noff(),
        *ioff = ctx->smooth_ioff();
    unsigned *nbr = ctx->pool_smooth_nbr.data(), *inc = ctx->pool_smooth_inc.data(), *faces = ctx->pool_weld_faces.data();
    const int *index = ctx->pool_weld_index.data();
    // (the masks and the incidence counts: all that lies before the neighbour counts)
    ARVX_HIP(hipMemsetAsync(masks, 0, (size_t)(ncount - (int *)masks) * sizeof(int), ctx->stream));
    if (T > 0)
        ARVX_TRY(launch(ctx, arvx::mc_smooth_adjacency_kernel, blocks_t, 256, faces, T, V, index, ctx->X,
                        ctx->Y, masks, icount));
    ARVX_TRY(launch(ctx, arvx::mc_smooth_degree_kernel, blocks_v, 256, masks, V, ncount));
    // (a total no call reads)
    if (int rc = scan_counts(ctx, ncount, nullptr, V + 1, nullptr, noff, Ctx::kSmoothScan, nullptr)) return rc;
    if (int rc = scan_counts(ctx, icount, nullptr, V + 1, nullptr, ioff, Ctx::kSmoothScan, nullptr)) return rc;
    ARVX_TRY(launch(ctx, arvx::mc_smooth_neighbours_kernel, blocks_v, 256, masks, V, index, ctx->X, ctx->Y,
                    arvx::SparseList{ctx->pool_weld_rank.data()}, noff, ncap, nbr));
    if (T > 0)
        ARVX_TRY(launch(ctx, arvx::mc_smooth_incidence_kernel, blocks_t, 256, faces, T, V, icount, ioff, icap,
                        inc));
    ARVX_TRY(launch(ctx, arvx::mc_smooth_sort_kernel, blocks_v, 256, ioff, V, icap, inc));
    ctx->smooth_csr_ready = true;
    return ARVX_OK;
}

int arvx_mc_mesh_smooth(arvx_ctx *ctx, int iterations, float lambda, float mu) {
    ARVX_CHECK_CTX(ctx);
    if (iterations < 0 || !std::isfinite(lambda) || !std::isfinite(mu))
        return fail(ARVX_ERR_INVALID, "iterations must be >= 0 and the factors finite");
    if (!ctx->weld_ready) return fail(ARVX_ERR_STATE, "no welded mesh (call arvx_mc_mesh_welded)");
    ctx->smooth_ready = false;
    ctx->mesh_color_ended(ARVX_MESH_SMOOTHED);
    ctx->relax_ended(ARVX_MESH_SMOOTHED);
    const long long V = ctx->weld_verts, T = ctx->weld_tris;
    if (V == 0) {
        ctx->smooth_q = 0;
        ctx->smooth_ready = true;
        return ARVX_OK;
    }
    if (!ctx->smooth_csr_ready)
        if (int rc = smooth_csr(ctx)) return rc;
    const long long ncap = std::min(26 * V, 6 * T), icap = 3 * T;
    const unsigned blocks_v = blocks_for(V), blocks_t = blocks_for(T);
    // the steps: welded positions -> buffer 1 -> buffer 2 -> buffer 1 ...
    ARVX_HIP(ctx->pool_smooth_verts.reserve((size_t)2 * V * Ctx::kVertexBytes));
    int q = 0;
    for (int s = 0; s < 2 * iterations; ++s) {
        const int next = q == 1 ? 2 : 1;
        ARVX_TRY(launch(ctx, arvx::mc_smooth_step_kernel, blocks_v, 256, ctx->smooth_xyz(q), V, ctx->smooth_noff(),
                        ncap, ctx->pool_smooth_nbr.data(), (s & 1) ? mu : lambda, ctx->smooth_xyz(next)));
        q = next;
    }
    // the normals of the final positions
    ARVX_HIP(ctx->pool_smooth_cross.reserve((size_t)std::max(3 * T, 1ll) * sizeof(float)));
    ARVX_HIP(ctx->pool_smooth_normals.reserve((size_t)V * Ctx::kVertexBytes));
    if (T > 0)
        ARVX_TRY(launch(ctx, arvx::mc_smooth_cross_kernel, blocks_t, 256, ctx->pool_weld_faces.data(), T,
                        ctx->smooth_xyz(q), V, ctx->pool_smooth_cross.data()));
    ARVX_TRY(launch(ctx, arvx::mc_smooth_normal_kernel, blocks_v, 256, ctx->smooth_ioff(), V, icap,
                    ctx->pool_smooth_inc.data(), ctx->pool_smooth_cross.data(), T, ctx->pool_smooth_normals.data()));
    ctx->smooth_q = q;
    ctx->smooth_ready = true;
    return ARVX_OK;
}

int arvx_mc_mesh_smooth_download(arvx_ctx *ctx, float *verts, float *normals) {
    ARVX_CHECK_CTX(ctx);
    if (!ctx->smooth_ready) return fail(ARVX_ERR_STATE, "no smoothed mesh (call arvx_mc_mesh_smooth)");
    const size_t V = (size_t)ctx->weld_verts;
    ARVX_TRY(download(ctx, verts, ctx->smooth_xyz(ctx->smooth_q), V, Ctx::kVertexBytes));
    ARVX_TRY(download(ctx, normals, ctx->pool_smooth_normals.data(), V, Ctx::kVertexBytes));
    ARVX_HIP(hipStreamSynchronize(ctx->stream));
    if (int rc = check_fault(ctx)) {  // (a scan gave up: the CSRs are built again)
        ctx->smooth_ready = ctx->smooth_csr_ready = false;
        ctx->mesh_color_ended(ARVX_MESH_SMOOTHED);
        ctx->relax_ended(ARVX_MESH_SMOOTHED);
        return rc;
    }
    return ARVX_OK;
}

// Vertex clustering of the welded mesh (mc_decimate_kernels.h).  V and T are known on the host and
// Vd <= min(V, clusters), Td <= T: every buffer is sized from those bounds, nothing is retried, and
// the two counts come back in their own count words at the call's ONE synchronisation.
int arvx_mc_mesh_decimate(arvx_ctx *ctx, int cell, int source, int64_t *vertices, int64_t *triangles) {
    ARVX_CHECK_CTX(ctx);
    if (!vertices || !triangles) return fail(ARVX_ERR_INVALID, "null argument");
    if (cell < 1 || cell > 64) return fail(ARVX_ERR_INVALID, "cell %d (1..64 voxels)", cell);
    if (source != ARVX_DECIMATE_LATTICE && source != ARVX_DECIMATE_SMOOTHED)
        return fail(ARVX_ERR_INVALID, "source %d (ARVX_DECIMATE_LATTICE or ARVX_DECIMATE_SMOOTHED)", source);
    if (!ctx->weld_ready) return fail(ARVX_ERR_STATE, "no welded mesh (call arvx_mc_mesh_welded)");
    if (source == ARVX_DECIMATE_SMOOTHED && !ctx->smooth_ready)
        return fail(ARVX_ERR_STATE, "no smoothed mesh on this welded mesh (call arvx_mc_mesh_smooth)");
    ctx->dec_ready = false;
    ctx->mesh_color_ended(ARVX_MESH_DECIMATED);
    ctx->relax_ended(ARVX_MESH_DECIMATED);
    ctx->dec_verts = ctx->dec_tris = 0;
    const long long V = ctx->weld_verts, T = ctx->weld_tris;
    if (V == 0) {
        ctx->dec_ready = true;
        *vertices = *triangles = 0;
        return ARVX_OK;
    }
    arvx::DecGrid d;
    d.X = ctx->X, d.Y = ctx->Y, d.Z = ctx->Z, d.XW = (ctx->X + 63) / 64;
    d.cell = cell;
    d.CX = (ctx->X + cell - 1) / cell, d.CY = (ctx->Y + cell - 1) / cell, d.CZ = (ctx->Z + cell - 1) / cell;
    d.CXW = (d.CX + 63) / 64;
    const arvx::BitGrid cg{d.CX, d.CY, d.CZ, d.CXW};
    const size_t ncw = ctx->dec_words = bit_words(cg);
    const long long vcap = std::min<long long>(V, (long long)d.CX * d.CY * d.CZ);
    // the cluster plane, then its ranks (16-byte entries first)
    ARVX_HIP(ctx->pool_dec_planes.reserve(ncw * (sizeof(arvx::SparseWord) + sizeof(unsigned long long))));
    ARVX_HIP(ctx->pool_dec_index.reserve((size_t)vcap * sizeof(int)));
    ARVX_HIP(ctx->pool_dec_verts.reserve((size_t)vcap * 3 * sizeof(float)));
    ARVX_HIP(ctx->pool_dec_rgb.reserve((size_t)vcap * 3 * sizeof(float)));
    ARVX_HIP(ctx->pool_dec_members.reserve((size_t)vcap * sizeof(int)));
    ARVX_HIP(ctx->pool_dec_map.reserve((size_t)V * sizeof(int)));
    arvx::SparseWord *d_crank = ctx->dec_rank();
    Ctx::Plane *d_cbits = ctx->dec_bits();
    int *d_cidx = ctx->pool_dec_index.data(), *d_map = ctx->pool_dec_map.data();
    const arvx::SparseList vtx{ctx->pool_weld_rank.data()};
    const float *q = ctx->smooth_xyz(source == ARVX_DECIMATE_LATTICE ? 0 : ctx->smooth_q);
    // (the control block holds both totals: it must not move between the compaction and the scan)
    if (int rc = compact_control(ctx, (size_t)((T + arvx::kScanChunk - 1) / arvx::kScanChunk), nullptr)) return rc;
    int *d_counts = nullptr;
    if (int rc = chunk_counts(ctx, ncw, &d_counts)) return rc;
    ARVX_TRY(launch(ctx, arvx::mc_decimate_plane_kernel, blocks_for(ncw), 256, ctx->weld_vtx(), d, d_cbits, d_counts));
    const long long *d_nverts = nullptr;
    if (int rc = bit_compact(ctx, d_cbits, ncw, cg, vcap, d_cidx, d_crank, Ctx::kDecVerts, &d_nverts)) return rc;
    ARVX_TRY(launch(ctx, arvx::mc_decimate_vertex_kernel, blocks_for(vcap), 256, d_cidx, vcap, d_nverts, d, vtx,
                    V, q, ctx->pool_weld_rgb.data(), ctx->pool_dec_verts.data(), ctx->pool_dec_rgb.data(),
                    ctx->pool_dec_members.data()));
    ARVX_TRY(launch(ctx, arvx::mc_decimate_map_kernel, blocks_for(V), 256, ctx->pool_weld_index.data(), V, d,
                    arvx::SparseList{d_crank}, d_map));
    if (T > 0) {
        ARVX_HIP(ctx->pool_dec_faces.reserve((size_t)T * Ctx::kFaceBytes));
        ARVX_HIP(ctx->pool_dec_flags.reserve((size_t)T * 2 * sizeof(int)));
        ARVX_HIP(ctx->pool_dec_slots.reserve((size_t)vcap * arvx::kDecSlots * sizeof(unsigned)));
        const unsigned *faces = ctx->pool_weld_faces.data();
        unsigned *d_slots = ctx->pool_dec_slots.data();
        int *d_flags = ctx->dec_flags(), *d_off = ctx->dec_off();
        const unsigned blocks_t = blocks_for(T);
        ARVX_HIP(hipMemsetAsync(d_slots, 0xff, (size_t)vcap * arvx::kDecSlots * sizeof(unsigned), ctx->stream));
        ARVX_TRY(launch(ctx, arvx::mc_decimate_claim_kernel, blocks_t, 256, faces, T, V, d_map, d_cidx, vcap,
                        d_nverts, d, d_slots));
        ARVX_TRY(launch(ctx, arvx::mc_decimate_flag_kernel, blocks_t, 256, faces, T, V, d_map, d_cidx, vcap,
                        d_nverts, d, d_slots, d_flags));
        if (int rc = scan_counts(ctx, d_flags, nullptr, T, nullptr, d_off, Ctx::kDecTris, nullptr)) return rc;
        ARVX_TRY(launch(ctx, arvx::mc_decimate_write_kernel, blocks_t, 256, faces, T, V, d_map, d_flags,
                        d_off, T, ctx->pool_dec_faces.data()));
    }
    ARVX_SYNC(ctx);
    const long long nverts = host_total(ctx, Ctx::kDecVerts), ntris = T > 0 ? host_total(ctx, Ctx::kDecTris) : 0;
    if (nverts < 0 || ntris < 0) return fail(ARVX_ERR_HIP, "the decimation's kernels left no count");
    if (nverts > vcap || ntris > T) return fail(ARVX_ERR_HIP, "the decimated mesh outgrew the welded one");
    ctx->dec_verts = nverts;
    ctx->dec_tris = ntris;
    ctx->dec_ready = true;
    *vertices = nverts;
    *triangles = ntris;
    return ARVX_OK;
}

int arvx_mc_mesh_decimate_download(arvx_ctx *ctx, float *verts, uint32_t *faces, float *vertex_rgb,
                                   int32_t *members, int32_t *map) {
    ARVX_CHECK_CTX(ctx);
    if (!ctx->dec_ready) return fail(ARVX_ERR_STATE, "no decimated mesh (call arvx_mc_mesh_decimate)");
    const size_t Vd = (size_t)ctx->dec_verts, Td = (size_t)ctx->dec_tris, V = (size_t)ctx->weld_verts;
    ARVX_TRY(download(ctx, verts, ctx->pool_dec_verts.data(), Vd, Ctx::kVertexBytes));
    ARVX_TRY(download(ctx, faces, ctx->pool_dec_faces.data(), Td, Ctx::kFaceBytes));
    ARVX_TRY(download(ctx, vertex_rgb, ctx->pool_dec_rgb.data(), Vd, Ctx::kVertexBytes));
    ARVX_TRY(download(ctx, members, ctx->pool_dec_members.data(), Vd, sizeof(int)));
    ARVX_TRY(download(ctx, map, ctx->pool_dec_map.data(), V, sizeof(int)));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

// The refined mesh (mc_refine_kernels.h): the welded mesh's frame over the edge plane, the bisection in its
// vertex kernel.  Its buffers are its own: the welded mesh and what was made of it stay as they were.
int arvx_mc_mesh_refined(arvx_ctx *ctx, int apply_unseen, int bisections, int64_t *vertices,
                         int64_t *triangles) {
    ARVX_CHECK_CTX(ctx);
    if (!vertices || !triangles) return fail(ARVX_ERR_INVALID, "null argument");
    if (bisections < 0 || bisections > 10) return fail(ARVX_ERR_INVALID, "bisections %d (0..10)", bisections);
    if (!whole_grid(ctx))
        return fail(ARVX_ERR_STATE, "arvx_mc_mesh_refined needs a whole-grid context (vertex indices "
                                    "are ranks in the whole grid)");
    if (std::max({ctx->X, ctx->Y, ctx->Z}) > 4096)
        return fail(ARVX_ERR_STATE, "a grid side above 4096: the cut positions would not be exact in fp32");
    const arvx::BitGrid eg = arvx::refine_edge_grid(ctx->X, ctx->Y, ctx->Z);
    if ((long long)eg.X * eg.Y * eg.Z > (long long)INT32_MAX)
        return fail(ARVX_ERR_STATE, "3 (X+1)(Y+1)(Z+1) > INT32_MAX: the edge keys do not fit 32 bits");
    if (bisections > 0 && !ctx->views_ready)
        return fail(ARVX_ERR_STATE, "the bisection needs views with masks (arvx_set_views)");
    if (int frc = fills_without_colours(ctx)) return frc;
    if (int crc = closure_of_other_unseen(ctx, apply_unseen)) return crc;
    ctx->free_mc();
    ctx->ref_ready = false;
    ctx->mesh_color_ended(ARVX_MESH_REFINED);
    ctx->relax_ended(ARVX_MESH_REFINED);
    ctx->ref_verts = ctx->ref_tris = 0;
    *vertices = *triangles = 0;
    const arvx::BitGrid g = bit_grid(ctx);
    ctx->ref_words = bit_words(g);
    ARVX_HIP(ctx->pool_ref_planes.reserve((ctx->ref_words + bit_words(eg)) * sizeof(Ctx::Plane)));
    // (three cut edges per surface voxel, about)
    IndexedMesh m{ctx->ref_occ(), ctx->ref_edge_plane(), eg, ctx->pool_ref_rank, ctx->pool_ref_index,
                  ctx->pool_ref_verts, ctx->pool_ref_rgb, ctx->pool_ref_faces, Ctx::kRefVerts, 3,
                  &ctx->pool_ref_edges, (Ctx::kRefEdgeInts + 1) * sizeof(int), 0, 0};
    auto plane = [&](int *d_counts) {
        return launch(ctx, arvx::mc_refine_plane_kernel, blocks_for(bit_words(eg)), 256, m.occ, g, eg, m.vtx,
                      d_counts);
    };
    arvx::RefineViews vw{};
    if (ctx->views_ready)  // (without masks only bisections == 0 gets here: every cut is the midpoint)
        vw = arvx::RefineViews{ctx->M(), ctx->bg(), ctx->V, ctx->W, ctx->H, ctx->bgWords, ctx->s};
    auto build = [&](const MeshCells &mc, long long tcap, long long vcap, const long long *d_nverts) -> int {
        ARVX_TRY(launch(ctx, arvx::mc_refine_tri_kernel, blocks_for(mc.cap), 256, mc.mp,
                        arvx::SparseList{m.rank.data()}, eg, mc.cells, mc.cap, mc.d_ncells, tcap, mc.d_off,
                        m.faces.data()));
        ctx->ref_cap = vcap;  // (where the cut numerators start)
        return by_assoc(ctx, [&](auto left) {
            return launch(ctx, arvx::mc_refine_vertex_kernel<decltype(left)::value>, blocks_for(vcap), 256, mc.mp,
                          vw, m.occ, g, m.index.data(), vcap, d_nverts, bisections, m.verts.data(), m.rgb.data(),
                          ctx->ref_edges(), ctx->ref_cut());
        });
    };
    if (int rc = indexed_mesh(ctx, apply_unseen, m, plane, build)) return rc;
    *vertices = ctx->ref_verts = m.nverts;
    *triangles = ctx->ref_tris = m.ntris;
    ctx->ref_ready = true;
    return ARVX_OK;
}

int arvx_mc_mesh_refined_download(arvx_ctx *ctx, float *verts, uint32_t *faces, float *vertex_rgb,
                                  int32_t *edges, int32_t *cut) {
    ARVX_CHECK_CTX(ctx);
    if (!ctx->ref_ready) return fail(ARVX_ERR_STATE, "no refined mesh (call arvx_mc_mesh_refined)");
    const size_t Vr = (size_t)ctx->ref_verts, T = (size_t)ctx->ref_tris;
    ARVX_TRY(download(ctx, verts, ctx->pool_ref_verts.data(), Vr, Ctx::kVertexBytes));
    ARVX_TRY(download(ctx, faces, ctx->pool_ref_faces.data(), T, Ctx::kFaceBytes));
    ARVX_TRY(download(ctx, vertex_rgb, ctx->pool_ref_rgb.data(), Vr, Ctx::kVertexBytes));
    ARVX_TRY(download(ctx, edges, ctx->ref_edges(), Vr, Ctx::kRefEdgeInts * sizeof(int)));
    ARVX_TRY(download(ctx, cut, ctx->ref_cut(), Vr, sizeof(int)));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

// ---- render (render_kernels.h) ------------------------------------------------------------

// the images' places in pool_render_img: id | depth | bgr
static int *render_id(const Ctx *ctx) { return (int *)ctx->pool_render_img.p; }
static float *render_depth(const Ctx *ctx) {
    return (float *)ctx->pool_render_img.p + (size_t)ctx->render_W * ctx->render_H;
}
static uint8_t *render_bgr(const Ctx *ctx) {
    return (uint8_t *)ctx->pool_render_img.p + (size_t)ctx->render_W * ctx->render_H * 8;
}

// The refusals every render call shares, then the camera's own.
static int render_refusals(const Ctx *ctx, const float *M, int W, int H) {
    if (!ctx->weld_ready) return fail(ARVX_ERR_STATE, "no welded mesh (call arvx_mc_mesh_welded)");
    if (!M) return fail(ARVX_ERR_INVALID, "null M");
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(M[k])) return fail(ARVX_ERR_INVALID, "M[%d] is not finite", k);
    if (W < 1 || H < 1 || W > arvx::kMaxImageDim || H > arvx::kMaxImageDim)
        return fail(ARVX_ERR_INVALID, "image size %dx%d out of range", W, H);
    return ARVX_OK;
}

// What every render starts with: the pools, the keys cleared (with the list's header and the agreement
// counters: large_bytes of pool_render_large, 64 at least), the background in place.  A failure in
// here leaves no render.
static int render_begin(Ctx *ctx, int W, int H, const uint8_t *background, size_t bg_stride, size_t large_bytes) {
    ctx->render_ready = false;
    ctx->render_tris = false;
    const size_t npix = (size_t)W * H;
    ARVX_HIP(ctx->pool_render_keys.reserve(npix * sizeof(unsigned long long)));
    ARVX_HIP(ctx->pool_render_img.reserve(npix * 11));
    ARVX_HIP(ctx->pool_render_large.reserve(large_bytes));
    ctx->render_W = W;
    ctx->render_H = H;
    unsigned long long *keys = (unsigned long long *)ctx->pool_render_keys.p;
    arvx::RenderHeader *head = (arvx::RenderHeader *)ctx->pool_render_large.p;
    const int ncu = ctx->ncu > 0 ? ctx->ncu : 256;
    ARVX_TRY(launch(ctx, arvx::render_clear_kernel, (unsigned)std::min<size_t>((npix + 255) / 256, 8 * ncu),
                    256, keys, npix, head));
    // the background: the caller's rows, packed in the staging buffer, or zeros
    if (background) {
        if (!ctx->render_bg_done) ARVX_HIP(hipEventCreateWithFlags(&ctx->render_bg_done, hipEventDisableTiming));
        else ARVX_HIP(hipEventSynchronize(ctx->render_bg_done));  // (the last copy out of the buffer)
        if (ctx->render_bg_cap < npix * 3) {
            if (ctx->h_render_bg) (void)hipHostFree(ctx->h_render_bg);
            ctx->h_render_bg = nullptr;
            ctx->render_bg_cap = 0;
            ARVX_HIP(hipHostMalloc((void **)&ctx->h_render_bg, npix * 3, hipHostMallocDefault));
            ctx->render_bg_cap = npix * 3;
        }
        for (int r = 0; r < H; ++r)
            memcpy(ctx->h_render_bg + (size_t)r * W * 3, background + (size_t)r * bg_stride, (size_t)W * 3);
        ARVX_HIP(hipMemcpyAsync(render_bgr(ctx), ctx->h_render_bg, npix * 3, hipMemcpyHostToDevice, ctx->stream));
        ARVX_HIP(hipEventRecord(ctx->render_bg_done, ctx->stream));
    } else {
        ARVX_HIP(hipMemsetAsync(render_bgr(ctx), 0, npix * 3, ctx->stream));
    }
    return ARVX_OK;
}

// Clear, background, splat, large footprints, resolve: launches only.  The caller has refused what
// is to be refused; a failure in here leaves no render.
static int render_launch(Ctx *ctx, const float *M, int W, int H, const uint8_t *background, size_t bg_stride) {
    const size_t npix = (size_t)W * H;
    const long long n = ctx->weld_verts;
    // large footprints (large_list_cap): never more than there are vertices.
    // render_need is the count word as it stood at the last synchronisation of a render call
    // (arvx_render_download, arvx_render_agreement): renders launched back to back without one all
    // use the same capacity, whatever the device has finished by then.
    // (arvx_selftest_render_mesh_list bounds this list too: a small model cannot fill its own)
    const unsigned large_cap =
        ctx->render_mesh_list_cap >= 0
            ? (unsigned)std::min<long long>({ctx->render_mesh_list_cap, n, (long long)UINT32_MAX})
            : large_list_cap(n, ctx->render_need, n);
    ARVX_TRY(render_begin(ctx, W, H, background, bg_stride, 64 + (size_t)large_cap * sizeof(arvx::SplatRect)));
    unsigned long long *keys = (unsigned long long *)ctx->pool_render_keys.p;
    arvx::RenderHeader *head = (arvx::RenderHeader *)ctx->pool_render_large.p;
    arvx::SplatRect *large = (arvx::SplatRect *)((uint8_t *)ctx->pool_render_large.p + 64);
    const int ncu = ctx->ncu > 0 ? ctx->ncu : 256;
    if (n > 0) {
        arvx::RenderSplatParams sp;
        sp.index = ctx->pool_weld_index.data();
        sp.n = n;
        sp.X = ctx->X;
        sp.Y = ctx->Y;
        sp.s = ctx->s;
        sp.W = W;
        sp.H = H;
        memcpy(sp.M.m, M, 12 * sizeof(float));
        sp.keys = keys;
        sp.large = large;
        sp.n_large = &head->n_large;
        sp.large_cap = large_cap;
        // (the grid strides over the list)
        const dim3 sgrid((unsigned)std::min<long long>((n + 255) / 256, 8 * ncu));
        ARVX_TRY(by_assoc(ctx, [&](auto left) {
            return launch(ctx, arvx::render_splat_kernel<decltype(left)::value>, sgrid, 256, sp);
        }));
        ARVX_TRY(launch(ctx, arvx::render_splat_large_kernel, (unsigned)(4 * ncu), 256, large, &head->n_large,
                        large_cap, keys, W, ctx->word_dev(Ctx::kRenderNeed)));
    }
    ARVX_TRY(launch(ctx, arvx::render_resolve_kernel, blocks_for(npix), 256, keys, npix,
                    ctx->pool_weld_rgb.data(), render_id(ctx), render_depth(ctx), render_bgr(ctx)));
    ctx->render_ready = true;
    return ARVX_OK;
}

int arvx_render(arvx_ctx *ctx, const float M[12], int W, int H, const uint8_t *background, size_t bg_stride) {
    ARVX_CHECK_CTX(ctx);
    if (int rc = render_refusals(ctx, M, W, H)) return rc;
    if (background && bg_stride < (size_t)W * 3) return fail(ARVX_ERR_INVALID, "bg_stride %zu < 3 * W", bg_stride);
    return render_launch(ctx, M, W, H, background, bg_stride);
}

// arvx_render_view's refusals (arvx_render_agreement adds its own after them)
static int render_view_refusals(const Ctx *ctx, int view) {
    if (!ctx->weld_ready) return fail(ARVX_ERR_STATE, "no welded mesh (call arvx_mc_mesh_welded)");
    if (!ctx->cameras_ready) return fail(ARVX_ERR_STATE, "arvx_set_views has not been called");
    if (view < 0 || view >= ctx->V) return fail(ARVX_ERR_INVALID, "view %d outside [0,%d)", view, ctx->V);
    return render_refusals(ctx, ctx->h_M.data() + 12 * (size_t)view, ctx->W, ctx->H);
}

int arvx_render_view(arvx_ctx *ctx, int view) {
    ARVX_CHECK_CTX(ctx);
    if (int rc = render_view_refusals(ctx, view)) return rc;
    return render_launch(ctx, ctx->h_M.data() + 12 * (size_t)view, ctx->W, ctx->H, nullptr, 0);
}

int arvx_render_download(arvx_ctx *ctx, uint8_t *bgr, float *depth, int32_t *id) {
    ARVX_CHECK_CTX(ctx);
    if (!ctx->render_ready) return fail(ARVX_ERR_STATE, "no render (call arvx_render)");
    const size_t npix = (size_t)ctx->render_W * ctx->render_H;
    ARVX_TRY(download(ctx, bgr, render_bgr(ctx), npix, 3));
    ARVX_TRY(download(ctx, depth, render_depth(ctx), npix, sizeof(float)));
    ARVX_TRY(download(ctx, id, render_id(ctx), npix, sizeof(int32_t)));
    ARVX_SYNC(ctx);
    ctx->render_need = std::max(ctx->word(Ctx::kRenderNeed), 0ll);
    ctx->render_mesh_need = std::max(ctx->word(Ctx::kRenderMeshNeed), 0ll);
    return ARVX_OK;
}

int arvx_render_agreement(arvx_ctx *ctx, int view, int64_t counts[3]) {
    ARVX_CHECK_CTX(ctx);
    if (int rc = render_view_refusals(ctx, view)) return rc;
    if (!ctx->views_ready) return fail(ARVX_ERR_STATE, "arvx_set_views was given no masks");
    if (!counts) return fail(ARVX_ERR_INVALID, "null counts");
    if (int rc = render_launch(ctx, ctx->h_M.data() + 12 * (size_t)view, ctx->W, ctx->H, nullptr, 0)) return rc;
    const size_t npix = (size_t)ctx->W * ctx->H;
    arvx::RenderHeader *head = (arvx::RenderHeader *)ctx->pool_render_large.p;
    for (int k = 0; k < 3; ++k) ctx->word(Ctx::kRenderAgree + k) = -1;
    ARVX_TRY(launch(ctx, arvx::render_agreement_kernel, blocks_for(npix), 256, render_id(ctx), npix,
                    ctx->bg() + (size_t)view * ctx->bgWords, head->counts));
    ARVX_TRY(launch(ctx, arvx::render_counts_out_kernel, 1, 64, head->counts, ctx->word_dev(Ctx::kRenderAgree)));
    ARVX_SYNC(ctx);
    ctx->render_need = std::max(ctx->word(Ctx::kRenderNeed), 0ll);
    for (int k = 0; k < 3; ++k) {
        if (ctx->word(Ctx::kRenderAgree + k) < 0) return fail(ARVX_ERR_HIP, "the agreement left no count");
        counts[k] = ctx->word(Ctx::kRenderAgree + k);
    }
    return ARVX_OK;
}

// ---- triangle render (render_mesh_kernels.h) ------------------------------------------------

// A mesh as the rasteriser reads it: where its arrays lie and how long they are.
struct MeshSource {
    const float *verts, *rgb;
    const unsigned *faces;
    long long V, T;
    bool textured = false;  // drawn with arvx_mesh_texture's atlas in place of rgb
};

// The context's mesh `source`, or the refusal: an unknown source, or a mesh that does not exist
// (slab and striped contexts never build one).  With ARVX_MESH_IMAGE_COLORS (where the caller allows
// it) the colours are arvx_mesh_color's of that source, with ARVX_MESH_TEXTURED arvx_mesh_texture's
// atlas of that source.
static int mesh_source(const Ctx *ctx, int source, MeshSource &m, bool image_colours_allowed = true) {
    constexpr int both = ARVX_MESH_IMAGE_COLORS | ARVX_MESH_TEXTURED;
    if (image_colours_allowed && source >= 0 && (source & both) == both)
        return fail(ARVX_ERR_INVALID, "mesh source %#x: image colours and a texture exclude each other", source);
    const int base = image_colours_allowed && source >= 0 ? source & ~both : source;
    switch (base) {
    case ARVX_MESH_WELDED:
    case ARVX_MESH_SMOOTHED:
        if (!ctx->weld_ready) return fail(ARVX_ERR_STATE, "no welded mesh (call arvx_mc_mesh_welded)");
        if (base == ARVX_MESH_SMOOTHED && !ctx->smooth_ready)
            return fail(ARVX_ERR_STATE, "no smoothed mesh (call arvx_mc_mesh_smooth)");
        m = MeshSource{ctx->smooth_xyz(base == ARVX_MESH_WELDED ? 0 : ctx->smooth_q), ctx->pool_weld_rgb.data(),
                       ctx->pool_weld_faces.data(), ctx->weld_verts, ctx->weld_tris};
        break;
    case ARVX_MESH_DECIMATED:
        if (!ctx->dec_ready) return fail(ARVX_ERR_STATE, "no decimated mesh (call arvx_mc_mesh_decimate)");
        m = MeshSource{ctx->pool_dec_verts.data(), ctx->pool_dec_rgb.data(), ctx->pool_dec_faces.data(),
                       ctx->dec_verts, ctx->dec_tris};
        break;
    case ARVX_MESH_REFINED:
        if (!ctx->ref_ready) return fail(ARVX_ERR_STATE, "no refined mesh (call arvx_mc_mesh_refined)");
        m = MeshSource{ctx->pool_ref_verts.data(), ctx->pool_ref_rgb.data(), ctx->pool_ref_faces.data(),
                       ctx->ref_verts, ctx->ref_tris};
        break;
    case ARVX_MESH_RELAXED:  // the faces and colours of the product's base with the product's positions
        if (!ctx->relax_ready) return fail(ARVX_ERR_STATE, "no relaxed mesh (call arvx_mesh_relax)");
        if (int rc = mesh_source(ctx, ctx->relax_base, m, false)) return rc;  // (it ends with its base)
        if (ctx->relax_q != 0) m.verts = ctx->relax.xyz(ctx->relax_q);
        break;
    default:
        return fail(ARVX_ERR_INVALID, "unknown mesh source %d", source);
    }
    if (base != source && (source & ARVX_MESH_IMAGE_COLORS)) {
        if (!ctx->mesh_color_ready || ctx->mesh_color_source != base)
            return fail(ARVX_ERR_STATE, "no image colours of mesh source %d (call arvx_mesh_color)", base);
        m.rgb = ctx->pool_mcol_rgb.data();  // (as many as the source has vertices: the product ends with them)
    }
    if (base != source && (source & ARVX_MESH_TEXTURED)) {
        if (!ctx->mesh_texture_ready || ctx->mesh_texture_source != base || ctx->mesh_texture_faces != m.T)
            return fail(ARVX_ERR_STATE, "no texture of mesh source %d (call arvx_mesh_texture)", base);
        m.textured = true;  // (a cell half per face of the source: the product ends with them)
    }
    return ARVX_OK;
}

// ---- relaxed mesh (mesh_relax_kernels.h) -----------------------------------------------------

// The neighbour CSR and the incidence CSR of the mesh `faces` (V > 0 vertices, T faces) into r.  Every
// buffer is sized from V and T (6 T neighbour slots, 3 T incidences, a listed row per 49 of either),
// so no count comes back: launches only.
static int relax_csr(Ctx *ctx, Ctx::Relax &r, const unsigned *faces, long long V, long long T) {
    r.V = V, r.T = T;
    const long long ncap = r.ncap(), icap = r.icap();
    const int nrows_cap = r.nrows_cap(), irows_cap = r.irows_cap();
    ARVX_HIP(r.csr.reserve(r.csr_bytes()));
    ARVX_HIP(r.nbr.reserve((size_t)std::max(ncap, 1ll) * sizeof(unsigned)));
    ARVX_HIP(r.inc.reserve((size_t)std::max(icap, 1ll) * sizeof(unsigned)));
    ARVX_HIP(r.rows.reserve((size_t)(nrows_cap + irows_cap) * sizeof(int)));
    int *degree = r.degree(), *icount = r.icount(), *noff = r.noff(), *ioff = r.ioff();
    int *nrows = r.rows.data(), *irows = nrows + nrows_cap;
    const unsigned blocks_v = blocks_for(V), blocks_t = blocks_for(T);
    // (the row counters and both count arrays: all that lies before the offsets)
    ARVX_HIP(hipMemsetAsync(r.csr.data(), 0, (size_t)(noff - r.csr.data()) * sizeof(int), ctx->stream));
    if (T > 0) ARVX_TRY(launch(ctx, arvx::mesh_relax_count_kernel, blocks_t, 256, faces, T, V, degree, icount));
    // (a total no call reads)
    if (int rc = scan_counts(ctx, degree, nullptr, V + 1, nullptr, noff, Ctx::kRelaxScan, nullptr)) return rc;
    if (int rc = scan_counts(ctx, icount, nullptr, V + 1, nullptr, ioff, Ctx::kRelaxScan, nullptr)) return rc;
    if (T > 0)
        ARVX_TRY(launch(ctx, arvx::mesh_relax_fill_kernel, blocks_t, 256, faces, T, V, degree, icount, noff, ioff,
                        ncap, icap, r.nbr.data(), r.inc.data()));
    // the rows: a lane each, then the listed ones a workgroup each (the grid strides over the list)
    const int ncu = compute_units(ctx);
    ARVX_TRY(launch(ctx, arvx::mesh_relax_rows_kernel<true>, blocks_v, 256, noff, V, ncap, r.nbr.data(), degree,
                    nrows, r.n_rows(), nrows_cap));
    if (ncap > arvx::kRelaxLaneRow)
        ARVX_TRY(launch(ctx, arvx::mesh_relax_long_rows_kernel<true>, (unsigned)std::min(nrows_cap, 2 * ncu), 256,
                        noff, V, ncap, r.nbr.data(), degree, nrows, r.n_rows(), nrows_cap));
    ARVX_TRY(launch(ctx, arvx::mesh_relax_rows_kernel<false>, blocks_v, 256, ioff, V, icap, r.inc.data(), nullptr,
                    irows, r.n_rows() + 1, irows_cap));
    if (icap > arvx::kRelaxLaneRow)
        ARVX_TRY(launch(ctx, arvx::mesh_relax_long_rows_kernel<false>, (unsigned)std::min(irows_cap, 2 * ncu), 256,
                        ioff, V, icap, r.inc.data(), nullptr, irows, r.n_rows() + 1, irows_cap));
    return ARVX_OK;
}

// The steps from positions p0 and the normals of the final positions, on r's CSRs; *q: where the
// final positions are (0: p0 itself, else r.xyz(*q)).  Launches only.
static int relax_run(Ctx *ctx, Ctx::Relax &r, const float *p0, const unsigned *faces, int iterations, float lambda,
                     float mu, int *q_out) {
    const long long V = r.V, T = r.T;
    const unsigned blocks_v = blocks_for(V), blocks_t = blocks_for(T);
    if (iterations > 0) ARVX_HIP(r.verts.reserve((size_t)2 * V * Ctx::kVertexBytes));
    const float *in = p0;
    int q = 0;
    for (int s = 0; s < 2 * iterations; ++s) {
        const int next = q == 1 ? 2 : 1;
        ARVX_TRY(launch(ctx, arvx::mesh_relax_step_kernel, blocks_v, 256, in, V, r.noff(), r.degree(), r.ncap(),
                        r.nbr.data(), (s & 1) ? mu : lambda, r.xyz(next)));
        q = next;
        in = r.xyz(q);
    }
    ARVX_HIP(r.cross.reserve((size_t)std::max(3 * T, 1ll) * sizeof(float)));
    ARVX_HIP(r.normals.reserve((size_t)V * Ctx::kVertexBytes));
    if (T > 0) ARVX_TRY(launch(ctx, arvx::mc_smooth_cross_kernel, blocks_t, 256, faces, T, in, V, r.cross.data()));
    ARVX_TRY(launch(ctx, arvx::mc_smooth_normal_kernel, blocks_v, 256, r.ioff(), V, r.icap(), r.inc.data(),
                    r.cross.data(), T, r.normals.data()));
    *q_out = q;
    return ARVX_OK;
}

static int relax_arguments(int iterations, float lambda, float mu) {
    if (iterations < 0 || !std::isfinite(lambda) || !std::isfinite(mu))
        return fail(ARVX_ERR_INVALID, "iterations must be >= 0 and the factors finite");
    return ARVX_OK;
}

int arvx_mesh_relax(arvx_ctx *ctx, int source, int iterations, float lambda, float mu) {
    ARVX_CHECK_CTX(ctx);
    if (int rc = relax_arguments(iterations, lambda, mu)) return rc;
    if (source == ARVX_MESH_RELAXED) return fail(ARVX_ERR_INVALID, "the relaxed mesh cannot be its own source");
    MeshSource m;
    if (int rc = mesh_source(ctx, source, m, false)) return rc;
    if (6 * m.T > (long long)INT32_MAX || 3 * m.V > (long long)INT32_MAX)
        return fail(ARVX_ERR_STATE, "the mesh is too long: 6 T or 3 V > INT32_MAX (the CSR offsets are 32-bit)");
    ctx->relax_ready = false;
    ctx->mesh_color_ended(ARVX_MESH_RELAXED);
    // (the smoothed mesh has the welded mesh's faces: one adjacency for both)
    const int faces_of = source == ARVX_MESH_SMOOTHED ? ARVX_MESH_WELDED : source;
    int q = 0;
    if (m.V == 0) {
        ctx->relax_csr_ready = false;
        ctx->relax.V = ctx->relax.T = 0;
    } else {
        if (!ctx->relax_csr_ready || ctx->relax_csr_base != faces_of) {
            ctx->relax_csr_ready = false;
            if (int rc = relax_csr(ctx, ctx->relax, m.faces, m.V, m.T)) return rc;
            ctx->relax_csr_base = faces_of;
            ctx->relax_csr_ready = true;
        }
        if (int rc = relax_run(ctx, ctx->relax, m.verts, m.faces, iterations, lambda, mu, &q)) return rc;
    }
    ctx->relax_base = source;
    ctx->relax_q = q;
    ctx->relax_ready = true;
    return ARVX_OK;
}

int arvx_mesh_relax_info(arvx_ctx *ctx, int64_t out[3]) {
    ARVX_CHECK_CTX(ctx);
    if (!out) return fail(ARVX_ERR_INVALID, "null out");
    MeshSource m;
    if (int rc = mesh_source(ctx, ARVX_MESH_RELAXED, m, false)) return rc;
    out[0] = ctx->relax_base;
    out[1] = m.V;
    out[2] = m.T;
    return ARVX_OK;
}

int arvx_mesh_relax_download(arvx_ctx *ctx, float *verts, float *normals, int32_t *degree) {
    ARVX_CHECK_CTX(ctx);
    MeshSource m;
    if (int rc = mesh_source(ctx, ARVX_MESH_RELAXED, m, false)) return rc;
    const size_t V = (size_t)m.V;
    ARVX_TRY(download(ctx, verts, m.verts, V, Ctx::kVertexBytes));
    ARVX_TRY(download(ctx, normals, ctx->relax.normals.data(), V, Ctx::kVertexBytes));
    ARVX_TRY(download(ctx, degree, ctx->relax.degree(), V, sizeof(int)));
    ARVX_HIP(hipStreamSynchronize(ctx->stream));
    if (int rc = check_fault(ctx)) {  // (a scan gave up: the CSRs are built again)
        ctx->relax_ready = ctx->relax_csr_ready = false;
        ctx->mesh_color_ended(ARVX_MESH_RELAXED);
        return rc;
    }
    return ARVX_OK;
}

int arvx_mesh_relax_triangles(arvx_ctx *ctx, int64_t nv, const float *verts, int64_t nt, const uint32_t *faces,
                              int iterations, float lambda, float mu, float *out_verts, float *out_normals,
                              int32_t *out_degree) {
    ARVX_CHECK_CTX(ctx);
    if (!whole_grid(ctx)) return fail(ARVX_ERR_STATE, "arvx_mesh_relax_triangles needs a whole-grid context");
    if (int rc = relax_arguments(iterations, lambda, mu)) return rc;
    if (nv < 0 || nt < 0) return fail(ARVX_ERR_INVALID, "a negative count");
    if ((nv > 0 && !verts) || (nt > 0 && !faces)) return fail(ARVX_ERR_INVALID, "null mesh array");
    if (nt > (int64_t)INT32_MAX / 6 || nv > (int64_t)INT32_MAX / 3)
        return fail(ARVX_ERR_INVALID, "the mesh is too long: 6 nt or 3 nv > INT32_MAX (the CSR offsets are 32-bit)");
    for (int64_t t = 0; t < nt; ++t)
        for (int k = 0; k < 3; ++k)
            if ((int64_t)faces[6 * t + k] >= nv)
                return fail(ARVX_ERR_INVALID, "face %lld: index %u >= nv", (long long)t, faces[6 * t + k]);
    for (int64_t k = 0; k < 3 * nv; ++k)
        if (!(std::fabs(verts[k]) <= 1048576.f))  // (a NaN fails the comparison too)
            return fail(ARVX_ERR_INVALID, "vertex %lld: a coordinate that is not finite or above 2^20 in magnitude",
                        (long long)(k / 3));
    if (nv == 0) return ARVX_OK;  // (no face either: there is nothing to return)
    Ctx::Relax &r = ctx->relax_tri;
    ARVX_HIP(ctx->pool_rtri_verts.reserve((size_t)nv * Ctx::kVertexBytes));
    ARVX_HIP(ctx->pool_rtri_faces.reserve((size_t)std::max<int64_t>(nt, 1) * Ctx::kFaceBytes));
    ARVX_HIP(hipMemcpyAsync(ctx->pool_rtri_verts.p, verts, (size_t)nv * Ctx::kVertexBytes, hipMemcpyHostToDevice,
                            ctx->stream));
    if (nt > 0)
        ARVX_HIP(hipMemcpyAsync(ctx->pool_rtri_faces.p, faces, (size_t)nt * Ctx::kFaceBytes, hipMemcpyHostToDevice,
                                ctx->stream));
    int q = 0;
    if (int rc = relax_csr(ctx, r, ctx->pool_rtri_faces.data(), nv, nt)) return rc;
    if (int rc = relax_run(ctx, r, ctx->pool_rtri_verts.data(), ctx->pool_rtri_faces.data(), iterations, lambda, mu, &q))
        return rc;
    ARVX_TRY(download(ctx, out_verts, q == 0 ? ctx->pool_rtri_verts.data() : r.xyz(q), (size_t)nv, Ctx::kVertexBytes));
    ARVX_TRY(download(ctx, out_normals, r.normals.data(), (size_t)nv, Ctx::kVertexBytes));
    ARVX_TRY(download(ctx, out_degree, r.degree(), (size_t)nv, sizeof(int)));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

// the refusals of a camera, an image size, a background and a light
static int render_mesh_refusals(const float *M, int W, int H, const uint8_t *background, size_t bg_stride,
                                const float *light) {
    if (!M) return fail(ARVX_ERR_INVALID, "null M");
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(M[k])) return fail(ARVX_ERR_INVALID, "M[%d] is not finite", k);
    if (W < 1 || H < 1 || W > arvx::kMaxImageDim || H > arvx::kMaxImageDim)
        return fail(ARVX_ERR_INVALID, "image size %dx%d out of range", W, H);
    if (background && bg_stride < (size_t)W * 3) return fail(ARVX_ERR_INVALID, "bg_stride %zu < 3 * W", bg_stride);
    for (int k = 0; light && k < 3; ++k)
        if (!std::isfinite(light[k])) return fail(ARVX_ERR_INVALID, "light[%d] is not finite", k);
    return ARVX_OK;
}

// Clear, background, projection, raster, large boxes, resolve: launches only.  The caller has refused
// what is to be refused; a failure in here leaves no render.
static int render_mesh_launch(Ctx *ctx, const MeshSource &m, const float *M, int W, int H,
                              const uint8_t *background, size_t bg_stride, const float *light) {
    ARVX_TRY(render_begin(ctx, W, H, background, bg_stride, 64));
    const size_t npix = (size_t)W * H;
    // large pixel boxes (large_list_cap): never more than there are triangles.  render_mesh_need is
    // the count word as it stood at the last synchronisation of a render call.
    const unsigned large_cap =
        ctx->render_mesh_list_cap >= 0
            ? (unsigned)std::min<long long>({ctx->render_mesh_list_cap, m.T, (long long)UINT32_MAX})
            : large_list_cap(m.T, ctx->render_mesh_need, m.T);
    // (with a near plane the four clip counts lie behind the list)
    const bool clip = ctx->render_near > 0.f;
    const size_t clip_at = 64 + (size_t)large_cap * sizeof(arvx::SplatRect);
    constexpr size_t clip_bytes = arvx::kClipCounts * sizeof(unsigned long long);
    ARVX_HIP(ctx->pool_render_tris.reserve(clip_at + (clip ? clip_bytes : 0)));
    ctx->render_clip_at = 0;
    arvx::RenderMeshParams p{};
    p.verts = m.verts, p.rgb = m.rgb, p.faces = m.faces;
    p.V = m.V, p.T = m.T;
    p.s = ctx->s;
    p.W = W, p.H = H;
    memcpy(p.M.m, M, 12 * sizeof(float));
    p.keys = (unsigned long long *)ctx->pool_render_keys.p;
    p.head = (arvx::RenderMeshHeader *)ctx->pool_render_tris.p;
    p.large = (arvx::SplatRect *)((uint8_t *)ctx->pool_render_tris.p + 64);
    p.large_cap = large_cap;
    p.lit = light ? 1 : 0;
    for (int k = 0; k < 3; ++k) p.light[k] = light ? light[k] : 0.f;
    static_assert(sizeof(arvx::RenderMeshHeader) <= 64, "the header ends before the list");
    ARVX_HIP(hipMemsetAsync(p.head, 0, 64, ctx->stream));
    if (clip) {
        p.near = ctx->render_near;
        p.clip = (unsigned long long *)((uint8_t *)ctx->pool_render_tris.p + clip_at);
        ARVX_HIP(hipMemsetAsync(p.clip, 0, clip_bytes, ctx->stream));
    }
    if (m.T > 0 && m.V > 0) {
        ARVX_HIP(ctx->pool_render_proj.reserve((size_t)m.V * sizeof(arvx::MeshVertex)));
        p.proj = (arvx::MeshVertex *)ctx->pool_render_proj.p;
        const int ncu = ctx->ncu > 0 ? ctx->ncu : 256;
        ARVX_TRY(by_assoc(ctx, [&](auto left) {
            return launch(ctx, arvx::render_mesh_project_kernel<decltype(left)::value>, blocks_for(m.V), 256, p);
        }));
        // (the grid strides over the faces)
        const unsigned raster_blocks = (unsigned)std::min<long long>((m.T + 255) / 256, 8 * ncu);
        if (clip) {
            ARVX_TRY(by_assoc(ctx, [&](auto left) {
                constexpr bool L = decltype(left)::value;
                ARVX_TRY(launch(ctx, arvx::render_mesh_clip_raster_kernel<L>, raster_blocks, 256, p));
                return launch(ctx, arvx::render_mesh_clip_large_kernel<L>, (unsigned)(4 * ncu), 256, p,
                              ctx->word_dev(Ctx::kRenderMeshNeed));
            }));
        } else {
            ARVX_TRY(launch(ctx, arvx::render_mesh_raster_kernel, raster_blocks, 256, p));
            ARVX_TRY(launch(ctx, arvx::render_mesh_large_kernel, (unsigned)(4 * ncu), 256, p,
                            ctx->word_dev(Ctx::kRenderMeshNeed)));
        }
    } else {
        p.T = 0;  // (faces without vertices cannot be: every index is below V)
    }
    if (clip && p.T > 0) {
        // (the plane's resolve: the winner's piece re-derived)
        ARVX_TRY(by_assoc(ctx, [&](auto left) {
            constexpr bool L = decltype(left)::value;
            if (m.textured) {
                const arvx::MeshTextureColour tex{ctx->pool_mtex_atlas.data(),
                                                  arvx::texture_layout(m.T, ctx->mesh_texture_R, ctx->mesh_texture_AW)};
                return launch(ctx, arvx::render_mesh_clip_resolve_kernel<arvx::MeshTextureColour, L>, blocks_for(npix),
                              256, p, npix, render_id(ctx), render_depth(ctx), render_bgr(ctx), tex);
            }
            return launch(ctx, arvx::render_mesh_clip_resolve_kernel<arvx::MeshVertexColour, L>, blocks_for(npix), 256,
                          p, npix, render_id(ctx), render_depth(ctx), render_bgr(ctx), arvx::MeshVertexColour{});
        }));
    } else if (m.textured) {
        const arvx::MeshTextureColour tex{ctx->pool_mtex_atlas.data(),
                                          arvx::texture_layout(m.T, ctx->mesh_texture_R, ctx->mesh_texture_AW)};
        ARVX_TRY(launch(ctx, arvx::render_mesh_resolve_kernel<arvx::MeshTextureColour>, blocks_for(npix), 256, p,
                        npix, render_id(ctx), render_depth(ctx), render_bgr(ctx), tex));
    } else {
        ARVX_TRY(launch(ctx, arvx::render_mesh_resolve_kernel<arvx::MeshVertexColour>, blocks_for(npix), 256, p,
                        npix, render_id(ctx), render_depth(ctx), render_bgr(ctx), arvx::MeshVertexColour{}));
    }
    ctx->render_ready = true;
    ctx->render_tris = true;
    ctx->render_clip_at = clip ? clip_at : 0;
    return ARVX_OK;
}

int arvx_render_mesh(arvx_ctx *ctx, int source, const float M[12], int W, int H, const uint8_t *background,
                     size_t bg_stride, const float *light) {
    ARVX_CHECK_CTX(ctx);
    MeshSource m;
    if (int rc = mesh_source(ctx, source, m)) return rc;
    if (int rc = render_mesh_refusals(M, W, H, background, bg_stride, light)) return rc;
    return render_mesh_launch(ctx, m, M, W, H, background, bg_stride, light);
}

// arvx_render_mesh_view's refusals (arvx_render_mesh_agreement adds its own after them)
static int render_mesh_view_refusals(const Ctx *ctx, int source, int view, const float *light, MeshSource &m) {
    if (int rc = mesh_source(ctx, source, m)) return rc;
    if (!ctx->cameras_ready) return fail(ARVX_ERR_STATE, "arvx_set_views has not been called");
    if (view < 0 || view >= ctx->V) return fail(ARVX_ERR_INVALID, "view %d outside [0,%d)", view, ctx->V);
    return render_mesh_refusals(ctx->h_M.data() + 12 * (size_t)view, ctx->W, ctx->H, nullptr, 0, light);
}

int arvx_render_mesh_view(arvx_ctx *ctx, int source, int view, const float *light) {
    ARVX_CHECK_CTX(ctx);
    MeshSource m;
    if (int rc = render_mesh_view_refusals(ctx, source, view, light, m)) return rc;
    return render_mesh_launch(ctx, m, ctx->h_M.data() + 12 * (size_t)view, ctx->W, ctx->H, nullptr, 0, light);
}

int arvx_render_mesh_agreement(arvx_ctx *ctx, int source, int view, int64_t counts[3]) {
    ARVX_CHECK_CTX(ctx);
    MeshSource m;
    if (int rc = render_mesh_view_refusals(ctx, source, view, nullptr, m)) return rc;
    if (!ctx->views_ready) return fail(ARVX_ERR_STATE, "arvx_set_views was given no masks");
    if (!counts) return fail(ARVX_ERR_INVALID, "null counts");
    ARVX_TRY(render_mesh_launch(ctx, m, ctx->h_M.data() + 12 * (size_t)view, ctx->W, ctx->H, nullptr, 0, nullptr));
    const size_t npix = (size_t)ctx->W * ctx->H;
    arvx::RenderHeader *head = (arvx::RenderHeader *)ctx->pool_render_large.p;
    for (int k = 0; k < 3; ++k) ctx->word(Ctx::kRenderAgree + k) = -1;
    ARVX_TRY(launch(ctx, arvx::render_agreement_kernel, blocks_for(npix), 256, render_id(ctx), npix,
                    ctx->bg() + (size_t)view * ctx->bgWords, head->counts));
    ARVX_TRY(launch(ctx, arvx::render_counts_out_kernel, 1, 64, head->counts, ctx->word_dev(Ctx::kRenderAgree)));
    ARVX_SYNC(ctx);
    ctx->render_mesh_need = std::max(ctx->word(Ctx::kRenderMeshNeed), 0ll);
    for (int k = 0; k < 3; ++k) {
        if (ctx->word(Ctx::kRenderAgree + k) < 0) return fail(ARVX_ERR_HIP, "the agreement left no count");
        counts[k] = ctx->word(Ctx::kRenderAgree + k);
    }
    return ARVX_OK;
}

int arvx_render_triangles(arvx_ctx *ctx, int64_t nv, const float *verts, const float *vertex_rgb, int64_t nt,
                          const uint32_t *faces, const float M[12], int W, int H, const uint8_t *background,
                          size_t bg_stride, const float *light) {
    ARVX_CHECK_CTX(ctx);
    if (!whole_grid(ctx)) return fail(ARVX_ERR_STATE, "the render needs a whole-grid context");
    if (nv < 0 || nt < 0) return fail(ARVX_ERR_INVALID, "a negative count");
    if ((nv > 0 && (!verts || !vertex_rgb)) || (nt > 0 && !faces)) return fail(ARVX_ERR_INVALID, "null mesh array");
    if (nv > (int64_t)UINT32_MAX || nt > (int64_t)UINT32_MAX) return fail(ARVX_ERR_INVALID, "the mesh is too long");
    if (int rc = render_mesh_refusals(M, W, H, background, bg_stride, light)) return rc;
    for (int64_t t = 0; t < nt; ++t)
        for (int k = 0; k < 3; ++k)
            if ((int64_t)faces[6 * t + k] >= nv)
                return fail(ARVX_ERR_INVALID, "face %lld: index %u >= nv", (long long)t, faces[6 * t + k]);
    // (the pools may hold the mesh of a triangle render still in flight: the stream orders the copies
    // after it.  The caller's arrays are free when the call returns.)
    if (nv > 0) {
        ARVX_HIP(ctx->pool_tri_verts.reserve((size_t)nv * Ctx::kVertexBytes));
        ARVX_HIP(ctx->pool_tri_rgb.reserve((size_t)nv * Ctx::kVertexBytes));
        ARVX_HIP(hipMemcpyAsync(ctx->pool_tri_verts.p, verts, (size_t)nv * Ctx::kVertexBytes, hipMemcpyHostToDevice,
                                ctx->stream));
        ARVX_HIP(hipMemcpyAsync(ctx->pool_tri_rgb.p, vertex_rgb, (size_t)nv * Ctx::kVertexBytes,
                                hipMemcpyHostToDevice, ctx->stream));
    }
    if (nt > 0) {
        ARVX_HIP(ctx->pool_tri_faces.reserve((size_t)nt * Ctx::kFaceBytes));
        ARVX_HIP(hipMemcpyAsync(ctx->pool_tri_faces.p, faces, (size_t)nt * Ctx::kFaceBytes, hipMemcpyHostToDevice,
                                ctx->stream));
    }
    if (nv > 0 || nt > 0) ARVX_SYNC(ctx);
    const MeshSource m{ctx->pool_tri_verts.data(), ctx->pool_tri_rgb.data(), ctx->pool_tri_faces.data(), nv, nt, false};
    return render_mesh_launch(ctx, m, M, W, H, background, bg_stride, light);
}

int arvx_render_mesh_stats(arvx_ctx *ctx, int64_t out[4]) {
    ARVX_CHECK_CTX(ctx);
    if (!out) return fail(ARVX_ERR_INVALID, "null out");
    if (!ctx->render_ready || !ctx->render_tris)
        return fail(ARVX_ERR_STATE, "the current render is no triangle render (call arvx_render_mesh)");
    unsigned long long classes[arvx::kMeshClasses];
    const arvx::RenderMeshHeader *head = (const arvx::RenderMeshHeader *)ctx->pool_render_tris.p;
    ARVX_HIP(hipMemcpyAsync(classes, head->classes, sizeof classes, hipMemcpyDeviceToHost, ctx->stream));
    ARVX_SYNC(ctx);
    ctx->render_mesh_need = std::max(ctx->word(Ctx::kRenderMeshNeed), 0ll);
    for (int k = 0; k < arvx::kMeshClasses; ++k) out[k] = (int64_t)classes[k];
    return ARVX_OK;
}

int arvx_ctx_set_render_near(arvx_ctx *ctx, float near) {
    ARVX_CHECK_CTX(ctx);
    if (!(near == 0.f || (std::isfinite(near) && near >= FLT_MIN)))
        return fail(ARVX_ERR_INVALID, "near %g (0: no near plane; otherwise finite and >= FLT_MIN)", (double)near);
    ctx->render_near = near == 0.f ? 0.f : near;  // (-0 is 0)
    return ARVX_OK;
}

int arvx_ctx_render_near(const arvx_ctx *ctx, float *near) {
    ARVX_CHECK_CTX(ctx);
    if (!near) return fail(ARVX_ERR_INVALID, "null near");
    *near = ctx->render_near;
    return ARVX_OK;
}

int arvx_render_mesh_clip_stats(arvx_ctx *ctx, int64_t out[4]) {
    ARVX_CHECK_CTX(ctx);
    if (!out) return fail(ARVX_ERR_INVALID, "null out");
    if (!ctx->render_ready || !ctx->render_tris)
        return fail(ARVX_ERR_STATE, "the current render is no triangle render (call arvx_render_mesh)");
    unsigned long long counts[arvx::kClipCounts] = {0, 0, 0, 0};
    if (ctx->render_clip_at)
        ARVX_HIP(hipMemcpyAsync(counts, (const uint8_t *)ctx->pool_render_tris.p + ctx->render_clip_at, sizeof counts,
                                hipMemcpyDeviceToHost, ctx->stream));
    ARVX_SYNC(ctx);
    ctx->render_mesh_need = std::max(ctx->word(Ctx::kRenderMeshNeed), 0ll);
    for (int k = 0; k < arvx::kClipCounts; ++k) out[k] = (int64_t)counts[k];
    return ARVX_OK;
}

int arvx_selftest_render_mesh_list(arvx_ctx *ctx, int64_t cap) {
    ARVX_CHECK_CTX(ctx);
    if (cap < -1) return fail(ARVX_ERR_INVALID, "cap %lld (-1: the default room)", (long long)cap);
    ctx->render_mesh_list_cap = cap;
    return ARVX_OK;
}

int arvx_selftest_compute_units(arvx_ctx *ctx, int n) {
    ARVX_CHECK_CTX(ctx);
    (void)compute_units(ctx);  // (the device's own count, once)
    if (n < 0 || n > ctx->ncu_device)
        return fail(ARVX_ERR_INVALID, "compute units %d: must be 0 (the device's %d) or 1 .. %d", n,
                    ctx->ncu_device, ctx->ncu_device);
    ctx->ncu = n > 0 ? n : ctx->ncu_device;
    return ARVX_OK;
}

// ---- mesh colours from the images (mesh_color_kernels.h) -------------------------------------

// the projected vertices of one batch of views: never more than this, or one view's
static constexpr size_t kMeshColorProjBytes = (size_t)64 << 20;

// The depth pass of arvx_mesh_color and arvx_mesh_texture: the keys of mesh m in every view of the
// context, V x H x W into `keys` (the caller's), by batches of views -- project, raster, large boxes.
// Launches only.  Workspace: the batch's projected vertices and, behind its zeroed header, the list of
// large pixel boxes (pool_mcol_proj, pool_mcol_large); after the caller's synchronisation the word
// kMeshColorNeed holds what the fullest batch wanted to list.
static int mesh_depth_pass(Ctx *ctx, const MeshSource &m, unsigned long long *keys) {
    const int V = ctx->V, W = ctx->W, H = ctx->H;
    const size_t npix = (size_t)W * H;
    const bool faces = m.T > 0 && m.V > 0;
    // views per batch: what the bound on the projected vertices holds (one view at least)
    long long batch = std::max<long long>(1, (long long)(kMeshColorProjBytes / sizeof(arvx::MeshVertex)) / std::max(m.V, 1ll));
    if (ctx->mesh_color_batch > 0) batch = ctx->mesh_color_batch;
    batch = std::min<long long>({batch, V, 65535});
    // large pixel boxes of a batch (large_list_cap): never more than its (triangle, view) pairs
    const long long pairs = faces ? m.T * batch : 0;
    const unsigned large_cap =
        ctx->render_mesh_list_cap >= 0
            ? (unsigned)std::min<long long>({ctx->render_mesh_list_cap, pairs, (long long)UINT32_MAX})
            : large_list_cap(pairs, ctx->mesh_color_need, pairs);
    ARVX_HIP(ctx->pool_mcol_large.reserve(64 + (size_t)large_cap * sizeof(arvx::SplatRect)));
    static_assert(sizeof(arvx::MeshColorHeader) <= 64, "the header ends before the list");
    arvx::MeshColorHeader *head = (arvx::MeshColorHeader *)ctx->pool_mcol_large.p;
    ARVX_HIP(hipMemsetAsync(keys, 0xFF, (size_t)V * npix * sizeof(unsigned long long), ctx->stream));  // (kRenderEmpty)
    ARVX_HIP(hipMemsetAsync(head, 0, 64, ctx->stream));
    if (!faces) return ARVX_OK;
    const int ncu = compute_units(ctx);
    ARVX_HIP(ctx->pool_mcol_proj.reserve((size_t)batch * (size_t)m.V * sizeof(arvx::MeshVertex)));
    arvx::MeshColorParams p{};
    p.mesh.verts = m.verts, p.mesh.faces = m.faces;
    p.mesh.V = m.V, p.mesh.T = m.T;
    p.mesh.s = ctx->s;
    p.mesh.W = W, p.mesh.H = H;
    p.mesh.proj = (arvx::MeshVertex *)ctx->pool_mcol_proj.p;
    p.mesh.large = (arvx::SplatRect *)((uint8_t *)ctx->pool_mcol_large.p + 64);
    p.mesh.large_cap = large_cap;
    p.M = (const arvx::SelftestMatrix *)ctx->M();
    p.head = head;
    // (the grid strides over the faces: as many workgroups in all as the render's raster has)
    const unsigned tblocks = (unsigned)std::max<long long>(
        1, std::min<long long>((m.T + 255) / 256, (8ll * ncu + batch - 1) / batch));
    for (int v0 = 0; v0 < V; v0 += (int)batch) {
        p.view0 = v0;
        p.nviews = (int)std::min<long long>(batch, V - v0);
        p.mesh.keys = keys + (size_t)v0 * npix;
        if (v0 > 0) ARVX_HIP(hipMemsetAsync(&head->n_large, 0, sizeof head->n_large, ctx->stream));
        ARVX_TRY(by_assoc(ctx, [&](auto left) {
            return launch(ctx, arvx::mesh_color_project_kernel<decltype(left)::value>,
                          dim3(blocks_for(m.V), p.nviews), 256, p);
        }));
        ARVX_TRY(launch(ctx, arvx::mesh_color_raster_kernel, dim3(tblocks, p.nviews), 256, p));
        ARVX_TRY(launch(ctx, arvx::mesh_color_large_kernel, (unsigned)(4 * ncu), 256, p,
                        ctx->word_dev(Ctx::kMeshColorNeed)));
    }
    return ARVX_OK;
}

int arvx_mesh_color(arvx_ctx *ctx, int source, int mode, float tolerance, unsigned flags, int64_t *coloured) {
    ARVX_CHECK_CTX(ctx);
    if (!whole_grid(ctx)) return fail(ARVX_ERR_STATE, "arvx_mesh_color needs a whole-grid context");
    MeshSource m;
    if (int rc = mesh_source(ctx, source, m, false)) return rc;
    if (mode != ARVX_COLOR_CLOSEST && mode != ARVX_COLOR_AVERAGE) return fail(ARVX_ERR_INVALID, "colour mode %d", mode);
    if (flags & ~ARVX_MESH_COLOR_FOREGROUND) return fail(ARVX_ERR_INVALID, "unknown flag bits %#x", flags);
    if (std::isnan(tolerance) || tolerance < 0.f)
        return fail(ARVX_ERR_INVALID, "tolerance %g: must be >= 0 (finite or +inf)", (double)tolerance);
    if (!coloured) return fail(ARVX_ERR_INVALID, "null coloured");
    if (!ctx->cameras_ready) return fail(ARVX_ERR_STATE, "arvx_set_views has not been called");
    if (!ctx->images_ready) return fail(ARVX_ERR_STATE, "arvx_set_images has not been called");
    if ((flags & ARVX_MESH_COLOR_FOREGROUND) && !ctx->views_ready)
        return fail(ARVX_ERR_STATE, "ARVX_MESH_COLOR_FOREGROUND: arvx_set_views was given no masks");
    if (m.T > (long long)UINT32_MAX) return fail(ARVX_ERR_STATE, "the mesh is too long");
    ctx->mesh_color_ready = false;
    const int V = ctx->V, W = ctx->W, H = ctx->H;
    const size_t npix = (size_t)W * H;
    const bool faces = m.T > 0 && m.V > 0;
    ARVX_HIP(ctx->pool_mcol_keys.reserve((size_t)V * npix * sizeof(unsigned long long)));
    ARVX_HIP(ctx->pool_mcol_rgb.reserve((size_t)m.V * Ctx::kVertexBytes));
    ARVX_HIP(ctx->pool_mcol_views.reserve((size_t)m.V * sizeof(int)));
    unsigned long long *keys = (unsigned long long *)ctx->pool_mcol_keys.p;
    ARVX_TRY(mesh_depth_pass(ctx, m, keys));
    arvx::MeshColorHeader *head = (arvx::MeshColorHeader *)ctx->pool_mcol_large.p;
    unsigned long long n_coloured = 0;
    if (m.V > 0) {
        arvx::MeshVoteParams vp{};
        vp.verts = m.verts, vp.col = m.rgb;
        vp.Vn = m.V;
        vp.s = ctx->s;
        vp.V = V, vp.W = W, vp.H = H;
        vp.M = (const arvx::SelftestMatrix *)ctx->M();
        vp.keys = keys;
        vp.bg = (flags & ARVX_MESH_COLOR_FOREGROUND) ? ctx->bg() : nullptr;
        vp.bgWords = ctx->bgWords;
        vp.images = ctx->images();
        vp.average = mode == ARVX_COLOR_AVERAGE;
        vp.tol = tolerance;
        vp.rgb = ctx->pool_mcol_rgb.data();
        vp.views = ctx->pool_mcol_views.data();
        vp.coloured = &head->coloured;
        ARVX_TRY(by_assoc(ctx, [&](auto left) {
            return launch(ctx, arvx::mesh_color_vote_kernel<decltype(left)::value>, blocks_for(m.V), 256, vp);
        }));
        ARVX_HIP(hipMemcpyAsync(&n_coloured, &head->coloured, sizeof n_coloured, hipMemcpyDeviceToHost, ctx->stream));
    }
    ARVX_SYNC(ctx);
    if (faces) ctx->mesh_color_need = std::max(ctx->word(Ctx::kMeshColorNeed), 0ll);
    ctx->mesh_color_source = source;
    ctx->mesh_color_V = V, ctx->mesh_color_W = W, ctx->mesh_color_H = H;
    ctx->mesh_color_verts = m.V;
    *coloured = ctx->mesh_color_coloured = (int64_t)n_coloured;
    ctx->mesh_color_ready = true;
    return ARVX_OK;
}

int arvx_mesh_color_count(arvx_ctx *ctx, int64_t *vertices, int64_t *coloured) {
    ARVX_CHECK_CTX(ctx);
    if (!ctx->mesh_color_ready) return fail(ARVX_ERR_STATE, "no image colours (call arvx_mesh_color)");
    if (vertices) *vertices = ctx->mesh_color_verts;
    if (coloured) *coloured = ctx->mesh_color_coloured;
    return ARVX_OK;
}

int arvx_mesh_color_download(arvx_ctx *ctx, float *vertex_rgb, int32_t *views) {
    ARVX_CHECK_CTX(ctx);
    if (!ctx->mesh_color_ready) return fail(ARVX_ERR_STATE, "no image colours (call arvx_mesh_color)");
    const size_t Vn = (size_t)ctx->mesh_color_verts;
    ARVX_TRY(download(ctx, vertex_rgb, ctx->pool_mcol_rgb.data(), Vn, Ctx::kVertexBytes));
    ARVX_TRY(download(ctx, views, ctx->pool_mcol_views.data(), Vn, sizeof(int32_t)));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

int arvx_mesh_color_depth_download(arvx_ctx *ctx, int view, float *depth) {
    ARVX_CHECK_CTX(ctx);
    if (!ctx->mesh_color_ready) return fail(ARVX_ERR_STATE, "no image colours (call arvx_mesh_color)");
    if (view < 0 || view >= ctx->mesh_color_V)
        return fail(ARVX_ERR_INVALID, "view %d outside [0,%d)", view, ctx->mesh_color_V);
    if (!depth) return fail(ARVX_ERR_INVALID, "null depth");
    const size_t npix = (size_t)ctx->mesh_color_W * ctx->mesh_color_H;
    ARVX_HIP(ctx->pool_mcol_depth.reserve(npix * sizeof(float)));
    ARVX_TRY(launch(ctx, arvx::mesh_color_depth_kernel, blocks_for(npix), 256,
                    (const unsigned long long *)ctx->pool_mcol_keys.p + (size_t)view * npix, npix,
                    ctx->pool_mcol_depth.data()));
    ARVX_TRY(download(ctx, depth, ctx->pool_mcol_depth.data(), npix, sizeof(float)));
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

int arvx_selftest_mesh_color_batch(arvx_ctx *ctx, int views_per_batch) {
    ARVX_CHECK_CTX(ctx);
    if (views_per_batch < 0) return fail(ARVX_ERR_INVALID, "views_per_batch %d (0: the default bound)", views_per_batch);
    ctx->mesh_color_batch = views_per_batch;
    return ARVX_OK;
}

// ---- mesh textures from the images (mesh_texture_kernels.h) ----------------------------------

int arvx_mesh_texture(arvx_ctx *ctx, int source, int resolution, int atlas_width, float tolerance, unsigned flags,
                      int64_t out[4]) {
    ARVX_CHECK_CTX(ctx);
    if (!whole_grid(ctx)) return fail(ARVX_ERR_STATE, "arvx_mesh_texture needs a whole-grid context");
    MeshSource m;
    if (int rc = mesh_source(ctx, source, m, false)) return rc;
    if (resolution < 1 || resolution > ARVX_MESH_TEXTURE_MAX_RESOLUTION)
        return fail(ARVX_ERR_INVALID, "resolution %d outside [1,%d]", resolution, ARVX_MESH_TEXTURE_MAX_RESOLUTION);
    if (atlas_width < resolution + 3 || atlas_width > ARVX_MESH_TEXTURE_MAX_WIDTH)
        return fail(ARVX_ERR_INVALID, "atlas width %d outside [%d,%d]", atlas_width, resolution + 3,
                    ARVX_MESH_TEXTURE_MAX_WIDTH);
    if (flags & ~ARVX_MESH_TEXTURE_FOREGROUND) return fail(ARVX_ERR_INVALID, "unknown flag bits %#x", flags);
    if (std::isnan(tolerance) || tolerance < 0.f)
        return fail(ARVX_ERR_INVALID, "tolerance %g: must be >= 0 (finite or +inf)", (double)tolerance);
    if (!out) return fail(ARVX_ERR_INVALID, "null out");
    if (m.T > (long long)UINT32_MAX) return fail(ARVX_ERR_STATE, "the mesh is too long");
    {  // (the height before anything is laid out: rows of cells times ch)
        const long long per_row = atlas_width / (resolution + 3), cells = (m.T + 1) / 2;
        const long long AH = (cells + per_row - 1) / per_row * (resolution + 2);
        if (AH > ARVX_MESH_TEXTURE_MAX_HEIGHT)
            return fail(ARVX_ERR_INVALID, "an atlas %d wide would be %lld high (at most %d): widen it", atlas_width, AH,
                        ARVX_MESH_TEXTURE_MAX_HEIGHT);
    }
    if (!ctx->cameras_ready) return fail(ARVX_ERR_STATE, "arvx_set_views has not been called");
    if (!ctx->images_ready) return fail(ARVX_ERR_STATE, "arvx_set_images has not been called");
    if ((flags & ARVX_MESH_TEXTURE_FOREGROUND) && !ctx->views_ready)
        return fail(ARVX_ERR_STATE, "ARVX_MESH_TEXTURE_FOREGROUND: arvx_set_views was given no masks");
    ctx->mesh_texture_ready = false;
    const int V = ctx->V, W = ctx->W, H = ctx->H;
    const size_t npix = (size_t)W * H;
    const arvx::TextureLayout lay = arvx::texture_layout(m.T, resolution, atlas_width);
    const size_t ntex = (size_t)lay.AW * (size_t)lay.AH;
    const int words = (V + 31) / 32;
    unsigned long long n_textured = 0;
    if (m.T > 0 && m.V > 0) {
        ARVX_HIP(ctx->pool_mtex_keys.reserve((size_t)V * npix * sizeof(unsigned long long)));
        ARVX_HIP(ctx->pool_mtex_bits.reserve((size_t)words * (size_t)m.V * sizeof(uint32_t)));
        ARVX_HIP(ctx->pool_mtex_count.reserve(sizeof(unsigned long long)));
        ARVX_HIP(ctx->pool_mtex_view.reserve((size_t)m.T * sizeof(int)));
        ARVX_HIP(ctx->pool_mtex_atlas.reserve(ntex * 3));
        unsigned long long *keys = (unsigned long long *)ctx->pool_mtex_keys.p;
        unsigned long long *count = (unsigned long long *)ctx->pool_mtex_count.p;
        ARVX_TRY(mesh_depth_pass(ctx, m, keys));
        ARVX_HIP(hipMemsetAsync(count, 0, sizeof *count, ctx->stream));
        arvx::MeshVisibleParams vp{};
        vp.verts = m.verts;
        vp.Vn = m.V;
        vp.s = ctx->s;
        vp.V = V, vp.W = W, vp.H = H, vp.words = words;
        vp.M = (const arvx::SelftestMatrix *)ctx->M();
        vp.keys = keys;
        vp.bg = (flags & ARVX_MESH_TEXTURE_FOREGROUND) ? ctx->bg() : nullptr;
        vp.bgWords = ctx->bgWords;
        vp.tol = tolerance;
        vp.bits = (uint32_t *)ctx->pool_mtex_bits.p;
        arvx::MeshSelectParams sp{};
        sp.verts = m.verts, sp.faces = m.faces;
        sp.Vn = m.V, sp.T = m.T;
        sp.s = ctx->s;
        sp.V = V, sp.words = words;
        sp.M = vp.M;
        sp.bits = vp.bits;
        sp.face_view = ctx->pool_mtex_view.data();
        sp.textured = count;
        arvx::MeshFillParams fp{};
        fp.verts = m.verts, fp.col = m.rgb, fp.faces = m.faces;
        fp.Vn = m.V;
        fp.s = ctx->s;
        fp.W = W, fp.H = H;
        fp.M = vp.M;
        fp.images = ctx->images();
        fp.face_view = sp.face_view;
        fp.lay = lay;
        fp.atlas = ctx->pool_mtex_atlas.data();
        ARVX_TRY(by_assoc(ctx, [&](auto left) {
            constexpr bool L = decltype(left)::value;
            ARVX_TRY(launch(ctx, arvx::mesh_texture_visible_kernel<L>, blocks_for(m.V), 256, vp));
            ARVX_TRY(launch(ctx, arvx::mesh_texture_select_kernel<L>, blocks_for(m.T), 256, sp));
            return launch(ctx, arvx::mesh_texture_fill_kernel<L>, blocks_for(ntex, 1024), 256, fp);  // (4 texels a lane)
        }));
        ARVX_HIP(hipMemcpyAsync(&n_textured, count, sizeof n_textured, hipMemcpyDeviceToHost, ctx->stream));
        ARVX_SYNC(ctx);
        ctx->mesh_color_need = std::max(ctx->word(Ctx::kMeshColorNeed), 0ll);
    }
    ctx->mesh_texture_source = source;
    ctx->mesh_texture_R = resolution, ctx->mesh_texture_AW = lay.AW;
    ctx->mesh_texture_AH = m.T > 0 && m.V > 0 ? lay.AH : 0;
    ctx->mesh_texture_faces = m.T > 0 && m.V > 0 ? m.T : 0;
    ctx->mesh_texture_textured = (int64_t)n_textured;
    ctx->mesh_texture_ready = true;
    return arvx_mesh_texture_info(ctx, out);
}

int arvx_mesh_texture_info(arvx_ctx *ctx, int64_t out[4]) {
    ARVX_CHECK_CTX(ctx);
    if (!out) return fail(ARVX_ERR_INVALID, "null out");
    if (!ctx->mesh_texture_ready) return fail(ARVX_ERR_STATE, "no texture (call arvx_mesh_texture)");
    out[0] = ctx->mesh_texture_faces, out[1] = ctx->mesh_texture_textured;
    out[2] = ctx->mesh_texture_AW, out[3] = ctx->mesh_texture_AH;
    return ARVX_OK;
}

int arvx_mesh_texture_download(arvx_ctx *ctx, uint8_t *atlas_bgr, int32_t *face_view, float *face_uv) {
    ARVX_CHECK_CTX(ctx);
    if (!ctx->mesh_texture_ready) return fail(ARVX_ERR_STATE, "no texture (call arvx_mesh_texture)");
    const size_t T = (size_t)ctx->mesh_texture_faces;
    const arvx::TextureLayout lay = arvx::texture_layout((long long)T, ctx->mesh_texture_R, ctx->mesh_texture_AW);
    ARVX_TRY(download(ctx, atlas_bgr, ctx->pool_mtex_atlas.data(), (size_t)lay.AW * (size_t)lay.AH, 3));
    ARVX_TRY(download(ctx, face_view, ctx->pool_mtex_view.data(), T, sizeof(int32_t)));
    for (size_t f = 0; face_uv && f < T; ++f) {  // (the layout is the same arithmetic on the host)
        static const int ci[3] = {0, 1, 0}, cj[3] = {0, 0, 1};
        for (int k = 0; k < 3; ++k) {
            int x, y;
            arvx::texture_texel(lay, (long long)f, ci[k] * lay.R, cj[k] * lay.R, x, y);
            face_uv[6 * f + 2 * k] = ((float)x + 0.5f) / (float)lay.AW;
            face_uv[6 * f + 2 * k + 1] = ((float)y + 0.5f) / (float)lay.AH;
        }
    }
    ARVX_SYNC(ctx);
    return ARVX_OK;
}

int arvx_closure_download32(arvx_ctx *ctx, int32_t *index, float *rgba) {
    ARVX_CHECK_CTX(ctx);
    if (!index || !rgba) return fail(ARVX_ERR_INVALID, "null argument");
    if (!ctx->closure_ready) return fail(ARVX_ERR_STATE, "no closure result (call arvx_closure)");
    if (int rc_h = clo_host(ctx)) return rc_h;
    size_t lo, hi;
    long long base;
    owned_part(ctx, ctx->h_clo_index, lo, hi, base);
    if (hi > lo) {
        if (base == 0) memcpy(index, ctx->h_clo_index.data() + lo, (hi - lo) * sizeof(int32_t));
        else for (size_t k = lo; k < hi; ++k) index[k - lo] = (int32_t)(ctx->h_clo_index[k] - base);
        ARVX_HIP(hipMemcpyAsync(rgba, (const float4 *)ctx->d_clo_rgba + lo,
                                (hi - lo) * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
        ARVX_SYNC(ctx);
    }
    return ARVX_OK;
}

// ---- greedy carve -------------------------------------------------------------------

int arvx_fast_carve(arvx_ctx *ctx) {
    ARVX_CHECK_CTX(ctx);
    if (!ctx->views_ready) return fail(ARVX_ERR_STATE, "arvx_set_views has not been called");
    if (!whole_grid(ctx))
        return fail(ARVX_ERR_STATE,
                    "arvx_fast_carve needs the whole grid in one context (connectivity is global)");
    ctx->drop(Event::FastCarve);
    arvx::FloodParams fp;
    // a fresh model (the usual case: src/main.cpp calls fastCarve on a new Model) is neither
    // filled nor read: the kernels know its records, and flood_apply_rec_kernel writes them all
    fp.fresh = ctx->form == Form::Fresh ? 1 : 0;
    if (fp.fresh) {
        if (int rc = ensure_records(ctx, ctx->pool_rec)) return rc;
    } else if (int mrc = need_rec(ctx)) {
        return mrc;
    }
    fp.X = ctx->X;
    fp.Y = ctx->Y;
    fp.Z = ctx->Z;
    fp.XW = (ctx->X + 63) / 64;
    const size_t nwords = (size_t)fp.XW * fp.Y * fp.Z;
    const int tilesY = (fp.Y + 15) / 16, tilesZ = (fp.Z + 15) / 16;
    const int tile_rows = tilesY * tilesZ;
    const unsigned gflood = (unsigned)((size_t)fp.XW * tile_rows);
    const bool prepass = fp.XW <= 64 && tile_rows <= arvx::kFloodMaxTileRows;

    // one work buffer, kept by the context: open, reach bit planes | whole-tile rows (full,
    // reached) | wake flags (2 x tiles) | changed flag
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_bits = 0;
    const size_t o_tiles = o_bits + up(2 * nwords * sizeof(unsigned long long));
    const size_t o_dirty = o_tiles + up(2 * (size_t)tile_rows * sizeof(unsigned long long));
    const size_t o_changed = o_dirty + up(2 * (size_t)gflood);
    const size_t need = o_changed + 256;
    ARVX_HIP(ctx->pool_flood.reserve(need));
    uint8_t *base = (uint8_t *)ctx->pool_flood.p;
    fp.open = (unsigned long long *)(base + o_bits);
    fp.reach = fp.open + nwords;
    unsigned long long *d_tiles = (unsigned long long *)(base + o_tiles);
    uint8_t *d_dirty = base + o_dirty;
    fp.changed = (int *)(base + o_changed);
    fp.dirty_cur = fp.dirty_next = nullptr;  // set per launch of flood_step_kernel

    // carvable = what the dense carve clears on a fresh model: carved into records of its own
    if (int rc = ensure_records(ctx, ctx->pool_flood_rec)) return rc;
    arvx::CarveParams g = record_params(ctx);
    // (the coarse tiles that carve settles as a whole exist only as their codes, as in the model's
    // own lazy state: no N / 4 bytes of constants written here and read back by the conversion)
    const size_t ncoarse_f = (size_t)g.coarseX * g.coarseY * g.coarseZ;
    ARVX_HIP(ctx->pool_flood_code.reserve(ncoarse_f + 64));
    uint8_t *d_carv_code = (uint8_t *)ctx->pool_flood_code.p;
    if (int rc = launch_carve(ctx, (uint16_t *)ctx->pool_flood_rec.p, 0, ctx->V, 0, true, d_carv_code)) return rc;
    // (both conversions: one workgroup per row of tiles, 64 rows x (tiles along x + 1) words
    // of LDS, twice that for the way back)
    const int chunk = std::min(arvx::kFloodChunk, fp.XW);
    const size_t lds_words = (size_t)64 * (chunk + 1);
    ARVX_TRY(launch(ctx, arvx::flood_open_from_rec_kernel, (unsigned)(g.tilesY * g.tilesZ), 256,
                    Lds{lds_words * sizeof(unsigned long long)}, g, (const uint16_t *)ctx->pool_flood_rec.p,
                    d_carv_code, fp));
    // whole-tile pre-pass (fast_carve_kernels.h): seeds every completely open tile
    // that is connected to the origin tile through completely open tiles
    if (prepass) {
        const size_t tile_bytes = 2 * (size_t)tile_rows * sizeof(unsigned long long);
        ARVX_TRY(launch(ctx, arvx::flood_tile_full_kernel, tile_rows, 256, fp, d_tiles, d_dirty));
        ARVX_TRY(launch(ctx, arvx::flood_tile_fill_kernel, 1, 1024, Lds{tile_bytes}, d_tiles,
                        d_tiles + tile_rows, tilesY, tilesZ));
        ARVX_TRY(launch(ctx, arvx::flood_tile_seed_kernel, tile_rows, 256, fp, d_tiles + tile_rows));
    }
    // per-tile wake flags, two buffers swapped every launch; without the pre-pass
    // (which sets the first buffer) all tiles are awake at first
    if (!prepass) ARVX_HIP(hipMemsetAsync(d_dirty, 1, gflood, ctx->stream));
    ARVX_HIP(hipMemsetAsync(d_dirty + gflood, 0, gflood, ctx->stream));
    // every launch that is not the last grows at least one word; the launches of a batch write
    // one flag each, read back after 4, 4, 8, 8, ... launches: the fill has converged when the
    // LAST launch of a batch changed nothing (a launch with no tile awake costs microseconds)
    const long max_launches = 128 + (long)gflood * 256;
    long launched = 0;
    int *const flags = fp.changed;
    for (int batch = 4, round = 0;; ++round) {
        int changed[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        ARVX_HIP(hipMemsetAsync(flags, 0, 8 * sizeof(int), ctx->stream));
        for (int k = 0; k < batch; ++k, ++launched) {
            fp.dirty_cur = d_dirty + (launched & 1) * (size_t)gflood;
            fp.dirty_next = d_dirty + ((launched + 1) & 1) * (size_t)gflood;
            fp.changed = flags + k;
            ARVX_TRY(launch(ctx, arvx::flood_step_kernel, gflood, 256, fp));
        }
        ARVX_HIP(hipMemcpyAsync(changed, flags, 8 * sizeof(int), hipMemcpyDeviceToHost,
                                ctx->stream));
        ARVX_SYNC(ctx);
        if (!changed[batch - 1]) break;
        if (launched >= max_launches) return fail(ARVX_ERR_HIP, "flood fill did not converge");
        if (round >= 1 && batch < 8) batch *= 2;
    }
    const unsigned rows = (unsigned)((g.coarseY << g.cyShift) * (g.coarseZ << g.czShift));
    ARVX_TRY(launch(ctx, arvx::flood_apply_rec_kernel, rows, 256, Lds{2 * lds_words * sizeof(unsigned long long)},
                    g, fp));
    ctx->form = Form::Records;  // the records now hold every voxel's state
    ARVX_SYNC(ctx);
    // (arvx_last_fast_carve_path: all of it once the carve is through, or nothing)
    ctx->flood_bits = (prepass ? ARVX_FLOOD_PREPASS : 0u) | (fp.fresh ? ARVX_FLOOD_FRESH : 0u);
    ctx->flood_launches = (unsigned)launched;
    ctx->flood_tile_rows = (unsigned)tile_rows;
    ctx->flood_off_reached = prepass ? o_tiles + (size_t)tile_rows * sizeof(unsigned long long) : 0;
    return ARVX_OK;
}

int arvx_last_fast_carve_path(arvx_ctx *ctx, uint32_t out[4]) {
    ARVX_CHECK_CTX(ctx);
    if (!out) return fail(ARVX_ERR_INVALID, "null out");
    out[0] = ctx->flood_bits;
    out[1] = 0;
    out[2] = ctx->flood_launches;
    out[3] = ctx->flood_tile_rows;
    if (!ctx->flood_off_reached) return ARVX_OK;  // no pre-pass (or no greedy carve yet)
    // the rows the pre-pass left in the work buffer: bit xw of row (ty, tz) = tile seeded
    std::vector<unsigned long long> rows(ctx->flood_tile_rows);
    ARVX_SYNC(ctx);
    ARVX_HIP(hipMemcpy(rows.data(), (const uint8_t *)ctx->pool_flood.p + ctx->flood_off_reached,
                       rows.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    uint32_t seeded = 0;
    for (unsigned long long w : rows) seeded += (uint32_t)__builtin_popcountll(w);
    out[1] = seeded;
    return ARVX_OK;
}

}  // extern "C"
