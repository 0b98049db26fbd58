// arvx_ctx.h -- the opaque context behind the C-ABI (include/arvx/arvx.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace arvx {

int fail_hip(hipError_t e, const char *what, const char *file, int line);
int fail_msg(int code, const char *msg);

#define ARVX_HIP(call)                                                        \
    do {                                                                      \
        hipError_t arvx_e_ = (call);                                          \
        if (arvx_e_ != hipSuccess)                                            \
            return ::arvx::fail_hip(arvx_e_, #call, __FILE__, __LINE__);      \
    } while (0)

// Grow-only device buffer: results of repeated calls reuse the allocation (hipMalloc / hipFree of
// tens of MB cost more than the kernels that fill them).  It owns its memory: freed when the buffer
// grows and when the context goes.  Headroom: a quarter more than asked for, for lists whose length
// varies from call to call; Exact: what was asked for, for buffers whose size follows the grid, the
// views or the call's arguments.
struct DevPool {
    enum Size { Headroom, Exact };
    void *p = nullptr;
    size_t cap = 0;
    const bool exact;
    explicit DevPool(Size size = Headroom) : exact(size == Exact) {}
    DevPool(const DevPool &) = delete;
    DevPool &operator=(const DevPool &) = delete;
    ~DevPool() { release(); }
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        release();
        const size_t want = exact ? bytes : bytes + bytes / 4;
        const hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};
// A pool that holds one array: of what is said here, once.
template <class T>
struct DevArray : DevPool {
    T *data() const { return (T *)p; }
};
struct SparseWord;  // bitplane_kernels.h

struct Ctx {
    int device = 0;
    int X = 0, Y = 0, Z = 0;  // full grid
    int z0 = 0, z1 = 0;       // slab owned here
    int ze0 = 0, ze1 = 0;     // slab plus `halo` planes each side (clipped to the grid)
    int halo = 1;             // halo planes per inner side (arvx_ctx_create_slab_halo)
    int stripe_world = 1, stripe_rank = 0;  // striped slabs (arvx_ctx_create_striped)
    float s = 0.f;
    int assoc = 1;        // grouping of the M * world row sums (ARVX_ASSOC_*, arvx_device.h)
    size_t nvox = 0;      // owned voxels
    size_t nvox_ext = 0;  // voxels in the state buffer (owned + halo)

    // Kernels that wait for other workgroups inside a launch (views_strip_kernel, the streaming
    // carve) give up after seconds and leave a mark here instead of hanging the device: one word of
    // page-locked host memory the device writes directly, read by the host after its next
    // synchronisation (arvx_capi.hip, check_fault).  Never seen set by a kernel; the host's side of
    // it -- the call fails, the next one starts from clean control blocks -- is exercised by
    // tests/test_fault_gpu.py through the experiment build's arvx_experiment_mark_fault.
    unsigned *h_fault = nullptr;  // host address
    unsigned *d_fault = nullptr;  // the same word as the device sees it
    // The count words: 8-byte words of the same page-locked block, from byte 8 on, that kernels write
    // a length or a count to and the host reads after the call's synchronisation.  One word per
    // user, none shared.  The list lengths also have a copy on the device, for the kernels that
    // follow in the same call (arvx_capi.hip, device_total): the words below kDeviceTotals.
    enum Word {
        kSurface, kClosure, kCells, kTris, kVerts,  // list lengths, in the device copies' order
        kSmoothScan,                    // arvx_mc_mesh_smooth's offset scans: a total nobody reads
        kComponents,                    // the component table's length (arvx_components[_keep])
        kDecVerts, kDecTris,            // arvx_mc_mesh_decimate: decimated vertices, surviving faces
        kRefVerts,                      // arvx_mc_mesh_refined: cut edges (kCells and kTris carry its other lists)
        kRelaxScan,                     // arvx_mesh_relax's offset scans: a total nobody reads
        kDeviceTotals,
        kPhotoRemoved = kDeviceTotals,  // voxels an iteration of arvx_photo_carve removed
        kVisNeed,                       // large footprints the visible pass wanted to list
        kPacketOcc, kPacketSeen,        // arvx_state_download_packets: the two packets' words
        kCompKept, kCompRemoved,        // arvx_components_keep: components left, voxels emptied
        kRenderNeed, kRenderAgree,      // the render's large footprints; three agreement counts in a row
        kRectMiss = kRenderAgree + 3,   // a block's rectangle did not fit its table entry (rect_cache_kernels.h)
        kMorphChanged,                  // arvx_morph: voxels that left or joined the model
        kRenderMeshNeed,                // the triangle render's large pixel boxes
        kMeshColorNeed,                 // arvx_mesh_color: the large pixel boxes of its fullest batch
        kWords
    };
    static constexpr size_t kHostBlockBytes = 256;
    static_assert(8 + 8 * (size_t)kWords <= kHostBlockBytes, "the count words fit the block");
    long long &word(int w) const { return ((long long *)(h_fault + 2))[w]; }      // host value
    long long *word_dev(int w) const { return (long long *)(d_fault + 2) + w; }  // device address
    DevPool pool_vstrip;          // views_strip_kernel: ticket counters + published column counts
    size_t vstrip_key = 0;        // layout (V, strips, granules) the pool was zeroed for

    // scan_lookback_kernel (bitplane_kernels.h): ticket counter, device totals, status granules; and
    // what the host keeps beside it.
    DevPool pool_compact;
    // set bits per kBitChunk words of the plane being compacted: two buffers of counts_stride
    // ints used in turn (the compaction that reads one zeroes the other: arvx_capi.hip, chunk_counts)
    DevPool pool_chunk_counts;
    size_t counts_stride = 0;
    int counts_cur = 0;
    bool counts_clean[2] = {false, false};
    size_t counts_used[2] = {0, 0};  // chunks of the plane whose producer last added into each buffer
    unsigned long long compact_tickets = 0;  // tickets all launches so far have taken
    uint32_t compact_epoch = 0;
    long long surf_host_count = -1;  // entries of h_surf_index / h_surf_has that are valid (-1: fetch)
    long long clo_host_count = -1;   // ... of h_clo_index

    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t xstream = nullptr;  // arvx_ctx_set_exchange_stream: the occupancy hand-off (null: stream)

    // The state lives in sub-tile RECORDS (csrc/arvx_device.h), 2 bits per voxel: what every
    // stage reads and writes.  The one-byte-per-voxel plane of the C-ABI (arvx_state_upload /
    // _download / _device_ptr) is a staging buffer, allocated on demand and converted from / to
    // the records inside those calls; bit2 of uploaded bytes (voxel painted UNSEEN_COLOR by a
    // host Model) is kept beside the records as one bit plane (`paint`).
    // The state's form.  Fresh: a fresh model (all occupied, none seen) that exists only as this
    // value -- need_rec writes it out, a carve of it writes every record without reading one.
    // Records: pool_rec holds the state.  Lazy: as Records, but the coarse tiles the carve of a
    // fresh model settled as a whole exist only as their code in pool_ccode (arvx_device.h);
    // their records are not written.
    enum class Form { Fresh, Records, Lazy };
    Form form = Form::Fresh;
    DevPool pool_rec{DevPool::Exact};  // records of planes ze0..ze1-1 (+ padding to whole coarse tiles)
    uint16_t *rec() const { return (uint16_t *)pool_rec.p; }
    DevPool pool_ccode;
    // every call that changes occupied / seen bits counts here.  What is derived from the state
    // carries the count it was built at as its stamp (0: none): it is current while that count
    // still stands
    unsigned long long state_seq = 1;
    // the colour pass's bit planes of the state (occupied; seen by no view), kept for a closure that
    // follows; planes_unseen: handleUnseen has run since (the records' occupancy is the occupancy
    // plane | the never-seen plane: next_state)
    DevPool pool_state_planes;  // occupancy plane, then never-seen plane (planes_words words each)
    size_t planes_words = 0;
    unsigned long long planes_seq = 0;
    bool planes_unseen = false;
    DevPool pool_state_packets;  // arvx_state_download_packets: occupancy | seen, worst-case size each
    unsigned long long packets_seq = 0;
    long long packet_need[2] = {0, 0};
    DevPool pool_cstate;         // per coarse tile: settled by earlier carves (CarveParams::cstate)
    size_t cstate_tiles = 0;     // ... valid for this many tiles of the current layout (0: not)
    DevPool pool_state_bytes{DevPool::Exact};  // byte staging, planes ze0..ze1-1 (allocated on demand)
    uint8_t *owned() const { return (uint8_t *)pool_state_bytes.p + (size_t)(z0 - ze0) * X * Y; }
    DevPool pool_paint;          // bit plane (bitplane_kernels.h layout) over planes ze0..ze1-1
    bool paint_valid = false;    // some voxel is painted: the plane takes part in the stages
    int ncu = 0;                 // compute units that size the launches: the device's (cached), or
    int ncu_device = 0;          // ... fewer of them (arvx_selftest_compute_units); the device's own
    int carve_seq = 0;           // parity of the undecided-list counters (carve_coarse_kernel)
    size_t carve_layout = 0;     // pool_coarse layout those counters were zeroed for
    // arvx_last_carve_path: the last launch_carve's ARVX_PATH_* bits, its dense classify grid, and
    // where in pool_coarse its list length and work-list counters are (0: it had none)
    unsigned path_bits = 0, path_dense_grid = 0;
    size_t path_off_listed = 0, path_off_work = 0;
    // arvx_last_fast_carve_path: the last arvx_fast_carve's ARVX_FLOOD_* bits, its flood_step_kernel
    // launches and its tile rows, and where in pool_flood the whole-tile pre-pass left its `reached`
    // rows (0: it did not run).  All zero before the first greedy carve and once the state it left
    // has been replaced (drop).
    unsigned flood_bits = 0, flood_launches = 0, flood_tile_rows = 0;
    size_t flood_off_reached = 0;
    // the streaming carve (carve_stream_kernels.h): control block + list entries + item queues
    DevPool pool_stream{DevPool::Exact};
    size_t stream_layout = 0;    // layout the control block was zeroed for (0: zero it again)
    unsigned carve_epoch = 0;    // tag of the latest streaming launch's granules
    DevPool pool_timeline{DevPool::Exact};  // ARVX_TIMELINE diagnostic builds only
    int64_t timeline_n = 0;
    int timeline_rec = 32;  // bytes per record
    DevPool pool_flood_rec{DevPool::Exact};  // records of the "carvable" plane of arvx_fast_carve
    DevPool pool_flood_code;      // ... and the codes of the coarse tiles that exist only as a code
    DevPool pool_coarse{DevPool::Exact};  // coarse pre-pass masks of the carve kernel
    DevPool pool_stats{DevPool::Exact};   // 8 counters + flags
    unsigned long long *stats() const { return (unsigned long long *)pool_stats.p; }
    // times a list total had to be fetched from the device because the page-locked word still
    // read -1 at the synchronisation (host_total, arvx_capi.hip); expected: never
    unsigned long long host_total_fallbacks = 0;
    DevPool pool_scratch{DevPool::Exact};  // work buffer of the calls on `stream`
    // work buffer of the hand-off calls (arvx_occupancy_compress): they may run on `xstream`
    // BESIDE a set_views / carve on `stream`, so they never touch pool_scratch
    DevPool pool_xscratch;
    DevPool pool_flood{DevPool::Exact};  // work buffer of arvx_fast_carve, kept between calls

    // views
    bool views_ready = false;    // matrices + bit planes + tables: the carve can run
    bool cameras_ready = false;  // matrices (+ camera positions): enough for the colour pass
    bool has_campos = false;
    int V = 0, W = 0, H = 0;
    int bgWords = 0, satStride = 0;
    int satW = 0, satH = 0;  // summed-area table: satH = H + 1 rows of satW >= W + 1 entries
    // V x 12 matrices, V x 3 camera positions, V x bgWords background words, V x satStride table
    // entries: allocated for one number and size of views
    DevPool pool_M{DevPool::Exact}, pool_campos{DevPool::Exact}, pool_bg{DevPool::Exact},
        pool_sat{DevPool::Exact};
    float *M() const { return (float *)pool_M.p; }
    float *campos() const { return (float *)pool_campos.p; }
    uint32_t *bg() const { return (uint32_t *)pool_bg.p; }
    uint16_t *sat() const { return (uint16_t *)pool_sat.p; }
    std::vector<float> h_M, h_campos;
    // Cached rectangles (carve_kernels.h, rect_cache_kernels.h): what the carve's rectangle
    // arithmetic answers for every (4 x 4 x 4 block, view) of this context's grid, kept while the
    // matrices, V, W and H stand -- the masks do not enter.  Built at the second consecutive carve
    // of a fresh model that runs the dense classify kernel and the unshared block-mapped exact
    // kernel -- the instantiation that reads the table -- under the same views (rect_streak counts
    // them), and only while the table fits rect_limit bytes.  Refused: not
    // tried again for these views (it does not fit the limit or the device, or a block's rectangle
    // does not fit an entry).  New matrices take it back to None (views_common); free_views
    // releases the table; the events of drop() do not touch it.
    enum class Rect { None, Built, Refused };
    Rect rect_state = Rect::None;
    int rect_streak = 0;
    size_t rect_limit = (size_t)1 << 30;  // arvx_ctx_set_rect_cache_limit (0: no table)
    DevPool pool_rect{DevPool::Exact};
    // Cached pixels (carve_kernels.h table_view_blocks, pixel_cache_kernels.h): one byte per (voxel,
    // view), the pixel the exact kernel's projection gives, relative to the origin of the block's
    // cached rectangle.  Built right after the block table and only while that stands, under a
    // limit of its own (pix_limit); it also follows the grouping of the row sums (pix_assoc: built
    // again when that changes).  pix_miss: bit v = some pixel of view v does not fit its byte (the
    // device's words follow the table in pool_pix); such a view is projected as before.
    Rect pix_state = Rect::None;
    int pix_assoc = 0;
    size_t pix_limit = (size_t)6 << 30;  // arvx_ctx_set_pixel_cache_limit (0: no table)
    DevPool pool_pix{DevPool::Exact};
    std::vector<unsigned long long> pix_miss;
    void rect_invalidate() {
        rect_state = Rect::None;
        pix_state = Rect::None;
        rect_streak = 0;
        win_valid = false;  // (the windows follow the same inputs as the cached rectangles)
    }
    // View windows (arvx_capi.hip, view_window): per view the tiles of the summed-area table that
    // a rectangle test of this context's grid can read, as one word I0 | I1 << 8 | J0 << 16 |
    // J1 << 24 (strips I0..I1, tile columns J0..J1 of views_strip_kernel, inclusive).  They follow
    // the matrices, V, W, H, the voxel size and the grid, not the masks: derived again where the
    // cached rectangles are invalidated, sent to the device only when a word differs.
    // sat_partial: the last derivation left entries outside some window unwritten (stale or never
    // written); only rectangle tests of boxes of this grid may read the table while it stands
    // (complete_tables, arvx_capi.hip, clears it).
    bool win_on = true;      // arvx_ctx_set_view_window
    bool win_valid = false;  // h_win is that of the current matrices and sizes
    bool sat_partial = false;
    std::vector<uint32_t> h_win_geo;  // the cameras' windows (while win_valid)
    std::vector<uint32_t> h_win;      // what the device holds in pool_win: the last derivation's
    DevPool pool_win{DevPool::Exact};

    // arvx_segment_views (segment_kernels.h): two work planes of V x H rows of whole 64-bit words (the
    // final masks are plane seg_final; read only while seg_ready is set: the views are still the ones the
    // call derived), eight count words per view, the labels and areas of one batch of views (an int32
    // each per pixel) before the batch's "largest" words, the plates of the host form, a view as bytes
    DevPool pool_seg_planes{DevPool::Exact}, pool_seg_counts{DevPool::Exact}, pool_seg_label{DevPool::Exact},
        pool_seg_plates{DevPool::Exact}, pool_seg_bytes{DevPool::Exact};
    bool seg_ready = false;
    int seg_final = 0;
    int seg_batch = 0;  // arvx_selftest_segment_batch (0: the bound)

    // colour pass
    DevPool pool_images{DevPool::Exact};  // V x H x W x 3, BGR
    uint8_t *images() const { return (uint8_t *)pool_images.p; }
    bool images_ready = false;
    int *d_surf_index = nullptr;      // compacted flat indices (slab-local)
    float4 *d_surf_rgba = nullptr;    // r, g, b, has-sample flag per surface voxel
    float *d_surf_depth = nullptr;    // minimum sample depth per surface voxel
    uint8_t *d_surf_has = nullptr;    // 1 if the voxel received >= 1 sample
    int64_t surf_count = 0;           // occupied non-inner voxels found (planes c_lo .. c_hi)
    // Index lists (d_surf_index, d_clo_index) hold flat indices over the context's planes
    // ze0 .. ze1 - 1 (x + X * (y + Y * (z - ze0))): a slab with a halo wider than one plane
    // colours / closes some halo planes too, because its OWNED cells and voxels need their
    // neighbours' results (stage_ranges in arvx_capi.hip).  What the download calls return is
    // the owned part, relative to the owned planes.
    std::vector<int> h_surf_index;    // host copy (ascending)
    std::vector<uint8_t> h_surf_has;
    bool color_ready = false;         // the colour list: the fields above are read only while set
    // the list's plane and its index (bitplane_kernels.h, SparseWord) over the owned planes
    DevPool pool_col_bits, pool_col_rank;
    // arvx_color_visible: the colour list is its result (read only while color_ready is set too);
    // the views' depth buffers (V x H x W), the large-footprint list behind its counter, and the
    // number of views each list entry is visible in
    bool color_visible = false;
    long long vis_large_need = 0;  // large footprints the last call wanted to list (sizes the list)
    DevPool pool_vis_depth{DevPool::Exact}, pool_vis_large{DevPool::Exact}, pool_vis_views;
    // arvx_photo_carve: the removal counter (64 bytes) before one removal word per 64 list entries;
    // the removal plane (bitplane_kernels.h layout)
    DevPool pool_photo_rm, pool_photo_plane{DevPool::Exact};
    // arvx_carve_votes with ARVX_VOTES_COUNTS: the per-voxel counts, u16 each in flat index order --
    // background, then (from the next 256-byte boundary) inside; read only while votes_ready is set
    DevPool pool_votes{DevPool::Exact};
    bool votes_ready = false;

    // arvx_components: the per-voxel labels (int32, flat index order; -1 where empty); the occupancy
    // plane, the roots' plane and arvx_components_keep's removal plane (bitplane_kernels.h layout);
    // the roots' plane's index (SparseWord); the table -- comp_cap labels, then comp_cap sizes, then
    // comp_cap keep bytes --; and the control block (components_kernels.h, ctl).  The labels and the
    // table are read only while comp_ready is set.
    DevPool pool_comp_label{DevPool::Exact}, pool_comp_planes{DevPool::Exact}, pool_comp_rank{DevPool::Exact},
        pool_comp_table, pool_comp_ctl;
    bool comp_ready = false;
    int comp_conn = 0;
    long long comp_count = 0, comp_cap = 0;

    // arvx_distance / arvx_morph (distance_kernels.h): the field (int32 per voxel, flat index order; read
    // only while dist_ready is set), three bit planes (the occupancy, arvx_morph's intermediate set, the
    // voxels it removes or adds), the column passes' envelope stacks and the change counter
    DevPool pool_dist_field{DevPool::Exact}, pool_dist_planes{DevPool::Exact}, pool_dist_stack{DevPool::Exact},
        pool_dist_ctl;
    bool dist_ready = false;

    // closure (dilation) result: filled voxels, ascending index
    int *d_clo_index = nullptr;
    void *d_clo_rgba = nullptr;  // float4 per filled voxel
    int64_t clo_count = 0;
    bool closure_ready = false;  // the closure list: the fields around are read only while set
    int closure_unseen = 0;
    // the state holds the fills of a closure (its list may have been dropped since): colour calls
    // and a second closure are refused until a carve, an upload or a reset replaces the state (arvx.h)
    bool closure_fills = false;
    int closure_radius = 0;
    std::vector<int> h_clo_index;
    DevPool pool_clo_bits, pool_clo_rank;  // the filled voxels' plane and index (SparseWord)

    // ---- what each call drops --------------------------------------------------------------
    // The rules of arvx.h ("What the context's results belong to") as one table: a row per event,
    // restated by a method of CtxModel (tests/stage_model.py), from arvx.h and not from this table:
    // SetViews set_views, SetImages set_images, Color color, UploadColors upload_colors, HandleUnseen
    // handle_unseen, Closure closure, Carve carve and carve_votes, FastCarve fast_carve, UploadState
    // upload_state, UploadPlanes upload_planes, Reset reset, PhotoCarve photo_carve, ComponentsKeep
    // keep_components, MorphShrink and MorphGrow morph (by its op).  The render column is restated by
    // CtxModel.rendered, from the render's paragraph in arvx.h; ProjectionAssoc and UploadHalo have no
    // restatement there.  tests/test_stage_sequences_gpu.py replays orders of
    // those calls against it.  Every entry point calls drop() once, after its refusals and before its
    // work, so that a refused call leaves the context as it was.  (The closure calls it where its fills
    // go into the state: the colour pass's planes it starts from are those of the state before.)  The
    // mesh products (mc_ready, weld_ready, smooth_*, dec_ready, ref_ready, relax_ready) are not here: each lives until the next
    // call of its own stage (CtxModel holds them as well, and the sequences download them after other calls).  The render of the welded mesh (arvx_render) is: it shows the state the
    // mesh was built from, so whatever replaces that state drops it (and so does the next
    // arvx_mc_mesh_welded).
    enum class Event {
        SetViews, SetImages, Color, UploadColors, ProjectionAssoc, HandleUnseen, Closure,
        Carve, FastCarve, UploadState, UploadPlanes, UploadHalo, Reset, PhotoCarve, ComponentsKeep,
        MorphShrink, MorphGrow
    };
    void drop(Event e) {
        struct Row { uint8_t colours, closure, fills, paint, cstate, state, render, votes, comps; };
        static constexpr Row kRows[] = {
            //                    colour closure closure paint cstate state   render votes  component
            //                    list   list    fills         tiles  changes                labels,
            //                                                                                   distance field
            /* SetViews        */ {1,    1,      0,      0,    0,     0,      0,      1,     0},
            /* SetImages       */ {1,    1,      0,      0,    0,     0,      0,      0,     0},
            /* Color           */ {1,    1,      0,      0,    0,     0,      0,      0,     0},
            /* UploadColors    */ {1,    1,      0,      0,    0,     0,      0,      0,     0},
            /* ProjectionAssoc */ {1,    0,      0,      0,    0,     0,      0,      1,     0},  // (a change of grouping)
            /* HandleUnseen    */ {0,    1,      0,      0,    0,     2,      0,      1,     1},
            /* Closure         */ {0,    1,      0,      0,    1,     1,      0,      1,     1},
            /* Carve           */ {1,    1,      1,      1,    0,     1,      1,      1,     1},
            /* FastCarve       */ {1,    1,      1,      1,    0,     1,      1,      1,     1},
            /* UploadState     */ {1,    1,      1,      2,    1,     1,      1,      1,     1},
            /* UploadPlanes    */ {1,    1,      1,      1,    1,     1,      1,      1,     1},
            /* UploadHalo      */ {1,    1,      1,      0,    1,     1,      1,      1,     1},
            /* Reset           */ {1,    1,      1,      1,    1,     1,      1,      1,     1},
            /* PhotoCarve      */ {1,    1,      1,      1,    0,     1,      1,      1,     1},
            /* ComponentsKeep  */ {1,    1,      1,      1,    0,     1,      1,      1,     1},
            /* MorphShrink     */ {1,    1,      1,      1,    0,     1,      1,      1,     1},  // (ERODE, OPEN)
            /* MorphGrow       */ {1,    1,      1,      1,    1,     1,      1,      1,     1},  // (DILATE, CLOSE)
        };
        // paint 2: the owned planes' paint is replaced; the plane stays where halo planes keep
        // theirs.  state 2: only never-seen voxels become occupied (next_state).  cstate: a call
        // that may occupy or un-see voxels drops what earlier carves settled for whole coarse
        // tiles; carving and handleUnseen leave a tile that is carved and seen / seen as a whole
        // as it is.  Photo-consistency carving only empties voxels and keeps every seen bit: a tile
        // carved and seen as a whole stays empty, one seen as a whole stays seen -- both stay settled.
        // votes: the counts of arvx_carve_votes describe the state that call left under the views and
        // the grouping it ran with; whatever replaces one of them drops the counts.
        // component labels: the labelling of arvx_components describes the occupancy it read; every
        // call that changes the state drops it.  arvx_components_keep drops what photo carving drops,
        // for the same reasons: it only empties voxels and keeps every seen bit.
        // distance field: the field of arvx_distance describes the same occupancy and lives exactly as
        // long as the labelling.  arvx_morph: an erosion or an opening only empties voxels and keeps
        // every seen bit, so it drops what arvx_components_keep drops; a dilation or a closing occupies
        // voxels a later carve has to look at, so it drops the settled coarse tiles as an upload does.
        static_assert(sizeof kRows / sizeof kRows[0] == (size_t)Event::MorphGrow + 1, "a row per event");
        const Row &r = kRows[(int)e];
        if (r.colours) color_ready = color_visible = false;
        if (r.closure) closure_ready = false;
        if (r.fills) closure_fills = false;
        if (r.paint == 1 || (r.paint == 2 && nvox_ext == nvox)) paint_valid = false;
        if (r.cstate) cstate_tiles = 0;
        if (r.state) next_state(r.state == 2);
        if (r.state == 1) {  // (the greedy carve's report describes the carve that left the state)
            flood_bits = flood_launches = flood_tile_rows = 0;
            flood_off_reached = 0;
        }
        if (r.render) render_ready = false;
        if (r.votes) votes_ready = false;
        if (r.comps) comp_ready = dist_ready = false;
    }
    // The state changes: whatever carries the old count as its stamp is stale -- but for
    // handleUnseen (unseen_only) the colour pass's planes of the state before stay usable: its
    // occupancy is their occupancy | their never-seen plane (planes_unseen).
    void next_state(bool unseen_only) {
        if (unseen_only && planes_seq == state_seq) {
            planes_seq = state_seq + 1;
            planes_unseen = true;
        }
        ++state_seq;
    }

    // marching-cubes hand-off: active cells (x, y, z, cube index), reference order
    void *d_mc_cells = nullptr;
    int64_t mc_count = 0;
    bool mc_ready = false;
    // storage behind the d_surf_* / d_clo_* / d_mc_cells views
    DevPool pool_surf_index, pool_surf_rgb, pool_surf_depth, pool_surf_has, pool_clo_index,
        pool_clo_rgba, pool_mc_cells, pool_raw_masks;

    // ---- the meshes: where an array lies in a pool is said once, by the pool's type where it holds one
    // array and by the accessors under it where it holds several; the sizes such a layout depends on are
    // kept from the call that built the mesh (V and T of the welded mesh: weld_verts, weld_tris) ----
    using Plane = unsigned long long;  // a word of a bit plane (bitplane_kernels.h)
    // a face record: three vertex indices, then r, g, b; a position or a vertex colour: three floats
    static constexpr size_t kFaceBytes = 24, kFaceColour = 12, kVertexBytes = 12;
    // arvx_mc_mesh: three positions and a face record per triangle; every mesh's triangle offsets per cell
    DevArray<float> pool_mesh_verts;
    DevArray<unsigned> pool_mesh_rgb;
    DevArray<int> pool_mesh_off;
    int64_t mesh_tris = 0;  // triangles of the last arvx_mc_mesh
    // arvx_mc_mesh_welded: the occupancy plane and the vertex plane (weld_words words each), the vertex
    // plane's ranks and list, and the welded mesh (positions, vertex colours, face records)
    DevArray<Plane> pool_weld_planes;
    DevArray<SparseWord> pool_weld_rank;
    DevArray<int> pool_weld_index;
    DevArray<float> pool_weld_verts, pool_weld_rgb;
    DevArray<unsigned> pool_weld_faces;
    size_t weld_words = 0;
    int64_t weld_verts = 0, weld_tris = 0;
    bool weld_ready = false;
    Plane *weld_occ() const { return pool_weld_planes.data(); }
    Plane *weld_vtx() const { return weld_occ() + weld_words; }
    // arvx_mc_mesh_smooth: the welded mesh's CSRs, built once per welded mesh -- V masks, then counts and
    // offsets (V + 1 each); neighbour list; incidence list --, two position buffers, cross products, normals
    DevArray<int> pool_smooth_csr;
    DevArray<unsigned> pool_smooth_nbr, pool_smooth_inc;
    DevArray<float> pool_smooth_verts, pool_smooth_cross, pool_smooth_normals;
    bool smooth_csr_ready = false, smooth_ready = false;
    int smooth_q = 0;  // the smoothed positions are smooth_xyz(smooth_q)
    size_t smooth_csr_bytes() const { return (size_t)(5 * weld_verts + 4) * sizeof(int); }
    unsigned *smooth_masks() const { return (unsigned *)pool_smooth_csr.data(); }
    int *smooth_icount() const { return pool_smooth_csr.data() + weld_verts; }
    int *smooth_ncount() const { return smooth_icount() + weld_verts + 1; }
    int *smooth_noff() const { return smooth_ncount() + weld_verts + 1; }
    int *smooth_ioff() const { return smooth_noff() + weld_verts + 1; }
    float *smooth_xyz(int q) const {  // 0: the welded mesh's own positions, 1 / 2: a buffer
        return q == 0 ? pool_weld_verts.data() : pool_smooth_verts.data() + (q - 1) * 3 * weld_verts;
    }
    // arvx_mesh_relax / arvx_mesh_relax_triangles (mesh_relax_kernels.h): the CSRs of one mesh of V vertices
    // and T faces -- two counters of listed rows (and two ints of padding), then V + 1 ints each of neighbour
    // counts (the degrees once the rows are finished), incidence counts, neighbour offsets, incidence offsets;
    // the neighbour list (6 T slots) and the incidence list (3 T); the listed rows (neighbour rows, then
    // incidence rows) --, two position buffers, cross products, normals.  V, T: what the layout was made for.
    struct Relax {
        DevArray<int> csr, rows;
        DevArray<unsigned> nbr, inc;
        DevArray<float> verts, cross, normals;
        int64_t V = 0, T = 0;
        size_t csr_bytes() const { return (size_t)(4 * (V + 1) + 4) * sizeof(int); }
        int *n_rows() const { return csr.data(); }  // [0] neighbour rows listed, [1] incidence rows
        int *degree() const { return csr.data() + 4; }
        int *icount() const { return degree() + V + 1; }
        int *noff() const { return icount() + V + 1; }
        int *ioff() const { return noff() + V + 1; }
        long long ncap() const { return 6 * T; }
        long long icap() const { return 3 * T; }
        // (a listed row has more than kRelaxLaneRow = 48 slots)
        int nrows_cap() const { return (int)(ncap() / 49 + 1); }
        int irows_cap() const { return (int)(icap() / 49 + 1); }
        float *xyz(int q) const { return verts.data() + (q - 1) * 3 * V; }  // q = 1, 2: a buffer
    };
    // relax: the context's product, "the relaxed mesh" -- positions (those of its base where relax_q == 0,
    // else relax.xyz(relax_q)), normals, degrees; read only while relax_ready is set -- and the CSRs of the
    // mesh whose faces relax_csr_base names (ARVX_MESH_WELDED for the welded faces, _DECIMATED, _REFINED),
    // current while relax_csr_ready is set.  relax_tri: a caller's mesh, nothing kept between calls.
    // relax_ended(source) is called where a mesh stage replaces or drops the arrays of `source`.
    Relax relax, relax_tri;
    DevArray<float> pool_rtri_verts;
    DevArray<unsigned> pool_rtri_faces;
    bool relax_ready = false, relax_csr_ready = false;
    int relax_base = 0, relax_csr_base = 0, relax_q = 0;
    void relax_ended(int source) {
        constexpr int kSmoothed = 1, kRelaxed = 5;  // (ARVX_MESH_SMOOTHED, ARVX_MESH_RELAXED: arvx.h)
        if (relax_ready && relax_base == source) {
            relax_ready = false;
            mesh_color_ended(kRelaxed);
        }
        // (the smoothed mesh has the welded faces: its end alone leaves their CSRs)
        if (source != kSmoothed && relax_csr_base == source) relax_csr_ready = false;
    }
    // arvx_mc_mesh_decimate: the cluster plane behind its dec_words ranks, the cluster list, the decimated
    // mesh, the welded vertices' map, the welded faces' flags and offsets (T each), the slot table
    DevArray<SparseWord> pool_dec_planes;
    DevArray<int> pool_dec_index, pool_dec_members, pool_dec_map, pool_dec_flags;
    DevArray<float> pool_dec_verts, pool_dec_rgb;
    DevArray<unsigned> pool_dec_faces, pool_dec_slots;
    size_t dec_words = 0;
    int64_t dec_verts = 0, dec_tris = 0;
    bool dec_ready = false;
    SparseWord *dec_rank() const { return pool_dec_planes.data(); }
    inline Plane *dec_bits() const;  // (arvx_capi.hip: it takes the size of a SparseWord)
    int *dec_flags() const { return pool_dec_flags.data(); }
    int *dec_off() const { return dec_flags() + weld_tris; }
    // arvx_mc_mesh_refined: the occupancy plane (ref_words words) and the edge plane, its ranks and list (the
    // keys), the refined mesh; per vertex kRefEdgeInts ints of edge, then -- ref_cap entries in -- the cuts
    DevArray<Plane> pool_ref_planes;
    DevArray<SparseWord> pool_ref_rank;
    DevArray<int> pool_ref_index, pool_ref_edges;
    DevArray<float> pool_ref_verts, pool_ref_rgb;
    DevArray<unsigned> pool_ref_faces;
    static constexpr int kRefEdgeInts = 4;
    size_t ref_words = 0;
    int64_t ref_verts = 0, ref_tris = 0, ref_cap = 0;
    bool ref_ready = false;
    Plane *ref_occ() const { return pool_ref_planes.data(); }
    Plane *ref_edge_plane() const { return ref_occ() + ref_words; }
    int *ref_edges() const { return pool_ref_edges.data(); }
    int *ref_cut() const { return ref_edges() + kRefEdgeInts * ref_cap; }

    // arvx_render: the W x H keys, the images (id | depth | bgr), the large-footprint list behind
    // its header (render_kernels.h), all sized at first use and kept.  Count words: kRenderNeed, then
    // the three agreement counts.  The first is copied to render_need at a render call's synchronisation
    // (download, agreement) and sizes the next renders' lists from there; the word itself is never
    // read while a kernel may be writing it.  A caller's background goes through a
    // page-locked staging buffer: the copy out of it is not waited for, so the event after it is
    // waited for before the buffer is written again.
    DevPool pool_render_keys{DevPool::Exact}, pool_render_img{DevPool::Exact},
        pool_render_large{DevPool::Exact};
    int render_W = 0, render_H = 0;
    bool render_ready = false;
    long long render_need = 0;
    uint8_t *h_render_bg = nullptr;
    size_t render_bg_cap = 0;
    hipEvent_t render_bg_done = nullptr;
    // arvx_render_mesh / arvx_render_triangles (render_mesh_kernels.h): a triangle render is the current
    // render -- the keys, the images and render_ready above -- with render_tris set.  Its own: the
    // projected vertices (16 bytes each), the list of large pixel boxes behind its header with the class
    // counts, sized from kRenderMeshNeed as the voxel render's list is from kRenderNeed (or by
    // arvx_selftest_render_mesh_list: render_mesh_list_cap >= 0), and a caller's mesh (positions, colours,
    // face records).
    DevPool pool_render_proj, pool_render_tris{DevPool::Exact};
    DevArray<float> pool_tri_verts, pool_tri_rgb;
    DevArray<unsigned> pool_tri_faces;
    bool render_tris = false;
    long long render_mesh_need = 0, render_mesh_list_cap = -1;
    // arvx_ctx_set_render_near (render_mesh_clip_kernels.h): the plane of the next triangle render (0:
    // none), and where the current one's four clip counts lie in pool_render_tris, behind its list (0:
    // it was made without a plane and has none).
    float render_near = 0.f;
    size_t render_clip_at = 0;
    // arvx_mesh_color (mesh_color_kernels.h): the product -- per vertex r, g, b and the number of views
    // that see it, the V x H x W depth keys, tagged with its source (read only while mesh_color_ready is
    // set) -- and its workspace: the projected vertices of one batch of views, the list of large pixel
    // boxes behind its header (sized from kMeshColorNeed, or by arvx_selftest_render_mesh_list), the
    // depth image a download converts a view's keys into.  None of them is the render's: a call leaves
    // the current render as it is.  mesh_color_ended(source) is called where a mesh stage replaces or
    // drops the arrays of `source`.
    DevArray<float> pool_mcol_rgb, pool_mcol_depth;
    DevArray<int> pool_mcol_views;
    DevPool pool_mcol_keys{DevPool::Exact}, pool_mcol_proj, pool_mcol_large{DevPool::Exact};
    bool mesh_color_ready = false;
    int mesh_color_source = 0, mesh_color_V = 0, mesh_color_W = 0, mesh_color_H = 0;
    int64_t mesh_color_verts = 0, mesh_color_coloured = 0;
    long long mesh_color_need = 0, mesh_color_batch = 0;  // (batch: arvx_selftest_mesh_color_batch; 0: the bound)
    // arvx_mesh_texture (mesh_texture_kernels.h): the product -- the atlas and the view of every face,
    // tagged with its source, its resolution and its layout (read only while mesh_texture_ready is set)
    // -- and the call's workspace: depth keys of its own (arvx_mesh_color's product keeps its keys), the
    // vertices' visibility words, the count of textured faces.  The projected vertices and the list of
    // large pixel boxes are the mesh colours' workspace above.  It ends where the mesh colours' product
    // of the same source would.
    DevArray<uint8_t> pool_mtex_atlas;
    DevArray<int> pool_mtex_view;
    DevPool pool_mtex_keys{DevPool::Exact}, pool_mtex_bits, pool_mtex_count{DevPool::Exact};
    bool mesh_texture_ready = false;
    int mesh_texture_source = 0, mesh_texture_R = 0, mesh_texture_AW = 0, mesh_texture_AH = 0;
    int64_t mesh_texture_faces = 0, mesh_texture_textured = 0;
    void mesh_color_ended(int source) {
        if (mesh_color_source == source) mesh_color_ready = false;
        if (mesh_texture_source == source) mesh_texture_ready = false;
    }

    // (the device buffers are freed by their DevPool members, after this)
    ~Ctx() {
        if (render_bg_done) (void)hipEventDestroy(render_bg_done);
        if (h_render_bg) (void)hipHostFree(h_render_bg);
        if (h_fault) (void)hipHostFree(h_fault);
    }
    void free_mc() {
        d_mc_cells = nullptr;
        mc_count = 0;
        mc_ready = false;
    }
    void cells_built(long long n) {  // the cell list a call leaves (no buffer where it is empty)
        if (n == 0) d_mc_cells = nullptr;
        mc_count = n;
        mc_ready = true;
    }
    void free_views() {
        pool_M.release();
        pool_campos.release();
        pool_bg.release();
        pool_sat.release();
        pool_rect.release();
        pool_pix.release();
        rect_invalidate();
        views_ready = false;
        cameras_ready = false;
    }
};

}  // namespace arvx

struct arvx_ctx : arvx::Ctx {};
