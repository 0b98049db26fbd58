/*
 * arvx.h -- C-ABI of the MI355X (gfx950) voxel-carving library, libarvx.so.
 *
 * This is the drop-in boundary for ONE path of alxfox/AR_Voxel_Project: the
 * dense silhouette carve, the greedy carve and the per-voxel colour vote,
 * i.e. the bodies of
 *     carve(...)                    reference src/VoxelCarving.h:19
 *     fastCarve(...)                reference src/VoxelCarving.h:31
 *     reconstructClosestColor(...)  reference src/ColorReconstruction.h:131
 *     reconstructAvgColor(...)      reference src/ColorReconstruction.h:142
 *     Model::handleUnseen()         reference src/Model.cpp:36-47
 * The reference's third-party pre-processing (ChArUco pose estimation,
 * cv::undistort, cv::imread) stays on the caller's side: the boundary takes
 * the world->camera matrices and the already undistorted u8 images that the
 * reference feeds its voxel loops (src/VoxelCarving.cpp:25-36).
 *
 * Plain C types only.  Every call returns ARVX_OK or an error code and never
 * throws; arvx_last_error() gives the text.  A context owns one voxel grid (or
 * one Z slab of a grid) on one GPU; calls on one context are not thread safe.
 *
 * State plane: one byte per voxel, index x + X*(y + Y*z) (Model::flatten,
 * reference src/Model.h:104-106), bit0 = occupied (voxels[i].w != 0),
 * bit1 = seen (seen[i]).  That is the EXCHANGE form of arvx_state_upload / _download; on the
 * device the state lives as 2 bits per voxel (or use the bit planes of
 * arvx_state_upload_planes / _download_planes, 8x smaller, which is what the C++ layer does).
 *
 * Streams: every call enqueues on the context's stream (arvx_ctx_set_stream) and calls on one
 * context must not overlap -- with ONE exception: the occupancy hand-off (arvx_pack_occupancy
 * [_global], arvx_occupancy_compress, _expand[_striped]) may run on the exchange stream
 * (arvx_ctx_set_exchange_stream) while arvx_set_views_device / arvx_carve of the NEXT job run
 * on the main stream; those calls share no work buffer with the main stream.
 */
#ifndef ARVX_H
#define ARVX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARVX_VERSION 100

enum {
    ARVX_OK = 0,
    ARVX_ERR_INVALID = 1, /* bad argument (null pointer, size, range) */
    ARVX_ERR_HIP = 2,     /* a HIP runtime call failed */
    ARVX_ERR_STATE = 3,   /* call order (e.g. carve before set_views) */
    ARVX_ERR_NOMEM = 4
};

#define ARVX_OCC 1u
#define ARVX_SEEN 2u

/* flags of arvx_carve / arvx_carve_views */
#define ARVX_CARVE_NO_CULL 1u /* evaluate every voxel in every view (ablation) */
#define ARVX_CARVE_STATS 2u   /* fill the counters read by arvx_get_stats */
#define ARVX_CARVE_FUSED 8u   /* one kernel for rectangle tests and per-voxel work (A/B) */
#define ARVX_CARVE_STREAM 16u    /* a fresh model: the one-launch streaming carve.  It loses to the
                                    three-launch chain and is compiled only into
                                    -DARVX_EXPERIMENTS builds (libarvx_experiments.so, A/B and
                                    tests); the shipped library answers ARVX_ERR_INVALID */
#define ARVX_CARVE_NO_STREAM 32u /* never the streaming carve */
#define ARVX_CARVE_FILTER 64u    /* project through an fp32 filter first, exact fall-back for voxels within
                                    the filter's error of a rounding tie: the same model bit for bit, but
                                    1.16-1.23x SLOWER than the exact kernel (EXPERIMENTS.md round 5) --
                                    compiled only into -DARVX_EXPERIMENTS builds like ARVX_CARVE_STREAM */
/* Path flags: the split carve chooses two of its kernels by the number of voxels.
 * These take the large grids' choice on a grid of any size, so that small test scenes run the
 * kernels that carve 512^3 and 1024^3.  The model is the same bit for bit under every combination.
 * They are ignored where the split carve does not run or the choice does not exist: under
 * ARVX_CARVE_NO_CULL, ARVX_CARVE_FUSED and ARVX_CARVE_STATS, and with more than 256 views. */
#define ARVX_CARVE_DENSE_CLASSIFY 128u /* the sub-tile classification of grids of 2^26 voxels and more:
                                          a workgroup per listed coarse tile (or quarter), lanes =
                                          (sub-tile, view) pairs */
#define ARVX_CARVE_WHOLE_ITEMS 256u    /* the exact kernel of grids above 2^26 voxels: an item is never
                                          shared between waves */

/* colour modes: reference -color=1 / -color=2 (src/main.cpp:276-288) */
#define ARVX_COLOR_CLOSEST 0
#define ARVX_COLOR_AVERAGE 1

typedef struct arvx_ctx arvx_ctx;

typedef struct arvx_stats {
    uint64_t subtiles;        /* 16x8x8 sub-tiles visited */
    uint64_t subtiles_carved; /* decided "all carved" by one view's rectangle test */
    uint64_t subtile_views_mixed; /* (sub-tile, view) pairs evaluated per voxel */
    uint64_t subtile_views_total; /* (sub-tile, view) pairs classified */
    uint64_t surface_voxels;  /* colour pass: occupied non-inner voxels */
    uint64_t reserved[3];
    uint64_t host_total_fallbacks; /* list totals the host had to fetch from the device because the
                                      page-locked word did not show the kernel's store at the
                                      synchronisation (colour pass, closure, cell list, mesh);
                                      expected 0, counted over the context's life */
} arvx_stats;

int arvx_version(void);
const char *arvx_last_error(void);
int arvx_device_count(int *count);
/* How the four products of a row of M * world are summed -- the cv::gemm call behind
 * `intr * pose * world`, reference src/VoxelCarving.cpp:19, which takes cv::gemm's generic path
 * (GEMMSingleMul<float, double>: fp32 inputs, fp64 products and sums):
 *   ARVX_ASSOC_LEFT   ((p0 + p1) + p2) + p3   four accumulators, `(s0 + s1 + s2 + s3) * alpha`
 *   ARVX_ASSOC_RIGHT  p0 + ((p1 + p2) + p3)   `s0 += s1 + s2 + s3`
 * The two differ by double rounding in about one voxel-view in 1e8.  Which one an OpenCV build
 * uses cannot be checked in an image without OpenCV: the default (LEFT) follows the OpenCV 4.x
 * source as recalled, it is a property of a context that can be changed at run time, and
 * include/arvx/opencv_dropin.hpp settles it with one cv::gemm call at first use (see also
 * tools/pin_with_opencv.py).  arvx_projection_assoc: what new contexts start with. */
#define ARVX_ASSOC_RIGHT 0
#define ARVX_ASSOC_LEFT 1
int arvx_projection_assoc(void);
int arvx_set_projection_assoc(int assoc);

/* ---- context --------------------------------------------------------- */

/* Grid X*Y*Z voxels of edge `voxel_size` on HIP device `device`: the
 * arguments of the reference's Model constructor (src/Model.cpp:9). */
int arvx_ctx_create(arvx_ctx **out, int device, int X, int Y, int Z,
                    float voxel_size);
/* Same grid, but this context holds only planes z_begin <= z < z_end
 * (one Z slab of a multi-GPU split). State buffers cover the slab only. */
int arvx_ctx_create_slab(arvx_ctx **out, int device, int X, int Y, int Z,
                         float voxel_size, int z_begin, int z_end);
/* The same with `halo` planes kept (and recomputed by the carve: carving is a pure function of
 * the voxel position) on each side that lies inside the grid; arvx_ctx_create_slab keeps 1.
 * The stages after the carve look further: a voxel is on the surface by its six neighbours
 * (colour pass: 1 plane), the closure's box has radius r = (kernel_size - 1) / 2 and averages
 * its neighbours' COLOURS (r + 1 planes), and the mesh of a slab's cells needs the colours and
 * fills of plane z_begin - 1 (2 planes with colours, r + 2 after a closure: 3 for the
 * reference's kernel size 3).  With enough halo every slab computes its part of
 * carve -> colour -> handleUnseen -> closure -> mesh without any exchange, and the parts put
 * together are the whole-grid result (ar_voxel_project_amd/sharding.py: merge_closure,
 * merge_mesh; tests/test_sharded_stages_gpu.py).  A call that lacks halo planes says so. */
int arvx_ctx_create_slab_halo(arvx_ctx **out, int device, int X, int Y, int Z,
                              float voxel_size, int z_begin, int z_end, int halo);
/* Same grid, striped over `world` GPUs for load balance: with the planes cut
 * into groups of 8, this context holds groups rank, rank+world, rank+2*world, ...
 * back to back (Z must be a multiple of 8).  Carve, state up/download and
 * arvx_pack_occupancy_global work on striped contexts; the colour pass and
 * arvx_fast_carve need neighbouring planes and take contiguous slabs only. */
int arvx_ctx_create_striped(arvx_ctx **out, int device, int X, int Y, int Z,
                            float voxel_size, int world, int rank);
/* (The HIP stream a destroyed context owned is kept in a per-device pool and handed to the next
 * context: creating and destroying a stream costs milliseconds on this stack.  A caller that
 * resets the device (hipDeviceReset) between contexts must not have any context alive across
 * the reset -- the pooled streams die with the device and the library does not notice.) */
int arvx_ctx_destroy(arvx_ctx *ctx);
/* Launch on a caller-owned hipStream_t (borrowed); NULL = context's own. */
int arvx_ctx_set_stream(arvx_ctx *ctx, void *hip_stream);
/* A stream of its own for the occupancy hand-off (arvx_pack_occupancy[_global],
 * arvx_occupancy_compress / _expand[_striped]): a multi-GPU job runs the exchange of job k --
 * pack, compress, the collective, expand -- beside the carve of job k + 1.  The caller orders
 * the two streams with events: the pack reads the state the carve wrote (it must wait for the
 * carve, and the next carve for the pack).  NULL: back on the context's stream. */
int arvx_ctx_set_exchange_stream(arvx_ctx *ctx, void *hip_stream);
int arvx_ctx_synchronize(arvx_ctx *ctx);
/* The row-sum grouping of THIS context (see arvx_projection_assoc); takes effect with the next
 * carve / colour pass. */
int arvx_ctx_set_projection_assoc(arvx_ctx *ctx, int assoc);
int arvx_ctx_projection_assoc(const arvx_ctx *ctx, int *assoc);
/* Voxels held by this context (slab). */
int arvx_ctx_voxels(const arvx_ctx *ctx, int64_t *count);

/* ---- views ------------------------------------------------------------ */

/* M = K(3x3) * Rt(3x4), float, each element a0*b0 + a1*b1 + a2*b2 evaluated
 * left to right without FMA: what `intr * pose` yields through cv::gemm in
 * the reference (src/VoxelCarving.cpp:19).  Host helper; callers that have
 * OpenCV should pass OpenCV's own product instead. */
int arvx_compose_projection(const float K[9], const float Rt[12], float M[12]);

/* The V camera views.
 *   M      V*12 floats, row-major 3x4, M = intr * pose[0:3,:]  (world->pixel)
 *   campos V*3 floats, the translation column of the world->camera matrix
 *          (what the reference's colour pass calls `cameras[i]`,
 *          src/ColorReconstruction.h:21); may be NULL if arvx_color is unused
 *   masks  V host pointers; each an undistorted mask, H rows of `stride`
 *          bytes, C interleaved u8 channels (reference: 3, BGR); a pixel is
 *          background iff all C bytes are 0 (src/VoxelCarving.cpp:49-50)
 * Copies everything to the device; the host buffers may be freed on return.
 * masks == NULL: cameras only (M, campos, W, H) for a colour pass that follows -- arvx_color
 * never looks at the masks (the reference undistorts them there and drops them,
 * src/ColorReconstruction.h:25-28); arvx_carve / arvx_fast_carve then need a full
 * arvx_set_views first. */
int arvx_set_views(arvx_ctx *ctx, int V, const float *M, const float *campos,
                   const uint8_t *const *masks, int W, int H, int C,
                   size_t stride);
/* Same, masks already in device memory: V images back to back, tightly
 * packed (stride = W*C).  No host synchronisation. */
int arvx_set_views_device(arvx_ctx *ctx, int V, const float *M,
                          const float *campos, const void *dev_masks, int W,
                          int H, int C);
/* cv::undistort(src, dst, cameraMatrix, distCoeffs) for V images of one size on the device --
 * what the reference does to every mask and image before its voxel loops
 * (src/VoxelCarving.cpp:35-36; src/ColorReconstruction.h:22-27): map in double precision,
 * 5-bit fixed-point bilinear weights, constant-0 border (csrc/undistort_kernels.h; restated
 * from OpenCV 4.x, parity UNPINNED -- no OpenCV in this image).  K: cameraMatrix row-major;
 * dist: k1 k2 p1 p2 [k3 [k4 k5 k6]] (ndist = 4, 5 or 8).  src/dst: V host images, H rows of
 * `stride` bytes, C interleaved u8 channels; dst may equal src.  The _device form takes and
 * leaves tightly packed images in device memory (dst != src), ready for
 * arvx_set_views_device. */
int arvx_undistort(arvx_ctx *ctx, int V, const uint8_t *const *src, int W, int H, int C,
                   size_t stride, const double K[9], const double *dist, int ndist,
                   uint8_t *const *dst);
int arvx_undistort_device(arvx_ctx *ctx, int V, const void *dev_src, int W, int H, int C,
                          const double K[9], const double *dist, int ndist, void *dev_dst);
/* Undistorted colour images for arvx_color: V host pointers, BGR u8, H rows
 * of `stride` bytes, same W/H as the masks. */
int arvx_set_images(arvx_ctx *ctx, const uint8_t *const *images, size_t stride);

/* ---- silhouettes from the photographs (extension beyond the reference's -c=4) -------------------
 * arvx_segment_views turns V BGR photographs into the context's views -- the background bit planes
 * and summed-area tables arvx_set_views would derive from the masks defined below -- and leaves the
 * photographs resident as arvx_set_images would.  Everything is integer arithmetic, so a restatement
 * (tests/segment.py) is matched bit for bit.
 *
 * Definition.  Per view, on W x H pixels, flat pixel index i = y * W + x, the steps in this order:
 *  1. Rule: the raw foreground.
 *     ARVX_SEGMENT_RANGE  a pixel is background iff lo[c] <= p[c] <= hi[c] in all three channels (lo, hi
 *                         in B, G, R order); foreground is the complement: the reference's
 *                         ~inRange(lo, hi), src/Segmentation.h:10-11, whose constants are lo = 120,
 *                         hi = 255 in every channel.
 *     ARVX_SEGMENT_PLATE  a pixel is foreground iff max over c of |p[c] - plate[c]| > threshold, against
 *                         a background plate of the same size and stride: plate_count = 1 plate for all
 *                         views, or V, one per view.  threshold in [0, 255].
 *  2. Opening by a square of side 2 * open_radius + 1: erosion, then dilation.  The erosion treats
 *     pixels outside the image as foreground, the dilation as background.  Radius 0 skips the step; a
 *     radius of max(W, H) and more is legal.
 *  3. Closing by a square of side 2 * close_radius + 1: dilation, then erosion, borders as in step 2.
 *  4. Specks.  The foreground's components under 8-connectivity; a component's label is its least
 *     flat pixel index.  min_area > 0: components of fewer than min_area pixels become background.
 *     ARVX_SEGMENT_LARGEST: all but the largest surviving component become background, ties going
 *     to the smaller label.
 *  5. Holes, on the result of step 4.  The background's components under 4-connectivity (the pair
 *     that is consistent with 8 for the foreground: a pocket that reaches the outside only through a
 *     diagonal gap is a hole); a component with no pixel on the image border and an area of at most
 *     max_hole becomes foreground.  max_hole < 0: any area; max_hole == 0: the step is off.
 * The final mask gives background bit i = 1 iff pixel i is background, in the layout arvx_set_views
 * derives: bit index y * W + x, rows not word-aligned, padding bits and the word behind the pixels 0.
 *
 * Contract of both forms: in every later observation the context is as if arvx_set_views (with the
 * final masks, one channel, 255 = foreground) and then arvx_set_images (with these photographs) had
 * been called -- what those two calls drop is dropped, matrices that did not change keep the cached
 * rectangles, and the tables are written whole.  The host form takes V host pointers (H rows of
 * `stride` bytes each, plates too) and returns when the host buffers may go; the _device form takes
 * tightly packed device images (and plates) and does not synchronise with the host.
 * Refusals (ARVX_ERR_INVALID, nothing changed): null pointers (plates only under PLATE), V, W, H
 * outside arvx_set_views' ranges, an unknown rule, lo[c] > hi[c], a threshold outside [0, 255] (under
 * either rule), a plate_count that is neither 1 nor V under PLATE, negative radii, a negative
 * min_area, unknown flag bits, a stride below 3 * W.
 *
 * arvx_segment_download: the final mask of a view, W x H bytes, 255 foreground, 0 background.
 * arvx_segment_counts: out[0..3] foreground pixels after steps 1, 3, 4 and 5; out[4], out[5] the speck
 * components and pixels step 4 removed; out[6], out[7] the hole components and pixels step 5 filled.
 * Both answer ARVX_ERR_STATE before the first call and once a later arvx_set_views[_device] has
 * replaced the views; a view outside [0, V) or a null pointer: ARVX_ERR_INVALID.
 *
 * Memory: two work planes of a bit per pixel (rows padded to 64), and for steps 4 and 5 a label and
 * an area, int32 each, per pixel of one batch of views -- the views go through in batches of at most
 * 2^27 pixels (1 GiB), at least one view.  arvx_selftest_segment_batch: views per batch from the next
 * call on (0: that bound; larger values are clipped to it); batches never change the result. */
#define ARVX_SEGMENT_RANGE 0
#define ARVX_SEGMENT_PLATE 1
#define ARVX_SEGMENT_LARGEST 1u /* flags of arvx_segment_params */
typedef struct arvx_segment_params {
    int32_t rule;         /* ARVX_SEGMENT_RANGE or ARVX_SEGMENT_PLATE */
    uint8_t lo[3], hi[3]; /* RANGE: the background's range, B, G, R */
    uint8_t reserved[2];
    int32_t threshold;    /* PLATE */
    int32_t open_radius, close_radius;
    uint32_t flags;
    int64_t min_area, max_hole;
} arvx_segment_params;
int arvx_segment_views(arvx_ctx *ctx, int V, const float *M, const float *campos,
                       const uint8_t *const *images, int W, int H, size_t stride,
                       const uint8_t *const *plates, int plate_count, const arvx_segment_params *params);
int arvx_segment_views_device(arvx_ctx *ctx, int V, const float *M, const float *campos,
                              const void *dev_images, int W, int H, const void *dev_plates,
                              int plate_count, const arvx_segment_params *params);
int arvx_segment_download(arvx_ctx *ctx, int view, uint8_t *mask);
int arvx_segment_counts(arvx_ctx *ctx, int view, int64_t out[8]);
int arvx_selftest_segment_batch(arvx_ctx *ctx, int views_per_batch);

/* ---- state ------------------------------------------------------------ */

/* All voxels occupied, none seen: the state a fresh Model has. */
int arvx_state_reset(arvx_ctx *ctx);
int arvx_state_upload(arvx_ctx *ctx, const uint8_t *state);
int arvx_state_download(arvx_ctx *ctx, uint8_t *state);
/* The same state as two bit planes, 8x smaller than the byte plane each: occupied and seen,
 * rows padded to whole 32-bit words -- word (z, y, k) holds voxels x = 32 k .. 32 k + 31 of row
 * (y, z), bit x % 32; ceil(X / 32) * Y * (owned planes) words per plane (for X % 32 == 0 this
 * is the flat packing of arvx_pack_occupancy).  This is the form the device keeps (2 bits per
 * voxel) and the host-side arvx::Model mirrors, so a carve result crosses PCIe as N / 4 bytes. */
int arvx_state_upload_planes(arvx_ctx *ctx, const uint32_t *occ, const uint32_t *seen);
int arvx_state_download_planes(arvx_ctx *ctx, uint32_t *occ, uint32_t *seen);
/* The same two planes of the owned voxels as compressed PACKETS -- what a carved model mostly is:
 * long runs of empty space (all-zero words), solid interior (all-one words) and a thin shell of
 * mixed words.  The planes are read as 64-bit words in flat order (bit i % 64 of word i / 64 =
 * voxel i = x + X * (y + Y * z), z relative to the first owned plane; needs X % 32 == 0 and
 * X * Y % 64 == 0), and a packet is the layout of arvx_occupancy_compress (below):
 *   [0] number of mixed words   [1, 1+nb) bitmap of the all-one words   [1+nb, 1+2nb) bitmap of the
 *   mixed words   [1+2nb, H) per group of 64 words the number of mixed words before it (u32)
 *   [H, H+need) the mixed words in order           nb = ceil(n / 64), H = 1 + 2 nb + ceil(nb / 2)
 * so a reader finds word i without expanding anything: all-one / mixed by its bit in group i / 64,
 * a mixed word at H + offset[group] + popcount(mixed bits below it).  1024^3 sphere: 24 MB instead of
 * 268 MB across PCIe.  arvx_state_packet_geometry: n (words64) and H (header_words).
 * arvx_state_download_packets: each host buffer has room for H + cap words; *need = the packet's
 * number of mixed words.  A packet that needed more than its cap is copied up to the cap only: call
 * again with larger buffers -- the device keeps both packets while the state is unchanged, so the
 * second call only copies.  Host side: include/arvx/model.hpp answers get / isInner / visited
 * straight from the packets. */
int arvx_state_packet_geometry(arvx_ctx *ctx, int64_t *words64, int64_t *header_words);
int arvx_state_download_packets(arvx_ctx *ctx, uint64_t *occ_packet, int64_t occ_cap, uint64_t *seen_packet,
                                int64_t seen_cap, int64_t *occ_need, int64_t *seen_need);
/* Model::handleUnseen() on the device state (reference src/Model.cpp:36-47): every voxel that
 * no view saw becomes occupied (the reference paints it UNSEEN_COLOR, w = 1); seen bits stay. */
int arvx_handle_unseen(arvx_ctx *ctx);
/* Page-lock caller memory (hipHostRegister) so that uploads / downloads into it run at full
 * PCIe rate instead of through the runtime's staging buffers; optional.  Plain wrappers, so
 * that host code needs no HIP headers. */
int arvx_host_register(void *ptr, size_t bytes);
int arvx_host_unregister(void *ptr);
/* A device-side SNAPSHOT of the owned part of the state as one byte per voxel, for consumers
 * that read it in place.  The context keeps the state as 2-bit records; this call converts
 * them into a buffer the context owns (enqueued on the context's stream: synchronise or use
 * that stream before reading).  The pointer is valid until the context is destroyed, its
 * CONTENT only until the next call that changes the state (carve, fast carve, handleUnseen,
 * closure, uploads, reset): query again afterwards.  Writes through it are not seen by the
 * library -- use arvx_state_upload[_planes]. */
int arvx_state_device_ptr(arvx_ctx *ctx, void **ptr, size_t *bytes);
/* Slab contexts keep one halo plane on each side that lies inside the grid
 * (z_begin-1 and z_end), because the colour pass needs the six neighbours of
 * every voxel (reference Model::isInner, src/Model.h:126-132).  arvx_carve
 * recomputes the halo planes itself (carving is a pure function of the voxel
 * position), arvx_state_reset makes them fresh, arvx_state_upload leaves them
 * untouched.  A caller that uploads a pre-carved model into a slab passes the
 * neighbouring planes here (X*Y bytes each; NULL = leave as is). */
int arvx_state_upload_halo(arvx_ctx *ctx, const uint8_t *plane_below,
                           const uint8_t *plane_above);
/* Pack bit0 (occupied) of the slab into 32-bit words, voxel i -> bit i%32 of
 * word i/32, written to device memory dev_words (>= ceil(n/32) words). */
int arvx_pack_occupancy(arvx_ctx *ctx, void *dev_words);
/* Same bits, written at their place in the word plane of the WHOLE grid
 * (ceil(X*Y*Z/32) words at dev_global_words): plane z starts at word z*X*Y/32.
 * Works for contiguous and striped slabs; needs X*Y to be a multiple of 64. */
int arvx_pack_occupancy_global(arvx_ctx *ctx, void *dev_global_words);

/* Compressed form of a slab's packed occupancy for the end-of-carve exchange (SURVEY 8e:
 * over xGMI the exchange, not the carve, sets the pace of a multi-GPU step).  Most 64-bit
 * words of the packed plane are all-zero or all-one: a packet holds the number of mixed
 * words, two bitmaps (all-one, mixed), per 64 words the number of mixed words before them,
 * and the mixed words themselves -- arvx_occupancy_packet_words(n, cap) 64-bit words for a
 * slab of n words with room for cap mixed ones.
 *   arvx_occupancy_compress: device words of ONE slab -> one packet.
 *   arvx_occupancy_expand: the `world` packets of an all-gather, back to back -> the plain
 *   words of every other rank's slab at q * n in dev_full_words (equal slabs; 16-byte
 *   aligned); a packet whose
 *   slab had more than cap mixed words sets *dev_overflow = 1 and is skipped: fall back to
 *   the plain all-gather of the packed words then. */
int64_t arvx_occupancy_packet_words(int64_t n_words64, int64_t cap_words64);
int arvx_occupancy_compress(arvx_ctx *ctx, const void *dev_words, int64_t n_words64,
                            void *dev_packet, int64_t cap_words64);
int arvx_occupancy_expand(arvx_ctx *ctx, const void *dev_packets, int world, int self_rank,
                          int64_t n_words64, int64_t cap_words64, void *dev_full_words,
                          int *dev_overflow);
/* The same for striped slabs (arvx_ctx_create_striped: rank q owns the 8-plane groups q,
 * q + world, ...; a packet holds a rank's planes in its local order, arvx_pack_occupancy):
 * word i of rank q goes to ((i / wpg) * world + q) * wpg + i % wpg of the whole grid's plane,
 * wpg = words_per_group = X*Y*8/64 (must be even).  Every rank's packet is expanded, the
 * caller's own included. */
int arvx_occupancy_expand_striped(arvx_ctx *ctx, const void *dev_packets, int world,
                                  int64_t n_words64, int64_t cap_words64, int64_t words_per_group,
                                  void *dev_full_words, int *dev_overflow);
/* The rank's own packet straight from the state (no arvx_pack_occupancy in between): the
 * context's planes in local order -> dev_packet, the same packet arvx_pack_occupancy +
 * arvx_occupancy_compress produce, in two launches instead of four and one pass over the words
 * less.  dev_full_words (may be null): the whole grid's word plane -- the rank's own words are
 * stored at their place there as well (contiguous and striped slabs), so that the expansion of the
 * gathered packets can leave the caller's out (arvx_occupancy_expand's self_rank /
 * arvx_occupancy_expand_striped_others).  Needs X % 32 == 0 and X*Y % 64 == 0. */
int arvx_occupancy_pack_compress(arvx_ctx *ctx, void *dev_packet, int64_t cap_words64,
                                 void *dev_full_words);
/* arvx_occupancy_expand_striped that leaves rank self_rank's packet out (-1: none). */
int arvx_occupancy_expand_striped_others(arvx_ctx *ctx, const void *dev_packets, int world,
                                         int self_rank, int64_t n_words64, int64_t cap_words64,
                                         int64_t words_per_group, void *dev_full_words,
                                         int *dev_overflow);

/* ---- hot path --------------------------------------------------------- */

/* Dense carve over all views: reference carve(), src/VoxelCarving.cpp:60-72. */
int arvx_carve(arvx_ctx *ctx, unsigned flags);
/* Views first <= i < first+count only; count = 1 is the reference's
 * single-view carve (src/VoxelCarving.cpp:23-58), used for its per-view
 * intermediate meshes (:65-68). */
int arvx_carve_views(arvx_ctx *ctx, int first, int count, unsigned flags);
/* Greedy carve: reference fastCarve(), src/VoxelCarving.cpp:74-167.
 * Needs the whole grid in one context (no slab).  The context keeps the work
 * buffer of the flood fill (about 1.25 bytes per voxel) for later calls. */
int arvx_fast_carve(arvx_ctx *ctx);
/* Colour vote on the occupied surface voxels (reference
 * reconstructClosestColor / reconstructAvgColor). Result stays on the device
 * until arvx_export_model / arvx_surface_download. */
int arvx_color(arvx_ctx *ctx, int mode);
/* Number of coloured voxels of the last arvx_color, then their flat indices
 * and RGB values (3 floats each, integral), ascending index order. */
int arvx_surface_count(arvx_ctx *ctx, int64_t *count);
int arvx_surface_download(arvx_ctx *ctx, int64_t *index, float *rgb);
/* Smallest sample depth of each coloured voxel (same order), as the reference
 * computes it: (float)cv::norm(cameras[i] - world), src/ColorReconstruction.h:59. */
int arvx_surface_depth_download(arvx_ctx *ctx, float *depth);
/* ---- visible colour (extension beyond the reference) ----------------------------------------
 * The reference's colour pass never asks whether a camera sees a voxel.  arvx_color_visible is
 * arvx_color with a visibility test: a voxel votes only with the views in which it is visible,
 * decided by a per-view depth buffer of the carved surface.  Definition, on a whole-grid context,
 * its state, its views M (with campos) and its images.  S = the voxels arvx_color colours
 * (occupied and not inner), ascending flat index.  Every projection below is arvx_color's: fp64
 * products of the fp32 operands, the row sum in the context's grouping
 * (arvx_ctx_set_projection_assoc) rounded to fp32, then IEEE fp32 quotients.
 *  1. Centre.  For voxel s = (x, y, z) and view v, a0, a1, a2 = the rows of M_v * toWord(x, y, z);
 *     its pixel and "inside" test are the colour pass's (round half away of a0/a2, a1/a2).
 *  2. Footprint.  For the eight corners (dx, dy, dz) in {-1, +1}^3 the world point
 *     w0 = ((float)y + 0.5f*dy) * s, w1 = ((float)x + 0.5f*dx) * s, w2 = -(((float)z + 0.5f*dz) * s)
 *     (each operation rounded once in fp32), projected the same way to (c0, c1, c2), with
 *     qu = c0/c2, qv = c1/c2.  s SPLATS in view v iff the centre's a2 > 0, every corner's c2 > 0
 *     and all 16 quotients are finite.  Its footprint is then the pixels (c, r) with 0 <= c < W,
 *     0 <= r < H, round(min qu) <= c <= round(max qu), round(min qv) <= r <= round(max qv)
 *     (round = std::round on the fp32 value); it may be empty.
 *  3. Depth buffer.  Z_v[p] = the minimum of the centre a2 over the voxels of S that splat in v
 *     with p in their footprint; +inf where there are none.  (A minimum of fp32 values: the order
 *     in which voxels arrive cannot change it.)
 *  4. Visibility.  s is visible in v iff its centre is inside image v, a2 > 0 and
 *     a2 <= Z_v[pix] + tol (one fp32 addition).  tol: the caller's tolerance in world units,
 *     >= 0, finite or +inf.
 *  5. Vote.  arvx_color's rule (view order, strict < on the sample depth, the first view wins
 *     ties; average: roundf(sum / n)) over the samples of the views in which s is visible.  A
 *     voxel visible in no view gets exactly what arvx_color gives it.  So the coloured voxels,
 *     their w and arvx_surface_depth_download (the minimum over ALL samples) are arvx_color's;
 *     only RGB values change.  With tol = +inf and every voxel in front of every camera the
 *     result is arvx_color's bit for bit.
 * Same preconditions and refusals as arvx_color; slab and striped contexts: ARVX_ERR_STATE; a mode
 * other than ARVX_COLOR_CLOSEST / ARVX_COLOR_AVERAGE or a NaN or negative tolerance:
 * ARVX_ERR_INVALID.  It fills the colour list arvx_color fills, with the same lifetime, so
 * arvx_surface_*, arvx_export_model, arvx_closure and the meshes take it as they take
 * arvx_color's.  One host synchronisation, as arvx_color.  Device memory: the depth buffers,
 * V * W * H * 4 bytes, allocated at the first call and kept until the context is destroyed. */
int arvx_color_visible(arvx_ctx *ctx, int mode, float tolerance);
/* For each coloured voxel, in arvx_surface_download's order, the number of views it is visible
 * in (0: it took the fallback). */
int arvx_surface_visible_download(arvx_ctx *ctx, int32_t *views);
/* Z_view as H x W floats (row-major).  Both downloads need the colour list of an
 * arvx_color_visible (ARVX_ERR_STATE otherwise, after a plain arvx_color too); a view outside
 * [0, V): ARVX_ERR_INVALID. */
int arvx_view_depth_download(arvx_ctx *ctx, int view, float *depth);
/* ---- photo-consistency carving (extension beyond the reference) -----------------------------
 * Silhouettes leave the visual hull: a concavity no silhouette sees stays solid.  arvx_photo_carve
 * removes the surface voxels that the views which see them see in clearly different colours, and
 * repeats on the surface that uncovers.  Definition, on a whole-grid context, its state, its views
 * M (with campos) and its images; max_std >= 0 (finite or +inf), min_views >= 1, tolerance as
 * arvx_color_visible's (world units), max_iterations >= 1.  Iteration k:
 *  1. S = the voxels arvx_color would colour in the current state (occupied and not inner),
 *     ascending flat index.
 *  2. Z_v = the depth buffers of S: steps 1-3 of arvx_color_visible's definition, unchanged.
 *  3. For each s in S, its samples in the views in which it is visible (step 4 there): the centre
 *     pixel's (r, g, b), as the colour pass reads it.  n = their number; per channel c,
 *     S_c = sum x and Q_c = sum x^2 as exact integers; D = sum_c (n * Q_c - S_c^2) in int64 (exact
 *     for any V below 2^16).
 *  4. s is INCONSISTENT iff n >= min_views and
 *     (double)D > ((double)max_std * (double)max_std) * ((double)n * (double)n), in fp64.  D / n^2
 *     is the sum of the three channels' population variances; with max_std = +inf nothing is.
 *  5. Every inconsistent voxel of S becomes empty at once: its occupied bit is cleared, its seen bit
 *     stays.  The decisions of iteration k read only the state at its start (a Jacobi update): the
 *     result does not depend on the order of threads.
 * The call stops after an iteration that removes nothing (it counts) or after max_iterations; it
 * returns the iterations run and the voxels removed in all (either pointer may be null).
 * Refusals: no views, no campos or no images, a slab or a striped context: ARVX_ERR_STATE; a NaN or
 * negative max_std or tolerance, min_views < 1 or max_iterations < 1: ARVX_ERR_INVALID; a state
 * holding a closure's fills whose list is gone: ARVX_ERR_STATE, as the calls that return colours.
 * The call replaces the state as a carve does (see "What the context's results belong to",
 * arvx_closure).  One host synchronisation per iteration (a second one when the surface list
 * outgrows its buffers: that attempt decides nothing).  Device memory: the depth buffers of
 * arvx_color_visible, a removal plane of one bit per voxel and one bit per surface voxel. */
int arvx_photo_carve(arvx_ctx *ctx, float max_std, int min_views, float tolerance, int max_iterations,
                     int *iterations, int64_t *removed);
/* ---- vote carve (extension beyond the reference) ----------------------------------------------
 * The reference's carve empties a voxel at the first view whose mask pixel is background
 * (src/VoxelCarving.cpp:50-54): exact for perfect silhouettes, and one patch missing from one
 * segmentation drills a tunnel through the model along that camera's rays.  arvx_carve_votes
 * counts the views instead and empties a voxel only above a tolerance.  Definition, on a whole-grid
 * context, its state and its V views with masks:
 *  1. For voxel i = (x, y, z) and view v the pixel is the carve's: M_v * toWord(x, y, z) with the
 *     fp64 products of the fp32 operands, the row sums in the context's grouping
 *     (arvx_ctx_set_projection_assoc) rounded to fp32, IEEE fp32 quotients, std::round.
 *     inside_v(i) iff the pixel lies in the image; miss_v(i) iff inside_v(i) and all C bytes of the
 *     mask pixel are 0.
 *  2. in(i) = sum over v of inside_v(i), bg(i) = sum over v of miss_v(i).
 *  3. occ'(i) = occ(i) && bg(i) <= max_misses; seen'(i) = seen(i) || in(i) >= 1.
 * So arvx_carve_votes(ctx, 0, .) is arvx_carve(ctx, 0) bit for bit, and with max_misses >= V no
 * voxel is emptied and only seen bits are set.  The flags change the work, never the state:
 *   ARVX_VOTES_COUNTS   bg and in are kept on the device, u16 per voxel in flat index order, until
 *                       the next call that replaces the state (carve, fast carve, photo carve,
 *                       arvx_components_keep, handleUnseen, closure, upload, reset), the views or the
 *                       grouping.  Both are
 *                       the full sums over all V views whatever max_misses is: no early exit is
 *                       taken.  arvx_votes_download copies them out (either pointer may be null; it
 *                       synchronises); without such counts it returns ARVX_ERR_STATE.
 *   ARVX_VOTES_NO_CULL  every voxel is projected in every view: no rectangle test decides anything
 *                       and nothing stops early (ablation, and the yardstick of the tests).
 * Refusals: views missing or set with masks == NULL, a slab or a striped context (out of scope of
 * this call for now: the multi-GPU drivers keep the plain carve): ARVX_ERR_STATE; max_misses < 0 or
 * > 65535, more than 65535 views, unknown flag bits: ARVX_ERR_INVALID.  A refused call changes
 * nothing.  The call does not synchronise, like arvx_carve.  It replaces the state as a carve does:
 * it drops what arvx_photo_carve drops (see "What the context's results belong to", arvx_closure)
 * and keeps what earlier carves settled for whole coarse tiles, since it only empties voxels and
 * sets seen bits.  Device memory with ARVX_VOTES_COUNTS: 4 bytes per voxel, kept. */
#define ARVX_VOTES_COUNTS 1u  /* keep the two per-voxel counts for arvx_votes_download */
#define ARVX_VOTES_NO_CULL 2u /* project every voxel in every view (ablation, yardstick) */
int arvx_carve_votes(arvx_ctx *ctx, int max_misses, unsigned flags);
int arvx_votes_download(arvx_ctx *ctx, uint16_t *background, uint16_t *inside);
/* ---- connected components (extension beyond the reference) ------------------------------------
 * Every carve decides a voxel on its own; none asks whether it is attached to anything.  Where the
 * false foreground specks of a few silhouettes intersect, a clump of voxels survives in mid-air
 * (the vote carve, which tolerates misses, keeps more of them), and the reference has no answer:
 * its fastCarve follows connectivity only through empty space.  arvx_components labels the model,
 * arvx_components_keep drops the floaters.  Definition, on a whole-grid context, its current state:
 *  - a voxel is OCCUPIED iff bit0 of the byte arvx_state_download would return for it is set (a
 *    closure's fills included); the paint bit and the seen bit play no part;
 *  - two occupied voxels are ADJACENT under connectivity 6 iff they differ by 1 in exactly one
 *    coordinate, under connectivity 26 iff they differ by at most 1 in every coordinate and are not
 *    the same voxel; out-of-grid counts as empty;
 *  - a COMPONENT is a class of the transitive closure of that adjacency; its LABEL is the least flat
 *    index x + X*(y + Y*z) among its voxels, its SIZE the number of its voxels.
 * Everything is an integer: the result depends on no thread order and is compared bit for bit.
 *   arvx_components            labels; *count = number of components C.  The state is unchanged
 *                              and nothing is dropped.
 *   arvx_components_download   the table: the C labels ascending, and their sizes (either pointer
 *                              may be null).
 *   arvx_components_labels_download  per voxel, flat index order: the label of its component, -1
 *                              where empty.
 *   arvx_components_keep       keeps component c iff size(c) >= min_voxels and (ARVX_COMPONENTS_LARGEST
 *                              not set, or c has the greatest size -- the least label among equals);
 *                              every voxel of the other components becomes empty: occupied bit
 *                              cleared, seen bit kept.  *kept = components left, *removed = voxels
 *                              emptied (either may be null).
 * The labelling of arvx_components lives until any call that replaces the state (carve, vote carve,
 * fast carve, photo carve, arvx_handle_unseen, closure, state uploads, reset, arvx_components_keep);
 * before a labelling and after such a call the two downloads answer ARVX_ERR_STATE.
 * arvx_components_keep labels on its own account and leaves no labelling behind.  It replaces the
 * state as arvx_photo_carve does: it drops what photo carving drops even when it removes nothing
 * (see "What the context's results belong to", arvx_closure), ends a lazy state first, leaves what
 * earlier carves settled for whole coarse tiles valid, since it only empties voxels, and refuses a
 * state holding a closure's fills whose list is gone (ARVX_ERR_STATE).
 * Refusals: a slab or a striped context: ARVX_ERR_STATE; a connectivity other than 6 or 26,
 * min_voxels < 1, unknown flag bits, a null count (a null voxel_label): ARVX_ERR_INVALID.  A refused
 * call changes nothing.  An empty model is no error: 0 components, nothing removed.
 * One host synchronisation per call (the counts); a second one when the table outgrows its room
 * (first 1024 components, then what the last call held): that attempt counts no size and removes
 * nothing, and the call's launches run once more.  The downloads synchronise.
 * Device memory, allocated at first use and kept: 4 bytes per voxel (the labels), three bit planes
 * (occupancy, roots, removal: 3/8 byte per voxel), 16 bytes per 64 voxels (the roots' plane's index)
 * and 12 bytes per component of the table's room.
 * Out of scope: slabs and multi-GPU, connectivity 18, selecting components by an arbitrary list. */
#define ARVX_COMPONENTS_LARGEST 1u /* keep only the component of the greatest size */
int arvx_components(arvx_ctx *ctx, int connectivity, int64_t *count);
int arvx_components_download(arvx_ctx *ctx, int32_t *label, int32_t *size);
int arvx_components_labels_download(arvx_ctx *ctx, int32_t *voxel_label);
int arvx_components_keep(arvx_ctx *ctx, int connectivity, int64_t min_voxels, unsigned flags,
                         int64_t *kept, int64_t *removed);
/* ---- signed distance field and ball morphology (extension beyond the reference) ----------------
 * The stages above decide a voxel by its views or by its connectivity; none decides it by shape.  A
 * fin, a spur or a one-voxel bridge that is still attached survives arvx_components_keep, and the
 * only morphology of the reference is arvx_closure, one box dilation.  The exact Euclidean distance
 * transform answers both: once every voxel knows its squared distance to the nearest voxel of the
 * other kind, erosion, dilation, opening and closing by a ball of any radius are one threshold each.
 * Definition, on a whole-grid context, its current state:
 *  - OCCUPIED is what arvx_components calls occupied (bit0 of the byte arvx_state_download would
 *    return, a closure's fills included); lattice points are integer triples, the grid is
 *    [0,X) x [0,Y) x [0,Z), and |i - j|^2 is the integer dx^2 + dy^2 + dz^2;
 *  - the SIGNED SQUARED DISTANCE d(i), an int32 per voxel in flat index order x + X*(y + Y*z):
 *      i occupied: d(i) = +min |i - j|^2 over the EMPTY sites j: the empty voxels of the grid and,
 *        unless ARVX_DISTANCE_BORDER_OCCUPIED is set, every lattice point outside the grid (the
 *        nearest of those is axis-aligned, so the border alone contributes
 *        min(x+1, X-x, y+1, Y-y, z+1, Z-z)^2); d(i) >= 1;
 *      i empty: d(i) = -min |i - j|^2 over the occupied voxels j of the grid (nothing outside the
 *        grid is ever occupied for this purpose); d(i) <= -1;
 *      where the minimum runs over nothing (a full grid under BORDER_OCCUPIED, an empty grid):
 *        d(i) = +ARVX_DISTANCE_INF resp. -ARVX_DISTANCE_INF;
 *  - the BALL of squared radius R (an integer, 0 <= R < INT32_MAX) is the offsets o with |o|^2 <= R;
 *    with A the occupied set:
 *      ARVX_MORPH_ERODE   A' = { i in A : d(i) > R }, the border empty;
 *      ARVX_MORPH_DILATE  A' = A + { i not in A : -d(i) <= R }, clipped by the grid;
 *      ARVX_MORPH_OPEN    A' = DILATE(ERODE(A)); it never adds a voxel;
 *      ARVX_MORPH_CLOSE   B = DILATE(A), A' = { i in B : d_B(i) > R } with d_B taken under
 *                         BORDER_OCCUPIED, so that the grid's edge does not eat the model; it never
 *                         removes a voxel;
 *    R = 0 leaves the occupancy as it is under every op.
 * Everything is an integer and a minimum depends on no thread order: compared bit for bit.
 *   arvx_distance           builds the field of the current state.  The state is unchanged, nothing
 *                           is dropped, and the host is not synchronised.
 *   arvx_distance_download  the X*Y*Z values; synchronises.
 *   arvx_morph              applies the op.  A voxel that leaves A loses its occupied bit and keeps
 *                           its seen bit; a voxel that joins A gets the occupied bit, keeps its seen
 *                           bit as it was and carries no colour (MODEL_COLOR until a colour pass or a
 *                           closure gives it one).  *removed / *added (either may be null) compare the
 *                           final state with the initial one; one of them is 0 for every op.
 * The field of arvx_distance lives exactly as long as the labelling of arvx_components: until any
 * call that replaces the state, arvx_morph included; before a field and after such a call
 * arvx_distance_download answers ARVX_ERR_STATE.  arvx_morph computes the fields it needs itself and
 * leaves none behind.  It replaces the state: ERODE and OPEN only empty voxels and behave as
 * arvx_components_keep does -- they drop what photo carving drops (paint plane included) even when
 * nothing changes, and leave what earlier carves settled for whole coarse tiles valid --; DILATE and
 * CLOSE occupy voxels and drop the settled coarse tiles on top of that, as a state upload does, so
 * that a later carve looks at the new voxels.  All four end a lazy state first, refuse a state
 * holding a closure's fills whose list is gone, and drop a components labelling, a distance field
 * and the vote counts.
 * Refusals (a refused call changes nothing): a slab or a striped context, or a grid with
 * (X+1)^2 + (Y+1)^2 + (Z+1)^2 > INT32_MAX - 1, whose distances do not fit: ARVX_ERR_STATE; unknown
 * flag bits, an op outside 0..3, radius_sq outside [0, INT32_MAX), a null signed_sq:
 * ARVX_ERR_INVALID.
 * arvx_morph makes one host synchronisation, for the counts.
 * Device memory, allocated at first use and kept: 4 bytes per voxel (the field, transformed in
 * place), three bit planes (occupancy, intermediate set, change: 3/8 byte per voxel), and the column
 * passes' envelope stacks: 8 bytes per entry, (max(Y, Z) + 2) * 256 entries per workgroup, at most 4
 * workgroups per compute unit and never more than two lanes per column need (1.0 GiB at 512^3 on 256
 * compute units: the stage's largest buffer).
 * Out of scope: slabs and multi-GPU, structuring elements other than the ball, anisotropic voxels. */
#define ARVX_DISTANCE_BORDER_OCCUPIED 1u /* lattice points outside the grid are no empty sites */
#define ARVX_DISTANCE_INF 2147483647
#define ARVX_MORPH_ERODE 0
#define ARVX_MORPH_DILATE 1
#define ARVX_MORPH_OPEN 2
#define ARVX_MORPH_CLOSE 3
int arvx_distance(arvx_ctx *ctx, unsigned flags);
int arvx_distance_download(arvx_ctx *ctx, int32_t *signed_sq);
int arvx_morph(arvx_ctx *ctx, int op, int64_t radius_sq, int64_t *removed, int64_t *added);
/* The per-voxel colour lists behind the vote -- what the reference's voxel_pass appends with
 * Model::addColor (src/ColorReconstruction.h:44-60, src/Model.h:142-149) and getColors returns:
 * for each of n voxels (flat index over the context's own planes, any order) V samples in view
 * order, out[k * V + i] = view i's sample of voxel k: valid = 1 and (r, g, b) = the pixel the
 * voxel projects to in image i with depth = (float)cv::norm(cameras[i] - world), or valid = 0
 * when it projects outside the image.  Needs the cameras (with campos) and the images of the
 * colour pass (arvx_set_views, arvx_set_images); the occupancy is not looked at -- which voxels
 * a pass visits (occupied, not inner) is the caller's knowledge (arvx_surface_download). */
typedef struct arvx_color_sample {
    uint8_t r, g, b, valid;
    float depth;
} arvx_color_sample;
/* views: the samples per voxel `out` has room for -- must be the context's number of views
 * (ARVX_ERR_INVALID otherwise: a caller that sized its buffer for another set of views is told so
 * instead of being written past its end). */
int arvx_color_samples(arvx_ctx *ctx, int64_t n, const int64_t *index, int views,
                       arvx_color_sample *out);

/* Replace the device-side sparse colours by a caller-supplied list (n voxels,
 * ascending flat index, 3 floats RGB each, w = 1): lets a host Model that was
 * coloured elsewhere go through arvx_closure / arvx_export_model. */
int arvx_colors_upload(arvx_ctx *ctx, int64_t n, const int64_t *index, const float *rgb);

/* Morphological closure: reference applyClosure(model, kernel_size),
 * src/Postprocessing3d.cpp:4-100 (called at src/main.cpp:297-299 after the
 * colour pass and handleUnseen).  As in the reference the erosion half never
 * removes anything (it tests w < 0), so this is one dilation with a
 * kernel_size^3 box whose new voxels get the mean RGBA of their occupied
 * neighbours.  apply_unseen != 0: the model is taken as it is after
 * handleUnseen().  State bytes may carry bit2 (voxel painted UNSEEN_COLOR by
 * a host Model; kept beside the records as a bit plane until the next carve, plane upload or
 * reset).  bit2 is meant for occupied voxels -- the C++ Model sends it on no other, since there
 * handleUnseen occupies what it paints.  On an empty voxel it is kept as given (the byte downloads
 * unchanged) and the paint wins where colours are returned: arvx_export_model gives UNSEEN_COLOR
 * with w = 1 there, and the closure averages it as an occupied UNSEEN_COLOR neighbour.
 * Whole-grid contexts and slabs with at least r + 1 halo planes
 * (arvx_ctx_create_slab_halo): a slab fills -- and reports -- the voxels of its own planes.
 * The filled voxels become occupied;
 * arvx_export_model(ctx, ., same apply_unseen) then returns the closed model.
 * What the context's results belong to, for any order of calls:
 *   - the colour list (arvx_color, arvx_colors_upload) lives until the next carve, fast carve,
 *     state upload or reset, arvx_set_views or arvx_set_images; handleUnseen and the closure keep it;
 *   - the closure's list of filled voxels lives until any of those, arvx_handle_unseen, the next
 *     arvx_color or arvx_colors_upload;
 *   - the paint plane (bit2 of arvx_state_upload) lives until the next carve, fast carve, upload
 *     or reset;
 *   - arvx_photo_carve drops what a carve drops (the colour list, the closure's list, the mark of a
 *     closure's fills and the paint plane), even when it removes nothing; what earlier carves
 *     settled for whole coarse tiles stays valid, since it only empties voxels;
 *   - arvx_components_keep drops exactly what arvx_photo_carve drops, for the same reason;
 *   - the labelling of arvx_components lives until the next call that replaces the state: carve,
 *     vote carve, fast carve, photo carve, arvx_handle_unseen, closure, state upload, reset,
 *     arvx_components_keep or arvx_morph; the field of arvx_distance lives exactly as long;
 *   - arvx_morph with ERODE or OPEN drops exactly what arvx_components_keep drops; with DILATE or
 *     CLOSE it also drops what earlier carves settled for whole coarse tiles, as a state upload
 *     does, because it occupies voxels;
 *   - the relaxed mesh (arvx_mesh_relax) lives until the next arvx_mesh_relax or the call that
 *     replaces or ends its base mesh (arvx_mc_mesh_welded, and arvx_mc_mesh_smooth, _decimate or
 *     _refined for the base each of them builds); none of the calls above touches it.
 * A closure that filled voxels leaves them occupied in the state.  Once its list is gone the
 * context no longer has their colours, which the reference's Model keeps: until a carve, fast
 * carve, upload or reset replaces the state, the calls that return colours (arvx_export_model,
 * arvx_mc_mesh, arvx_mc_mesh_welded) and a second arvx_closure -- which would average those
 * colours -- are refused with ARVX_ERR_STATE.  A second closure is refused while the first one's
 * list is still there as well ("already applied").  Occupancy-only calls (state downloads,
 * arvx_mc_cells) and the colour pass stay available.  The C++ Model keeps the fills' colours on the
 * host and uploads state and colours again before the stages that need them. */
int arvx_closure(arvx_ctx *ctx, int kernel_size, int apply_unseen);
int arvx_closure_count(arvx_ctx *ctx, int64_t *count);
/* Filled voxels, ascending flat index, 4 floats RGBA each. */
int arvx_closure_download(arvx_ctx *ctx, int64_t *index, float *rgba);
/* The same with 32-bit indices (a grid has at most INT_MAX voxels, Model::flatten). */
int arvx_closure_download32(arvx_ctx *ctx, int32_t *index, float *rgba);

/* Marching-cubes hand-off.  The reference's marchingCubes() visits every cell
 * (x,y,z) of [-1,X) x [-1,Y) x [-1,Z), x outermost and z innermost
 * (src/MarchingCubes.cpp:12-18); a cell emits triangles only when its cube index
 * -- bit i set when corner i (order of src/MarchingCubes.h:537-552) is not part
 * of the model, :479-484 -- is neither 0 nor 255 (:486-488).  arvx_mc_cells
 * finds those cells on the device from the current occupancy and returns how
 * many there are; arvx_mc_cells_download copies them out, 4 ints per cell
 * (x, y, z, cube index), in the reference's visiting order, so that calling
 * ProcessVoxel on this list alone builds the same mesh.  Slab contexts list the
 * cells whose upper plane they own (global z; the last slab also those above the
 * grid); striped contexts are refused.  Valid for 0 < threshold <= 1, which
 * covers the 0.5 every reference call site passes.
 * The list is a snapshot of the occupancy at the walk.  It lives until the next walk: the next
 * arvx_mc_cells, arvx_mc_mesh, arvx_mc_mesh_welded or arvx_mc_mesh_refined (each runs the walk
 * itself; a call of theirs that is refused leaves the list).  No other call touches it -- a carve, an
 * upload or a reset replaces the state and leaves the list of the state before; before the first walk
 * arvx_mc_cells_download answers ARVX_ERR_STATE.  Only arvx_mc_cells returns the length: a caller
 * that downloads the list a mesh call left sizes its buffer by the bound, one cell per lattice cell,
 * (X+1) * (Y+1) * (owned planes + 1). */
int arvx_mc_cells(arvx_ctx *ctx, int64_t *count);
int arvx_mc_cells_download(arvx_ctx *ctx, int32_t *cells);

/* The triangles marchingCubes() builds from the current model (before WriteMesh scales and
 * writes them), for the models the device holds: every w is 0 or 1, threshold in (0, 1].
 * Triangle t has the three fresh vertices 3t, 3t+1, 3t+2 (src/MarchingCubes.h:561-568) --
 * `verts` gets 9 floats per triangle, voxel units -- and the face colour face_rgb[3t..3t+2]
 * (rounded mean with the reference's `i + 1` quirk, :506).  Voxel colours: UNSEEN_COLOR where
 * handleUnseen painted (apply_unseen != 0: every never-seen voxel; bit2 of uploaded bytes),
 * else the closure's colour, else the colour pass's, else MODEL_COLOR.  Whole-grid contexts and
 * slabs with enough halo planes (arvx_ctx_create_slab_halo): a slab builds the triangles of the
 * cells arvx_mc_cells lists for it (global z).  Runs arvx_mc_cells itself; the order is the
 * reference's.
 * The mesh is a snapshot of the state and the colours at the call.  It lives until the next arvx_mc_mesh
 * (a refused one leaves it): no call that replaces the state, the views or the colours touches it, and
 * neither do arvx_mc_cells, arvx_mc_mesh_welded, arvx_mc_mesh_refined and what is made of their meshes.
 * Before the first arvx_mc_mesh the mesh has no triangle: the two downloads return ARVX_OK and copy
 * nothing. */
int arvx_mc_mesh(arvx_ctx *ctx, int apply_unseen, int64_t *triangles);
int arvx_mc_mesh_download(arvx_ctx *ctx, float *verts, uint32_t *face_rgb);
/* The same triangles with whole face records, 6 uints per triangle: the vertex numbers 3t,
 * 3t+1, 3t+2, then r, g, b -- the reference's Triangle (src/MarchingCubes.h:19-31), so that a
 * host mesh takes both arrays without a conversion loop. */
int arvx_mc_mesh_download_faces(arvx_ctx *ctx, float *verts, uint32_t *faces);

/* The same mesh with shared vertices (an extension beyond the reference, which gives every
 * triangle three fresh vertices).  Definition: take the T triangles arvx_mc_mesh returns for the
 * same state and apply_unseen, vertices v[3t+k] and face colours face_rgb[t].  The welded mesh has
 *   - vertices: the distinct positions v[.], compared as float values, ascending by (z, y, x) --
 *     on the device every vertex is a lattice point, so this is Model::flatten order (x fastest):
 *     the occupied voxels with an empty 6-neighbour (out-of-grid counts as empty), closure fills
 *     included.  V of them;
 *   - faces: the same T triangles in the same order; faces[t][k] is the index of v[3t+k] in the
 *     vertex list.  Snapping makes some triangles degenerate (two or three equal indices): they are
 *     kept, as the reference writes them;
 *   - face colours: face_rgb[t], unchanged (the `i + 1` quirk included);
 *   - vertex colours: the colour Model::get returns for the vertex's voxel, with arvx_mc_mesh's
 *     precedence (UNSEEN paint, closure, colour pass, MODEL_COLOR); so for corners a, b, c:
 *     face_rgb[t] == round(((col[a] + col[b]) + col[b]) / 3) per channel in fp32.
 * arvx_mc_mesh_welded builds it with ONE host synchronisation and returns V and T; whole-grid
 * contexts only (slab and striped contexts: ARVX_ERR_STATE).  arvx_mc_mesh_welded_download copies
 * 3V floats of positions (voxel units), 6T uints of face records {i0, i1, i2, r, g, b} -- the C++
 * layer's Triangle -- and, if vertex_rgb is not null, 3V floats of vertex colours.  Runs
 * arvx_mc_cells itself; the unwelded mesh of an earlier arvx_mc_mesh stays valid.
 * The welded mesh is a snapshot of the state and the colours at the call, vertex colours included.  It
 * lives until the next arvx_mc_mesh_welded: a call that replaces the state, the views or the colours
 * leaves it, and arvx_mc_mesh_smooth, arvx_mc_mesh_decimate and the render keep working on it.  A new
 * welded mesh ends the smoothed mesh, the decimated mesh and the render of the old one.  A refused call
 * (fills whose list is gone, a closure computed with the other apply_unseen) leaves the previous mesh
 * and everything made of it; before the first mesh the download answers ARVX_ERR_STATE. */
int arvx_mc_mesh_welded(arvx_ctx *ctx, int apply_unseen, int64_t *vertices, int64_t *triangles);
int arvx_mc_mesh_welded_download(arvx_ctx *ctx, float *verts, uint32_t *faces, float *vertex_rgb);

/* Taubin smoothing and vertex normals of the welded mesh (an extension beyond the reference, whose
 * vertices all sit on the voxel lattice).  Definition, on a welded mesh with V positions p (fp32)
 * and T faces (i0, i1, i2); every fp32 operation rounded on its own (no fma), '/' and sqrtf IEEE:
 *   - neighbours: N(i) = { j != i : some face contains both i and j }, each once, ascending;
 *   - one step with factor f, per component: p'_i = p_i when N(i) is empty, else
 *     s = +0; s = s + p_j for j in N(i) ascending; m = s / (float)|N(i)|; d = m - p_i;
 *     p'_i = p_i + (f * d).  Every vertex reads the previous step's positions (Jacobi);
 *   - Taubin (iterations, lambda, mu): 2 * iterations steps with factors lambda, mu, lambda, mu,
 *     ... (iterations = 0: the positions unchanged; mu = 0: plain Laplacian smoothing).  The
 *     usual factors are lambda = 0.5, mu = -0.53;
 *   - vertex normals on the final positions q: per face c_t = a x b with a = q[i2] - q[i0],
 *     b = q[i1] - q[i0] (c_t.x = a.y*b.z - a.z*b.y, and so on; the mesh's own winding points into
 *     the model, this points out); n_i = sum of c_t over the faces that contain i, each face once,
 *     in ascending t from +0; l = sqrtf((n.x*n.x + n.y*n.y) + n.z*n.z); normal = n / l per
 *     component, (0, 0, 0) when l == 0.
 * arvx_mc_mesh_smooth acts on the mesh of the last arvx_mc_mesh_welded (none: ARVX_ERR_STATE, as
 * on slab and striped contexts; iterations < 0 or a factor that is not finite: ARVX_ERR_INVALID).
 * It does not synchronise.  The adjacency is built at the first call on a welded mesh and reused
 * by the next ones; arvx_mc_mesh_welded_download keeps returning the lattice positions.
 * arvx_mc_mesh_smooth_download copies 3V floats of positions and 3V floats of unit normals; either
 * pointer may be null (ARVX_ERR_STATE before the first arvx_mc_mesh_smooth on the welded mesh).
 * The smoothed mesh is replaced by the next arvx_mc_mesh_smooth and ended by the next
 * arvx_mc_mesh_welded; nothing else touches it. */
int arvx_mc_mesh_smooth(arvx_ctx *ctx, int iterations, float lambda, float mu);
int arvx_mc_mesh_smooth_download(arvx_ctx *ctx, float *verts, float *normals);

/* The welded mesh reduced by vertex clustering (Rossignac-Borrel; an extension beyond the
 * reference).  Definition, on the welded mesh of the last arvx_mc_mesh_welded -- V vertices with
 * lattice positions l_i (integers stored as fp32), vertex colours col_i, T face records {i0, i1,
 * i2, r, g, b} --, an integer cell, 1 <= cell <= 64, and a source: ARVX_DECIMATE_LATTICE with
 * q_i = l_i, or ARVX_DECIMATE_SMOOTHED with q_i the positions of the last arvx_mc_mesh_smooth on
 * this welded mesh:
 *   - the cluster of vertex i is (l_i.x / cell, l_i.y / cell, l_i.z / cell), integer division; its
 *     flat index is taken over a cluster grid of ceil(X / cell) x ceil(Y / cell) x ceil(Z / cell),
 *     x fastest;
 *   - decimated vertices: the non-empty clusters in ascending flat index, Vd of them; map[i] is the
 *     decimated index of welded vertex i;
 *   - the members of a cluster are its welded vertices in ascending i (ascending (z, y, x) inside
 *     the cluster's box); members[d] is their count n;
 *   - position and colour of a decimated vertex, per component, every fp32 operation rounded on its
 *     own (no fma): s = +0; s = s + q_i over the members ascending; the result is s / (float)n, an
 *     IEEE quotient.  The colour is the same sum over col_i;
 *   - clustering always uses the lattice positions: the clusters, map, members, the colours and
 *     the faces do not depend on the source;
 *   - faces: face t maps to (map[i0], map[i1], map[i2]).  A face with two equal mapped corners is
 *     dropped.  Among the faces with the same set of three mapped corners (unordered, whatever the
 *     winding) only the one with the least t stays.  The survivors keep ascending t order, their
 *     corner order (the winding) and their own r, g, b.  Td of them.
 * So cell = 1 gives Vd = V, the positions unchanged, and the welded mesh without its degenerate and
 * repeated faces; a cell no smaller than the grid gives Vd <= 1 and Td = 0; an empty welded mesh
 * gives 0 and 0.
 * arvx_mc_mesh_decimate acts on the context's welded mesh with ONE host synchronisation and returns
 * Vd and Td.  Its buffers are sized from the bounds the host knows -- Vd <= min(V, clusters),
 * Td <= T --, so nothing is retried; beside the outputs (24 Vd + 4 Vd + 4 V + 24 T bytes) it keeps
 * 8 T bytes of flags and offsets, the cluster plane and, for the duplicate test, a table of 78
 * 4-byte slots -- 312 bytes -- per possible decimated vertex, all sized at first use and kept.
 * arvx_mc_mesh_decimate_download copies 3 Vd floats of positions, 6 Td uints of face records,
 * 3 Vd floats of colours, Vd member counts and V map entries; any pointer may be null.
 * Refusals.  ARVX_ERR_STATE: no welded mesh (slab and striped contexts never have one);
 * ARVX_DECIMATE_SMOOTHED without a smoothed mesh on this welded mesh; a download before a
 * decimation.  ARVX_ERR_INVALID: cell outside [1, 64]; an unknown source; null count pointers.  A
 * refused call leaves the previous decimated mesh as it was.
 * The decimated mesh lives until the next arvx_mc_mesh_decimate or the next arvx_mc_mesh_welded.
 * It changes nothing else: the welded and smoothed meshes, a render and arvx_mc_mesh stay as they
 * were. */
#define ARVX_DECIMATE_LATTICE 0
#define ARVX_DECIMATE_SMOOTHED 1
int arvx_mc_mesh_decimate(arvx_ctx *ctx, int cell, int source, int64_t *vertices, int64_t *triangles);
int arvx_mc_mesh_decimate_download(arvx_ctx *ctx, float *verts, uint32_t *faces, float *vertex_rgb,
                                   int32_t *members, int32_t *map);

/* The refined mesh: marching cubes with one vertex per cut edge, placed where the edge leaves the
 * visual hull (the classic visual-hull refinement; an extension beyond the reference, whose
 * VertexInterp snaps every cut edge to its occupied corner).  The views' background bit planes and
 * matrices say for any point of space whether it lies in the hull, so a few bisection steps along a
 * cut edge find where it leaves.  Definition, on a whole-grid context, its current state,
 * apply_unseen and an integer bisections = B, 0 <= B <= 10:
 *   - cells: the cells, their order and their cube indices are those of arvx_mc_cells;
 *   - cut edges: a lattice edge between two points one step apart along x, y or z of which exactly
 *     one is occupied (out of the grid counts as empty; occupied as arvx_mc_cells reads it, closure
 *     fills included).  Its lower end is q (the componentwise minimum), its axis a in {0, 1, 2};
 *   - vertices: one per cut edge, ascending by the key
 *     (((q.z+1) * (Y+1) + (q.y+1)) * (X+1) + (q.x+1)) * 3 + a.  Vr of them;
 *   - faces: the T triangles of arvx_mc_mesh for the same state in the same order.  Corner k of
 *     triangle t came from edge e of its cell, between corners e % 8 and MC_SECOND[e]
 *     (include/arvx/mc_tables.hpp, kSecondCorner); it becomes the index of that cut edge's vertex.
 *     r, g, b are arvx_mc_mesh's face_rgb[t], unchanged.  So T is arvx_mc_mesh's T, no face repeats
 *     an index, and every vertex is used;
 *   - inside(p), for a point p = (px, py, pz) in fp32 voxel coordinates: there is no view in which p
 *     projects into the image onto a background pixel.  The projection is the carve's own with
 *     coordinates in place of integers: world = (py * s, px * s, (-pz) * s, 1) in fp32, the rows'
 *     fp64 products summed in the context's grouping and rounded to fp32, the two quotients IEEE
 *     fp32 divisions, rounding std::round; a non-finite or out-of-range value or a pixel outside the
 *     image means the view does not see p.  For integer p this is exactly what arvx_carve tests;
 *   - cut position: for an edge with occupied end A and empty end E, a SILHOUETTE edge is one with
 *     inside(A) && !inside(E).  For it: lo = 0, hi = 2^B; B times: mid = (lo + hi) / 2, and if
 *     inside(A + (mid / 2^B) (E - A)) then lo = mid, else hi = mid; then n = lo + hi.  Every other
 *     edge -- one the silhouettes do not explain: a pit cut by photo carving, an eroded or dilated
 *     surface, an uploaded state -- takes n = 2^B, the midpoint.  The vertex is A with n / 2^(B+1)
 *     added to or subtracted from its component along the axis, towards E.  With B <= 10 and no grid
 *     side above 4096 every such value is exact in fp32.  B = 0 is plain midpoint marching cubes;
 *   - vertex colour: the colour arvx_mc_mesh_welded gives the occupied end's voxel, with the same
 *     precedence (UNSEEN paint, closure, colour pass, MODEL_COLOR).
 * arvx_mc_mesh_refined builds it with ONE host synchronisation, for the counts, and returns Vr and
 * T.  Its buffers are sized by the list protocol of the other meshes (what the last call needed, or
 * a surface's share; a mesh that outgrew them is built once more) and nothing falls back to the
 * host.  Device memory beside the outputs (44 Vr + 24 T bytes): the occupancy plane (1 bit per
 * voxel) and the edge plane with its ranks (3 bits and 6 bytes per 8 lattice points), kept.
 * arvx_mc_mesh_refined_download copies 3 Vr floats of positions (voxel units), 6 T uints of face
 * records {i0, i1, i2, r, g, b}, 3 Vr floats of vertex colours, 4 Vr ints of edges -- x, y, z of the
 * OCCUPIED end, then the direction to the empty end: 0 +x, 1 -x, 2 +y, 3 -y, 4 +z, 5 -z, plus 8
 * when the edge is not a silhouette edge -- and Vr ints of n; any pointer may be null.
 * Refusals.  ARVX_ERR_STATE: a slab or a striped context; views set without masks, or no views at
 * all, when B > 0 (B = 0 needs none: no edge is a silhouette edge then); a state holding a closure's
 * fills whose list is gone, as for arvx_mc_mesh; a grid side above 4096, or a grid with
 * 3 (X+1)(Y+1)(Z+1) > INT32_MAX, whose keys do not fit 32 bits; a download before a mesh.
 * ARVX_ERR_INVALID: B outside [0, 10]; null count pointers.  A refused call leaves the previous
 * refined mesh as it was.
 * The refined mesh lives until the next arvx_mc_mesh_refined.  It is a snapshot of the state and the
 * views at the call and touches no other product -- the unwelded, welded, smoothed and decimated
 * meshes and a render stay as they were; like arvx_mc_mesh_welded it runs arvx_mc_cells itself.
 * Out of scope: decimating this mesh (arvx_render_mesh draws it; arvx_mesh_relax smooths it and gives
 * its normals); slabs and multi-GPU; colour interpolation along the edge (arvx_mesh_color samples the
 * photographs at the vertex itself instead). */
int arvx_mc_mesh_refined(arvx_ctx *ctx, int apply_unseen, int bisections, int64_t *vertices,
                         int64_t *triangles);
int arvx_mc_mesh_refined_download(arvx_ctx *ctx, float *verts, uint32_t *faces, float *vertex_rgb,
                                  int32_t *edges, int32_t *cut);

/* ---- relaxed mesh: Taubin smoothing and vertex normals of any mesh (extension beyond the reference) --
 * arvx_mc_mesh_smooth's stage for every mesh with shared vertices the context holds, and for a caller's.
 * Input: the V positions p (fp32) and the T faces (i0, i1, i2) of `source`, one of ARVX_MESH_WELDED,
 * ARVX_MESH_SMOOTHED (the welded faces with the positions of the last arvx_mc_mesh_smooth),
 * ARVX_MESH_DECIMATED, ARVX_MESH_REFINED: the positions and face records the arvx_render_mesh family
 * draws for that source.  A source with an ARVX_MESH_IMAGE_COLORS or ARVX_MESH_TEXTURED bit, and
 * ARVX_MESH_RELAXED itself, are ARVX_ERR_INVALID.
 * Result: exactly the definition of arvx_mc_mesh_smooth (its block above: neighbours N(i), ascending,
 * each once; the Jacobi step with factor f; Taubin as 2 * iterations steps with factors lambda, mu,
 * lambda, mu, ...; the normals from the final positions q -- c_t per face, summed per vertex in
 * ascending t from +0, then normalised, (0, 0, 0) when the length is 0), applied to that mesh, bit for
 * bit, with every fp32 operation rounded on its own.  The mesh may have any valence, may hold a face
 * more than once (each copy is a face of its own: it adds its c_t again and no neighbour) and faces
 * with a repeated corner.  Such a face has a = 0 or b = 0 or a = b, so c_t = (+-0, +-0, +-0) for finite
 * positions: it changes no sum that starts at +0, and the implementation leaves it out of the normals'
 * sums as the welded one does; its distinct corners are neighbours of each other all the same.
 * degree[i] = |N(i)|.  A vertex no face uses keeps its position, has normal (0, 0, 0) and degree 0.
 * The sums of a vertex are serial, in the definition's order, whatever its valence: no result depends
 * on the order the device's threads run in.
 * Product: "the relaxed mesh" -- q (3 V floats), normals (3 V floats), degree (V int32) --, tagged with
 * its base `source`; one per context.  arvx_mesh_relax does not synchronise.  arvx_mesh_relax_download
 * synchronises; any of its pointers may be null.  arvx_mesh_relax_info returns the base source, V and
 * T (ARVX_ERR_STATE without a product).
 * ARVX_MESH_RELAXED as a source of arvx_render_mesh, _view, _agreement, arvx_mesh_color and
 * arvx_mesh_texture (and, OR-ed with ARVX_MESH_IMAGE_COLORS or ARVX_MESH_TEXTURED, of the renders): the
 * faces and vertex colours of the product's base mesh with the product's positions; ARVX_ERR_STATE
 * without a product.
 * Lifetime: the product is replaced by the next arvx_mesh_relax and ended by whatever replaces or ends
 * its base -- base WELDED: arvx_mc_mesh_welded; SMOOTHED: arvx_mc_mesh_welded, arvx_mc_mesh_smooth;
 * DECIMATED: arvx_mc_mesh_welded, arvx_mc_mesh_decimate; REFINED: arvx_mc_mesh_refined.  Nothing else
 * touches it (a carve, an upload, new views, a render leave it), and it touches nothing else: the four
 * meshes, the current render and arvx_mc_mesh_smooth's product stay as they are.  The image colours
 * and the texture of source ARVX_MESH_RELAXED end where the product is replaced or ended.  A refused
 * call leaves the previous product as it was.
 * The adjacency (a neighbour CSR and an incidence CSR) is built on the device at the first call on a
 * base mesh and reused by later calls that name the same faces (WELDED and SMOOTHED share theirs) while
 * that mesh has not been built again.
 * Refusals.  ARVX_ERR_STATE: the source mesh does not exist (slab and striped contexts never have
 * one); 6 T or 3 V above INT32_MAX (the CSR offsets are 32-bit); info or download before a product.
 * ARVX_ERR_INVALID: iterations < 0, a factor that is not finite, an unknown source (see above).
 * arvx_mesh_relax_triangles does the same for a caller's mesh: nv positions (3 floats each) and nt face
 * records of 6 uints, as the mesh downloads return them and arvx_render_triangles takes them (r, g, b
 * are not read).  It copies the mesh in, relaxes it in buffers of its own, copies the three outputs
 * out (any may be null) and synchronises; the context's relaxed mesh and everything else stay as they
 * were.  Refused, on the host, before anything is enqueued -- ARVX_ERR_STATE: a slab or a striped
 * context (as arvx_render_triangles); ARVX_ERR_INVALID: iterations < 0 or a factor that is not finite,
 * a negative count, a null array with a non-zero count, 6 nt or 3 nv above INT32_MAX, a face index
 * >= nv, a coordinate that is not finite or has |c| > 2^20 (so that no product of the normals
 * overflows).  nv == 0 or nt == 0 is legal: positions unchanged, normals 0, degrees 0.
 * Device memory, beside the base mesh: the CSRs -- 16 V + 36 T bytes (four arrays of V + 1 ints; 6 T
 * neighbour slots and 3 T incidences of 4 bytes; rows are sorted in place and not compacted) and the
 * list of rows longer than 48 slots (at most 4 bytes per 49 slots) --, kept with the product; the
 * ping-pong positions 24 V (none for iterations == 0), the cross products 12 T, the normals 12 V; the
 * degrees are the CSR's first array.  A caller's mesh takes the same again plus its copy, 12 nv + 24 nt.
 * Out of scope: boundary pinning, constraining refined vertices to their edges, consuming the normals
 * in the renders and the colour votes, slabs and multi-GPU. */
/* (5, not 4: source 4 has been refused as unknown, ARVX_ERR_INVALID, by every call that takes a source, and
 * callers rely on that; it stays unknown.) */
#define ARVX_MESH_RELAXED 5 /* a source of the arvx_render_mesh / arvx_mesh_color / arvx_mesh_texture families */
int arvx_mesh_relax(arvx_ctx *ctx, int source, int iterations, float lambda, float mu);
int arvx_mesh_relax_info(arvx_ctx *ctx, int64_t out[3]); /* base source, V, T */
int arvx_mesh_relax_download(arvx_ctx *ctx, float *verts, float *normals, int32_t *degree);
int arvx_mesh_relax_triangles(arvx_ctx *ctx, int64_t nv, const float *verts, int64_t nt, const uint32_t *faces,
                              int iterations, float lambda, float mu, float *out_verts, float *out_normals,
                              int32_t *out_degree);

/* ---- render (extension beyond the reference) -------------------------------------------------
 * Draws the welded mesh's vertex voxels into a camera view: the model over a photograph, the voxel
 * under a pixel, a carve checked against its own silhouettes.  Definition, on a whole-grid context
 * that holds the mesh of the last arvx_mc_mesh_welded: its Vn vertex voxels k = 0 .. Vn-1 in
 * ascending flat index, their colours col[k] (3 floats: what arvx_mc_mesh_welded_download returns
 * as vertex_rgb), and the caller's camera: M, 12 fp32 values, row-major 3 x 4, world -> pixel, and
 * the image size W x H, 1 <= W, H <= 16384 (the views' limit).  The camera has nothing to do with
 * the context's views.
 *  1. Footprint.  For vertex voxel k, steps 1 and 2 of arvx_color_visible's definition with
 *     M, W, H in place of M_v, W, H (the same fp64 products of fp32 operands, the context's
 *     row-sum grouping, IEEE fp32 quotients): the centre's a2, whether k splats, and its clipped
 *     pixel rectangle, which may be empty.
 *  2. Winner.  For pixel p, among the voxels that splat with p in their footprint, the one with
 *     the lexicographically least (a2, k); there may be none.  a2 is a positive fp32, so the
 *     winner is the minimum of the 64-bit words bits(a2) << 32 | k: the order in which voxels
 *     arrive cannot change it.
 *  3. Images, each H x W row-major:
 *       id     int32: the winner's k (an index into the welded vertex list); -1 where there is none;
 *       depth  fp32: the winner's a2; +inf where there is none;
 *       bgr    u8, 3 channels, laid out like the input images: for the winner, channel
 *              c = (uint8_t)roundf(fminf(fmaxf(col_c, 0.f), 255.f)), stored B, G, R; where there is
 *              no winner, the pixel of the caller's background image if one was given, else
 *              (0, 0, 0).
 * Consequence: depth equals, bit for bit, the depth buffer Z of arvx_color_visible's step 3 computed
 * over the same voxel set with the same camera.
 * arvx_render takes the camera and an optional background (host memory, H rows of bg_stride >= 3 W
 * bytes, BGR; it is copied before the call returns); arvx_render_view takes M_v, W, H of the
 * context's view `view` and no background.  Neither synchronises; arvx_render_download does, and
 * copies the tightly packed images out (any pointer may be null).  arvx_render_agreement renders
 * view `view` as arvx_render_view does, leaves that render as the current one, and counts on the
 * device, against the view's background bit plane (the one arvx_selftest_view_tables returns):
 *   counts[0] = pixels covered and foreground, counts[1] = covered and background,
 *   counts[2] = uncovered and foreground -- with ONE host synchronisation.
 * An empty mesh (Vn == 0) renders the background.
 * Refusals.  ARVX_ERR_STATE: no welded mesh (slab and striped contexts never have one);
 * arvx_render_download before a render; arvx_render_view or arvx_render_agreement without views;
 * arvx_render_agreement when the views were set with masks == NULL.  ARVX_ERR_INVALID: a null M or
 * a non-finite entry of it, W or H out of range, bg_stride < 3 W, a view outside [0, V), null
 * counts.  A refused call leaves the previous render as it was.
 * The render always draws the held welded mesh with the colours that mesh was built with, also after
 * the state has moved on.  It lives until the next render, the next arvx_mc_mesh_welded, or a call that
 * replaces the state the mesh was built from: every call that replaces occupied or seen bits other than
 * arvx_handle_unseen and arvx_closure -- carve, vote carve, fast carve, photo carve,
 * arvx_components_keep, arvx_morph (all four ops, a radius of 0 too), the state uploads and reset.  The
 * colour calls, arvx_set_views, arvx_set_images, arvx_handle_unseen, arvx_closure, arvx_components,
 * arvx_distance, arvx_mc_cells, arvx_mc_mesh, arvx_mc_mesh_refined, arvx_mc_mesh_smooth and
 * arvx_mc_mesh_decimate keep it.  Device
 * memory, sized at first use and kept: W * H * 8 bytes of keys, the three images (W * H * 11
 * bytes) and the large-footprint list. */
int arvx_render(arvx_ctx *ctx, const float M[12], int W, int H, const uint8_t *background,
                size_t bg_stride);
int arvx_render_view(arvx_ctx *ctx, int view);
int arvx_render_download(arvx_ctx *ctx, uint8_t *bgr, float *depth, int32_t *id);
int arvx_render_agreement(arvx_ctx *ctx, int view, int64_t counts[3]);

/* ---- triangle render (extension beyond the reference) -----------------------------------------
 * Draws a mesh's triangles into a camera view with a depth buffer: any mesh the context holds, or a
 * caller's.  Definition, bit for bit and without a thread order in it; the library is built with
 * -ffp-contract=off, so every operation below is rounded on its own, and '/' is IEEE.  Inputs: V
 * positions p (fp32 voxel coordinates x, y, z), V vertex colours col (fp32 r, g, b), T faces (i0, i1,
 * i2), the camera M with W x H as for arvx_render, the context's voxel size s and row-sum grouping.
 *  1. Vertex.  (a0, a1, a2) is the refined mesh's projection of a point: world = (py * s, px * s,
 *     (-pz) * s, 1) in fp32, the rows' fp64 products summed in the context's grouping and rounded to
 *     fp32.  qu = a0 / a2, qv = a1 / a2.  The vertex is VALID iff a2 >= FLT_MIN (normal, positive), qu
 *     and qv are finite, |qu| <= 32768 and |qv| <= 32768.  Its fixed-point position is
 *     fx = (int)std::round(qu * 16.0f), fy = (int)std::round(qv * 16.0f): the products are exact and
 *     |fx|, |fy| <= 2^19.  Pixel (c, r) is the point (16 c, 16 r): pixel centres are the integers, as
 *     everywhere in this library.
 *  2. Triangle.  REFUSED if a corner is not VALID (near-plane clipping: below).  With corners (x0, y0),
 *     (x1, y1), (x2, y2): A = (x1 - x0)(y2 - y0) - (x2 - x0)(y1 - y0) in int64; FLAT if A == 0.  Both
 *     windings are drawn.
 *  3. Coverage.  For P = (px, py) = (16 c, 16 r): E0 = (x1 - px)(y2 - py) - (x2 - px)(y1 - py),
 *     E1 = (x2 - px)(y0 - py) - (x0 - px)(y2 - py), E2 = (x0 - px)(y1 - py) - (x1 - px)(y0 - py), int64
 *     and exact (|E| < 2^42; E0 + E1 + E2 = A).  If A < 0, all four are negated.  The pixel is COVERED
 *     iff E0, E1, E2 >= 0: edges are inclusive on every side, so two faces that share an edge both
 *     cover its pixels and step 4 decides.  Only pixels with 0 <= c < W, 0 <= r < H,
 *     ceil(min fx / 16) <= c <= floor(max fx / 16) and the same in r can be covered (floor and ceil
 *     towards -inf and +inf).  A valid triangle with an area that covers no pixel is EMPTY, every
 *     other one DRAWN: each triangle is in exactly one of the four classes.
 *  4. Depth and winner.  iz_i = 1.0 / (double)a2_i of corner i; t_i = (double)E_i * iz_i;
 *     S = (t0 + t1) + t2; depth = (float)((double)A / S): perspective-correct, positive.  The winner of
 *     a pixel is the minimum of bits(depth) << 32 | t over the triangles t that cover it: the nearest,
 *     among equally near ones the least t, whatever the order in which triangles arrive.
 *  5. Colour of the winner, per channel: n = (t0 * col[i0] + t1 * col[i1]) + t2 * col[i2] in fp64,
 *     v = (float)(n / S).  With a light L (3 finite floats along the voxel axes x, y, z): c = a x b
 *     with a = p[i2] - p[i0], b = p[i1] - p[i0] (the smoothing block's face normal, fp32);
 *     l = sqrtf((c.x * c.x + c.y * c.y) + c.z * c.z), m the same expression over L;
 *     d = (c.x * L.x + c.y * L.y) + c.z * L.z; f = (l == 0 || m == 0) ? 1 : fminf(fabsf(d) / (l * m), 1);
 *     v = (0.25f + 0.75f * f) * v.  The pixel's channel is arvx_render's
 *     (uint8_t)roundf(fminf(fmaxf(v, 0.f), 255.f)), stored B, G, R.
 *  6. Images, as arvx_render's: id = the winner's t, an index into the source's face list (-1 where
 *     there is none), depth (+inf where there is none), bgr (the background or zeros where there is
 *     none).
 * Sources: ARVX_MESH_WELDED -- the mesh of arvx_mc_mesh_welded, lattice positions --,
 * ARVX_MESH_SMOOTHED -- the same faces and colours with the positions of the last arvx_mc_mesh_smooth
 * --, ARVX_MESH_DECIMATED -- arvx_mc_mesh_decimate's --, ARVX_MESH_REFINED -- arvx_mc_mesh_refined's
 * --, ARVX_MESH_RELAXED -- the faces and colours of arvx_mesh_relax's base with its positions.
 * arvx_render_triangles draws a caller's mesh instead: nv positions and colours (3 floats each), nt
 * face records {i0, i1, i2, r, g, b} as the mesh downloads return them (r, g, b are not read); the
 * arrays are copied before the call returns, into buffers of their own.
 * arvx_render_mesh takes the camera, an optional background and an optional light (NULL: unshaded) as
 * arvx_render does; arvx_render_mesh_view takes M_v, W, H of the context's view.  Neither
 * synchronises.  The result is the context's current render: arvx_render_download returns it, and it
 * lives and ends exactly as a render of arvx_render does (its lifetime paragraph; the next render of
 * either kind replaces it).  The images are resolved inside the call: a later change of the source
 * mesh does not touch them.  arvx_render_mesh_agreement renders view `view` unshaded, leaves that
 * render as the current one and counts as arvx_render_agreement does, with ONE host synchronisation.
 * arvx_render_mesh_stats returns the class counts of the current render, {DRAWN, EMPTY, FLAT,
 * REFUSED}; they sum to T; it synchronises.  An empty mesh renders the background.
 * Near plane (arvx_ctx_set_render_near; 0, the default: none, and everything above holds as it
 * stands).  With near = n > 0, steps 1-6 stay as they are except for the following.
 *  Front and behind.  Corner i is IN FRONT iff a2_i >= n (a NaN is behind).  All three corners in
 *     front: the triangle is treated exactly as above.  None in front: REFUSED, and counted as WHOLLY
 *     BEHIND.  Otherwise the face STRADDLES the plane.
 *  Clipped vertex C(i, j) of an edge with exactly one end in front: with lo < hi its two VERTEX
 *     indices in index order (not face order: two faces that share the edge compute the same vertex,
 *     bit for bit), t = ((double)n - (double)a2_lo) / ((double)a2_hi - (double)a2_lo);
 *     c0 = (float)((double)a0_lo + t * ((double)a0_hi - (double)a0_lo)), c1 the same from a1; its a2
 *     is n exactly; qu = c0 / n, qv = c1 / n; VALID and fx, fy are decided as in step 1.  Its weights
 *     towards the face's corners are B_hi = (float)t, B_lo = (float)(1.0 - t) and 0 for the third; an
 *     original corner has the unit weight vector.
 *  Polygon and pieces, the face's corners P_0, P_1, P_2 in face order, indices mod 3.  One corner r
 *     in front: (P_r, C(r, r+1), C(r+2, r)), one piece.  Two in front, r and r+1: (v0, v1, v2, v3) =
 *     (P_r, P_{r+1}, C(r+1, r+2), C(r+2, r)); piece 0 is (v0, v1, v2), piece 1 (v0, v2, v3).  Each
 *     piece goes through steps 2-4 as a triangle of its own corners: one with a corner that is not
 *     VALID is REFUSED; iz of a clipped corner is 1.0 / (double)n.  The key is still
 *     bits(depth) << 32 | t with t the FACE.
 *  Winner and colour.  The winner of a pixel is the minimum of (bits(depth), t, k), k the piece:
 *     the key is unchanged, and k is the least piece of face t that covers the pixel with exactly
 *     that depth.  With the piece's t_0, t_1, t_2, S and the rows B_0, B_1, B_2 of its corners:
 *     w_j = (t_0 * (double)B_0j + t_1 * (double)B_1j) + t_2 * (double)B_2j, j = 0, 1, 2; step 5 (and
 *     the mesh textures' lookup) runs with (w_0, w_1, w_2, S) and the face's corners' colours.  For
 *     an unclipped triangle B is the identity and w_j = t_j exactly.  The shade is the face's.
 *  Classes.  id is the face.  A straddling face takes the best class among its pieces, in the order
 *     DRAWN, EMPTY, FLAT, REFUSED; the four classes still sum to T.
 * arvx_ctx_set_render_near sets n for the context, as arvx_ctx_set_view_window sets its switch: it
 * drops no product and leaves the current render alone, and holds from the next arvx_render_mesh,
 * _view, _agreement or arvx_render_triangles on, with ARVX_MESH_IMAGE_COLORS and ARVX_MESH_TEXTURED
 * too.  near == 0: off; a finite near >= FLT_MIN: on; a negative, NaN, infinite or subnormal one:
 * ARVX_ERR_INVALID, nothing changed.  arvx_ctx_render_near returns it.  arvx_render (the voxel
 * render), arvx_mesh_color and arvx_mesh_texture ignore it.  arvx_render_mesh_clip_stats returns
 * {faces wholly behind, faces that straddle, pieces made, pieces DRAWN} of the current render (zeros
 * for one made with the plane off); it synchronises; ARVX_ERR_STATE when the current render is no
 * triangle render.  With the plane on, the four counts lie behind the list (32 bytes).
 * Refusals.  ARVX_ERR_STATE: the source mesh does not exist (slab and striped contexts never have
 * one); the _view and _agreement forms without views, or the agreement form when the views were set
 * with masks == NULL; arvx_render_mesh_stats when the current render is no triangle render;
 * arvx_render_triangles on a slab or a striped context.  ARVX_ERR_INVALID: an unknown source; a null
 * M or a non-finite entry of it, W or H out of range, bg_stride < 3 W, a view outside [0, V), a
 * non-finite light, null counts; for arvx_render_triangles a negative count, a null array with a
 * non-zero count, or a face index >= nv (checked on the host before anything is enqueued).  A refused
 * call leaves the previous render as it was.
 * Device memory beside the render's, sized at first use and kept: 16 bytes per vertex of projected
 * positions and the list of triangles whose pixel box exceeds 64 pixels (16 bytes each), swept by a
 * wave each; what does not fit the list is swept by the wave that found it.
 * Out of scope: guard-band clipping (a piece with a corner that is not VALID is REFUSED), a far plane,
 * anti-aliasing, per-vertex normals, slabs and multi-GPU.  (Textures: the mesh textures' block below, ARVX_MESH_TEXTURED.) */
#define ARVX_MESH_WELDED 0
#define ARVX_MESH_SMOOTHED 1
#define ARVX_MESH_DECIMATED 2
#define ARVX_MESH_REFINED 3
int arvx_render_mesh(arvx_ctx *ctx, int source, const float M[12], int W, int H, const uint8_t *background,
                     size_t bg_stride, const float *light);
int arvx_render_mesh_view(arvx_ctx *ctx, int source, int view, const float *light);
int arvx_render_mesh_agreement(arvx_ctx *ctx, int source, int view, int64_t counts[3]);
int arvx_render_triangles(arvx_ctx *ctx, int64_t nv, const float *verts, const float *vertex_rgb, int64_t nt,
                          const uint32_t *faces, const float M[12], int W, int H, const uint8_t *background,
                          size_t bg_stride, const float *light);
int arvx_render_mesh_stats(arvx_ctx *ctx, int64_t out[4]);
int arvx_ctx_set_render_near(arvx_ctx *ctx, float near); /* 0: off (default) */
int arvx_ctx_render_near(const arvx_ctx *ctx, float *near);
int arvx_render_mesh_clip_stats(arvx_ctx *ctx, int64_t out[4]);
/* Self-test hook: room of the triangle render's list of large pixel boxes from the next render on
 * (0: everything large is swept in place; -1: the default sizing), and of arvx_render's list of large
 * footprints.  The room changes the time, never the images. */
int arvx_selftest_render_mesh_list(arvx_ctx *ctx, int64_t cap);
/* Self-test hook: the compute-unit count that sizes the context's launches from the next call on
 * (every grid and ticket pool that is "so many workgroups per compute unit"), as a partition of the
 * device would show it.  0: back to the device's own count; 1 .. the device's count: that many;
 * anything else: ARVX_ERR_INVALID, nothing changed -- the hook only ever shrinks a launch.  The count
 * changes the time, never a result. */
int arvx_selftest_compute_units(arvx_ctx *ctx, int n);

/* ---- mesh colours from the images (extension beyond the reference) -----------------------------
 * Colours the vertices of a held mesh from the photographs: per view the depth buffer of the mesh's
 * own triangles, per vertex a vote over the views that really see it, sampled bilinearly.  Definition,
 * bit for bit and without a thread order in it.  Inputs: a whole-grid context; its V views (M_v, W, H)
 * and its images (arvx_set_images, BGR u8, I_v[r, c] per channel); a source mesh among ARVX_MESH_WELDED,
 * _SMOOTHED, _DECIMATED, _REFINED with its Vn positions p, vertex colours col and T faces -- exactly
 * the arrays arvx_render_mesh would draw --; mode ARVX_COLOR_CLOSEST or ARVX_COLOR_AVERAGE; tol >= 0,
 * finite or +inf, in the units of a2.
 *  1. Projection.  For vertex i and view v, step 1 of the triangle render with M_v: a2, VALID, fx, fy
 *     (the same code, the same bits).
 *  2. Depth buffer.  D_v is the depth image arvx_render_mesh_view(source, v, NULL) defines: steps 2-4
 *     of the triangle render over all T faces, +inf where no triangle covers the pixel.
 *  3. Candidate.  Vertex i is IN IMAGE in v iff it is VALID, 0 <= fx <= 16 (W - 1) and
 *     0 <= fy <= 16 (H - 1).  Its nearest pixel is cn = (fx + 8) >> 4, rn = (fy + 8) >> 4.  It is
 *     VISIBLE in v iff it is in image and a2 <= D_v[rn, cn] + tol (one fp32 addition) and -- with
 *     ARVX_MESH_COLOR_FOREGROUND only -- pixel (cn, rn) is foreground in the view's background bit
 *     plane (the one arvx_selftest_view_tables returns).  A vertex on the hull's rim is, in the view
 *     whose silhouette it lies on, a grazing sample next to the photograph's background: the flag
 *     drops that view.
 *  4. Sample, in integers.  c0 = fx >> 4, r0 = fy >> 4, wx = fx & 15, wy = fy & 15,
 *     c1 = min(c0 + 1, W - 1), r1 = min(r0 + 1, H - 1) (the clamp only ever meets a weight of 0).  Per
 *     channel S = (16 - wx)(16 - wy) I[r0, c0] + wx (16 - wy) I[r0, c1] + (16 - wx) wy I[r1, c0]
 *     + wx wy I[r1, c1]: an integer in [0, 255 * 256]; the sample is S / 256.
 *  5. Vote over the visible views, n of them.  CLOSEST: the visible view with the least a2, compared
 *     as fp32 with strict < in ascending view order (the first view wins ties: arvx_color's rule);
 *     rgb_c = (float)S_c / 256.0f, exact.  AVERAGE: Sum_c the integer sum of S_c over the visible views
 *     (64 bits: no order matters); rgb_c = (float)((double)Sum_c / (double)(256 n)).  n == 0:
 *     rgb = col[i], the source's own vertex colour.
 *  6. Product: vertex_rgb, 3 Vn floats r, g, b; views, Vn int32, the value n; *coloured, the number of
 *     vertices with n > 0.  An empty mesh gives 0 and empty arrays.
 * Consequence: arvx_mesh_color_depth_download(v) equals, bit for bit, the depth arvx_render_download
 * returns after arvx_render_mesh_view(source, v, NULL).
 * arvx_mesh_color takes ONE host synchronisation, for *coloured; nothing falls back to the host.
 * arvx_mesh_color_count returns Vn and the count again (host bookkeeping; either pointer may be
 * null); arvx_mesh_color_download copies vertex_rgb and views (either may be null);
 * arvx_mesh_color_depth_download copies D_v, H x W floats.
 * Drawing: in arvx_render_mesh, _view and _agreement, source | ARVX_MESH_IMAGE_COLORS draws the same
 * mesh with the product's vertex_rgb in place of col; nothing else of that definition changes.
 * Refusals.  ARVX_ERR_STATE: a slab or a striped context; the source mesh does not exist; no views, or
 * no images; ARVX_MESH_COLOR_FOREGROUND when the views were set with masks == NULL; the count or
 * either download before a product; ARVX_MESH_IMAGE_COLORS in a render when the product does not exist or was computed
 * for another source.  ARVX_ERR_INVALID: an unknown source, an unknown mode, unknown flag bits, a NaN
 * or negative tolerance, a null `coloured`, a null `depth`, a view outside [0, V).  A refused call
 * leaves the previous product as it was.
 * Lifetime.  One product per context, tagged with its source: a snapshot of the mesh, the views and the
 * images at the call.  Later arvx_set_views, arvx_set_images, colour calls, carves and renders keep it.
 * It ends at the next successful arvx_mesh_color, and at any call that replaces or drops the
 * positions, faces or colours of its source: arvx_mc_mesh_welded for WELDED, SMOOTHED and DECIMATED,
 * arvx_mc_mesh_smooth for SMOOTHED, arvx_mc_mesh_decimate for DECIMATED, arvx_mc_mesh_refined for
 * REFINED.  It never ends the context's current render: its buffers are its own.
 * Device memory.  Kept with the product: 16 Vn bytes of colours and counts and the depth keys,
 * V * W * H * 8 bytes.  Workspace: the views are processed in batches, and the projected vertices of a
 * batch (16 bytes per vertex and view) take at most max(64 MiB, 16 Vn) bytes -- a batch is
 * floor(64 MiB / 16 Vn) views, one at least --; the list of a batch's (triangle, view) pairs whose pixel
 * box exceeds 64 pixels (16 bytes each; what does not fit is swept by the wave that found it, and
 * arvx_selftest_render_mesh_list bounds this list too); W * H * 4 bytes for a depth download.
 * Out of scope (per-face textures are the next block's): view weighting by surface normal, blending
 * across seams, a caller's mesh (arvx_render_triangles), near-plane clipping (the depth pass ignores
 * arvx_ctx_set_render_near: the plane is the drawing's alone), slabs and multi-GPU,
 * writing the colours back into the meshes' own vertex_rgb or the voxel colour list. */
#define ARVX_MESH_COLOR_FOREGROUND 1u /* flags of arvx_mesh_color */
#define ARVX_MESH_IMAGE_COLORS 0x100  /* OR-ed into `source` of the arvx_render_mesh family */
int arvx_mesh_color(arvx_ctx *ctx, int source, int mode, float tolerance, unsigned flags, int64_t *coloured);
int arvx_mesh_color_count(arvx_ctx *ctx, int64_t *vertices, int64_t *coloured);
int arvx_mesh_color_download(arvx_ctx *ctx, float *vertex_rgb, int32_t *views);
int arvx_mesh_color_depth_download(arvx_ctx *ctx, int view, float *depth);
/* Self-test hook: views per batch of arvx_mesh_color's depth pass from the next call on (0: the bound
 * above).  The batches change the workspace and the launches, never the product. */
int arvx_selftest_mesh_color_batch(arvx_ctx *ctx, int views_per_batch);

/* ---- mesh textures from the images (extension beyond the reference) ----------------------------
 * Builds, for a held mesh, a texture atlas with one small triangle of texels per face, each face
 * sampled from the one view that sees its three corners and shows it largest.  Definition, bit for bit
 * and without a thread order in it.  Inputs: a whole-grid context with its V views (M_v, W, H) and
 * images; a source among ARVX_MESH_WELDED, _SMOOTHED, _DECIMATED, _REFINED with its Vn positions p,
 * vertex colours col and T faces -- exactly the arrays arvx_render_mesh would draw --; a resolution R,
 * 1 <= R <= 253; an atlas width AW in texels; tol as arvx_mesh_color takes it; flags:
 * ARVX_MESH_TEXTURE_FOREGROUND, with the meaning of ARVX_MESH_COLOR_FOREGROUND.
 *  1. Layout, in integers, the same on host and device.  A cell is cw = R + 3 texels wide and
 *     ch = R + 2 high and holds two faces: face f lives in cell f >> 1, half f & 1.  The atlas has
 *     per_row = AW / cw >= 1 cells per row, rows = ceil(ceil(T / 2) / per_row) rows of cells and the
 *     height AH = rows * ch; cell k has its top-left texel at ((k % per_row) * cw, (k / per_row) * ch).
 *     A face's local texels (i, j) have i, j >= 0 and i + j <= R + 1: (R + 2)(R + 3) / 2 of them.  Half
 *     0 puts (i, j) at cell texel (i, j), half 1 at (cw - 1 - i, ch - 1 - j): the two halves tile the
 *     cell exactly.  Corners 0, 1, 2 of the face sit on the centres of local texels (0, 0), (R, 0),
 *     (0, R); the texels with i + j = R + 1 are a gutter along the hypotenuse.  The corners lie on
 *     texel centres, so the two legs need none, for nearest and for bilinear look-ups without mip
 *     levels.  Zero are: the padding columns of every atlas row where cw does not divide AW, the unused
 *     cells of the last row, and the second half of the last cell when T is odd.  The corner at atlas
 *     texel (x, y) has the UV ((float)x + 0.5f) / (float)AW, ((float)y + 0.5f) / (float)AH: row 0 is
 *     the top row, as in the images.
 *  2. Best view of face f.  View v is a candidate iff all three corners are VISIBLE in v -- step 3 of
 *     arvx_mesh_color with tol and with the foreground flag, D_v that definition's step 2 -- and the
 *     doubled area A_v of step 2 of the triangle render (int64) is not zero.  The best view is the
 *     candidate with the greatest |A_v|, among equals the least v; there is no back-face test, as in the
 *     render.  face_view[f] is that view, or -1 without a candidate.
 *  3. Texel (i, j) of a face with best view v.  b1 = i, b2 = j, b0 = R - i - j: integers, b0 = -1 in
 *     the gutter.  Per coordinate q = (float)((((double)b0 * p0 + (double)b1 * p1) + (double)b2 * p2) /
 *     (double)R) of the corners' positions.  q is projected with step 1 of the triangle render under
 *     M_v.  If it is VALID: fx is clamped to [0, 16 (W - 1)], fy to [0, 16 (H - 1)], S is step 4 of
 *     arvx_mesh_color (the integer bilinear sample) and the texel's channel is (S + 128) >> 8, stored B,
 *     G, R.  If it is not VALID, the texel is a fall-back texel.
 *  4. Fall-back texel (a face without a view, or a projection that is not VALID).  Per channel
 *     w = (float)((((double)b0 * col0 + (double)b1 * col1) + (double)b2 * col2) / (double)R), stored as
 *     the render stores a channel: (uint8_t)roundf(fminf(fmaxf(w, 0.f), 255.f)).
 *  5. Product: the atlas, AH x AW x 3 u8; face_view, T int32; face_uv, T x 3 x 2 fp32; the four numbers
 *     {T, textured faces (face_view >= 0), AW, AH}.  An empty mesh gives AH = 0 and empty arrays.
 *  6. Drawing: in arvx_render_mesh, _view and _agreement, source | ARVX_MESH_TEXTURED replaces the
 *     interpolated vertex colour of the render's step 5.  With the winner's t1, t2 and S:
 *     i = (int)floor((t1 / S) * (double)R + 0.5), j = (int)floor((t2 / S) * (double)R + 0.5), each
 *     clamped to [0, R] (i + j <= R + 1 always holds: what the gutter is for); v is the channel of the
 *     face's local texel (i, j) as a float.  The light factor and the final rounding are unchanged.
 *     ARVX_MESH_IMAGE_COLORS and ARVX_MESH_TEXTURED together are ARVX_ERR_INVALID.
 * arvx_mesh_texture takes ONE host synchronisation, for the textured count, and fills out[4] with the
 * four numbers; arvx_mesh_texture_info returns them again (host bookkeeping);
 * arvx_mesh_texture_download copies the three arrays (any pointer may be null; face_uv is computed on
 * the host from the layout).
 * Refusals.  ARVX_ERR_STATE: a slab or a striped context; the source mesh does not exist; no views, or
 * no images; ARVX_MESH_TEXTURE_FOREGROUND when the views were set with masks == NULL; info or download
 * before a product; ARVX_MESH_TEXTURED in a render when the product does not exist or was computed for
 * another source.  ARVX_ERR_INVALID: R outside [1, 253], AW outside [cw, 16384], AH above 32768, an
 * unknown source, unknown flag bits, a NaN or negative tolerance, a null `out`.  A refused call leaves
 * the previous product as it was.
 * Lifetime.  One product per context, tagged with its source: a snapshot of the mesh, the views and
 * the images at the call.  It ends at the next successful arvx_mesh_texture and wherever
 * arvx_mesh_color's product of the same source would end (that block's lifetime paragraph).  Its
 * buffers are its own: it ends neither the current render nor the mesh colours' product, and
 * arvx_mesh_color does not end it.
 * Device memory.  Kept with the product: 3 AW AH bytes of atlas and 4 T bytes of views.  Workspace:
 * depth keys of its own, V * W * H * 8 bytes (arvx_mesh_color_depth_download stays right after a
 * texture call); ceil(V / 32) words per vertex of visibility bits; the batches' projected vertices and
 * list of large boxes are arvx_mesh_color's, bounded by the same two self-test hooks.
 * Out of scope: blending across the seams between faces that chose different views, view weighting by
 * normals, mip levels, packing by projected area, charts larger than one face, a caller's mesh,
 * near-plane clipping (filling the atlas ignores arvx_ctx_set_render_near; drawing with
 * ARVX_MESH_TEXTURED honours it), slabs and multi-GPU. */
#define ARVX_MESH_TEXTURE_FOREGROUND 1u /* flags of arvx_mesh_texture */
#define ARVX_MESH_TEXTURED 0x400       /* OR-ed into `source` of the arvx_render_mesh family */
#define ARVX_MESH_TEXTURE_MAX_RESOLUTION 253
#define ARVX_MESH_TEXTURE_MAX_WIDTH 16384
#define ARVX_MESH_TEXTURE_MAX_HEIGHT 32768
int arvx_mesh_texture(arvx_ctx *ctx, int source, int resolution, int atlas_width, float tolerance, unsigned flags,
                      int64_t out[4]);
int arvx_mesh_texture_info(arvx_ctx *ctx, int64_t out[4]);
int arvx_mesh_texture_download(arvx_ctx *ctx, uint8_t *atlas_bgr, int32_t *face_view, float *face_uv);

/* Model::voxels as the reference would hold it after carve [+ colour]
 * [+ handleUnseen]: n*4 floats (RGBA), n = slab voxels. */
int arvx_export_model(arvx_ctx *ctx, float *rgba, int apply_unseen);

int arvx_get_stats(arvx_ctx *ctx, arvx_stats *out);

/* Diagnostic: which kernels the context's last arvx_carve / arvx_carve_views (or the carve inside
 * arvx_fast_carve) launched, and how much work its pre-passes handed on.  For tests that must know
 * they ran the path they meant to; synchronises, not for the hot path.
 *   out[0]  ARVX_PATH_* bits, as the host chose them (0: the context has not carved yet)
 *   out[1]  coarse tiles the carve listed for the sub-tile classification
 *   out[2]  workgroups of the dense classify kernel's launch (0: the other kernel ran)
 *   out[3]  sub-tiles queued for the exact kernel, over all work lists
 * out[1] and out[3] are 0 where the split carve did not run (ARVX_PATH_FUSED, ARVX_PATH_BRUTE_FORCE,
 * ARVX_PATH_STREAM).  They are read from the carve's work buffer, which the next carve of the
 * context reuses: call this before it. */
#define ARVX_PATH_DENSE_CLASSIFY 1u /* carve_classify_dense_kernel, not carve_classify_kernel */
#define ARVX_PATH_ITEM_SHARING 2u   /* the exact kernel may hand an item's views to several waves */
#define ARVX_PATH_FRESH 4u          /* the model was fresh: nothing read, every record written */
#define ARVX_PATH_LAZY_CODES 8u     /* decided coarse tiles were left as codes, not written */
#define ARVX_PATH_FUSED 16u         /* one kernel for rectangle tests and voxels (FUSED, > 256 views) */
#define ARVX_PATH_BRUTE_FORCE 32u   /* no rectangle tests at all (ARVX_CARVE_NO_CULL) */
#define ARVX_PATH_STREAM 64u        /* the one-launch streaming carve (-DARVX_EXPERIMENTS builds) */
#define ARVX_PATH_RECT_BLOCKS 128u  /* the exact kernel's block tests came from the table of cached rectangles */
#define ARVX_PATH_PIXEL_TABLE 256u  /* ... and the pixels of the views that fit from the table of cached pixels */
int arvx_last_carve_path(arvx_ctx *ctx, uint32_t out[4]);

/* Diagnostic: how the context's last arvx_fast_carve grew its component.  Host bookkeeping; the
 * greedy carve itself launches, copies and waits for nothing more on its account.
 *   out[0]  ARVX_FLOOD_* bits
 *   out[1]  64x16x16 tiles the whole-tile pre-pass seeded (0 without a pre-pass)
 *   out[2]  launches of the word-level step kernel, in batches of 4, 4, 8, 8, ...
 *   out[3]  rows of tiles, ceil(Y / 16) * ceil(Z / 16): the pre-pass runs up to 4096 of them
 * out[1] is counted on request from the rows the pre-pass left in the greedy carve's work buffer
 * (8 bytes per row of tiles, copied and counted on the host; synchronises).  All four are 0 before
 * the first greedy carve and after a call that replaces the state it left (carve, photo carve,
 * closure, state upload, reset). */
#define ARVX_FLOOD_PREPASS 1u /* the whole-tile pre-pass ran (at most 64 words per row, 4096 tile rows) */
#define ARVX_FLOOD_FRESH 2u   /* the model was fresh: its records were not read, all were written */
int arvx_last_fast_carve_path(arvx_ctx *ctx, uint32_t out[4]);

/* Self-test hook: evaluates the kernel's shared-reciprocal division and the IEEE
 * `/` on n host operand triples; out gets 4 floats per triple:
 * (a0/b fast, a1/b fast, a0/b IEEE, a1/b IEEE). */
int arvx_selftest_divide(arvx_ctx *ctx, int64_t n, const float *a0, const float *a1,
                         const float *b, float *out);

/* Self-test hooks for a host that has OpenCV (include/arvx/opencv_dropin.hpp runs them at first
 * use): the raw values the kernels compute for n voxels xyz (3 ints each, global coordinates).
 *   arvx_selftest_project: rows_uv = 3 n floats a0 a1 a2 -- the fp32 rows of M * toWord(x, y, z)
 *     with the context's grouping, what `intr * pose * world` holds (src/VoxelCarving.cpp:19) --
 *     followed by 2 n floats u = a0 / a2, v = a1 / a2 (:20).
 *   arvx_selftest_depth: (float)cv::norm(cameras[i] - toWord(x, y, z)) for campos = the first
 *     three components of cameras[i] (src/ColorReconstruction.h:59). */
int arvx_selftest_project(arvx_ctx *ctx, int64_t n, const float M[12], float voxel_size,
                          const int32_t *xyz, float *rows_uv);
int arvx_selftest_depth(arvx_ctx *ctx, int64_t n, const float campos[3], float voxel_size,
                        const int32_t *xyz, float *depth);

/* Self-test hook: what arvx_set_views[_device] derived for view `view` -- its background bit
 * plane (bit i of word i / 32 = pixel i is background; (W*H + 31) / 32 words) and the
 * summed-area table the rectangle tests read: (H + 1) rows of *ld two-byte entries, entry
 * [Y][X], X <= W, = foreground pixels in rows < Y and columns < X, modulo 2^16.  Either buffer may
 * be null; *ld is always set (size the table buffer after a first call with both null). */
int arvx_selftest_view_tables(arvx_ctx *ctx, int view, uint32_t *bg_bits, uint16_t *table, int *ld);

/* Self-test hook: the kernels' one-instruction pixel rounding (v_cvt_rpi_i32_f32) against
 * std::round on every float in (-0.5, 2^24], i.e. every quotient that can fall inside an
 * image; *mismatches must come back 0. */
int arvx_selftest_round(arvx_ctx *ctx, int64_t *mismatches);

/* Cached rectangles.  The rectangle arithmetic of the carve depends on the cameras, the image size
 * and the grid, not on the masks.  At the second consecutive carve of a fresh model under the same
 * matrices, V, W and H that runs the large grids' kernels (dense classify + block-mapped exact kernel
 * without item sharing: above 2^26 voxels, or the ARVX_CARVE_DENSE_CLASSIFY | ARVX_CARVE_WHOLE_ITEMS
 * path flags) the context tabulates the pixel rectangles of its 4 x 4 x 4 blocks -- 4 bytes per
 * (block, view): V / 16 bytes per voxel, 302 MB at 512^3 x 36 views -- and the exact kernel of the carves of a fresh model that follow loads them instead of computing
 * them (ARVX_PATH_RECT_BLOCKS; the results are the same bit for bit).  That one carve synchronises.
 * New matrices or sizes invalidate the table, and the second carve under the new ones builds it
 * again; a caller who carves once pays nothing.  The table is built only while it fits `bytes`
 * (default 2^30; 0: no table) and every block's pixel rectangle fits its entry.  The call releases
 * the table; it is decided again under the new limit. */
int arvx_ctx_set_rect_cache_limit(arvx_ctx *ctx, uint64_t bytes);

/* Self-test hook: recomputes every entry of the table of cached rectangles; *mismatches, the entries
 * that differ, must come back 0 (-1: the context holds no table). */
int arvx_selftest_rect_cache(arvx_ctx *ctx, int64_t *mismatches);

/* Cached pixels.  The pixel a voxel projects to in a view follows the same inputs as the block
 * rectangles above, plus the grouping of the row sums (arvx_ctx_set_projection_assoc); the masks only
 * decide which bit is found there.  Together with the table of block rectangles, and only while
 * that one stands, the context therefore tabulates the exact kernel's projection: one byte per
 * (voxel, view) -- the pixel relative to the origin of the block's rectangle, a nibble each way --,
 * 1 KB per (sub-tile record, view): 4.83 GB at 512^3 x 36 views.  The exact kernel of the carves
 * that follow reads a view's pixels instead of projecting (ARVX_PATH_PIXEL_TABLE; the results are the
 * same bit for bit).  A view with a pixel more than 15 pixels from its rectangle's origin is
 * projected as before, as is a view of a sub-tile in which a block that needs a look has no
 * rectangle (it crosses the image's edge or the camera's plane).  The table has its own limit
 * (default 6 GiB; 0: no table): 512^3 x 36 fits, 1024^3 x 36 (38.7 GB) and 512^3 x 72 do not and
 * run as before.  A failed allocation means no table, not an error.  New matrices or sizes, a new
 * limit of either table, or another grouping drop it; it is built again with (or right after) the
 * block table.  The call releases the table; it is decided again under the new limit. */
int arvx_ctx_set_pixel_cache_limit(arvx_ctx *ctx, uint64_t bytes);

/* The views whose pixels are read from the table: bit v % 64 of fits[v / 64], nwords words (all 0
 * while the context holds no table of pixels). */
int arvx_pixel_cache_views(arvx_ctx *ctx, uint64_t *fits, int nwords);

/* Self-test hook: recomputes every byte of the table of cached pixels; *mismatches, the bytes that
 * differ, must come back 0 (-1: the context holds no table). */
int arvx_selftest_pixel_cache(arvx_ctx *ctx, int64_t *mismatches);

/* View windows.  A rectangle test of the carve reads a view's summed-area table only inside the
 * pixel rectangle that the whole grid projects into (plus a margin and the table's border row and
 * column).  That rectangle follows the cameras, the image size, the voxel size and the grid -- not
 * the masks -- so arvx_set_views[_device] writes only the part of each table inside it, rounded
 * outwards to tiles of 64 x 64 entries, where it derives the views in one launch (one- or
 * three-channel masks, W a multiple of 64; every other format writes whole tables).  The window is
 * derived again when the matrices or sizes change; a view whose camera is inside or next to the grid
 * takes its whole table.  The results of every stage are what they were; the bit planes are always
 * complete.
 *   arvx_ctx_set_view_window: on = 0 makes every view take its whole table from the next
 *     arvx_set_views[_device] on (default: on).
 *   arvx_view_window: rect = {first row, last row, first column, last column} of view `view`'s table
 *     (rows 0 .. H, columns 0 .. W and the row's padding), inclusive, that the last derivation
 *     wrote.
 *   arvx_view_window_host: the same for one camera and a grid of X x Y x Z voxels, as the one-launch
 *     derivation would choose it; host arithmetic, no device and no context. */
int arvx_ctx_set_view_window(arvx_ctx *ctx, int on);
int arvx_view_window(arvx_ctx *ctx, int view, int rect[4]);
int arvx_view_window_host(int X, int Y, int Z, float voxel_size, const float M[12], int W, int H,
                          int rect[4]);

/* Self-test hooks of the view windows.  arvx_selftest_fill_view_tables sets every byte of the
 * context's table buffer to `value` and marks the views as not derived: the next
 * arvx_set_views[_device] must leave nothing of it where a carve looks.
 * arvx_selftest_view_table_raw copies view `view`'s table as it stands ((H + 1) rows of the ld that
 * arvx_selftest_view_tables reports), without writing the entries outside the window first --
 * arvx_selftest_view_tables does write them, and returns complete tables as before. */
int arvx_selftest_fill_view_tables(arvx_ctx *ctx, int value);
int arvx_selftest_view_table_raw(arvx_ctx *ctx, int view, uint16_t *table);

#ifdef __cplusplus
}
#endif
#endif
