/*
 * aof.h -- C ABI of the MI355X-native sparse SAD block-matching flow engine.
 *
 * This is the drop-in boundary for the one hot path of
 * intel-aero/aero-optical-flow: the frame-to-frame flow estimate that
 * Mainloop::camera_callback() obtains from the PX4 OpticalFlow submodule via
 *     _optical_flow->calcFlow(img, t_us, dt_us, flow_x, flow_y)
 * (/root/reference/src/mainloop.cpp:322; constructor :423-424; getters
 * :295-297; negative-return gate :327-331).  The reference binds that path as
 * a C++ class (header <flow_opencv.hpp>, /root/reference/src/mainloop.h:36);
 * the C++ facade in aero-optical-flow_amd/facade re-exports those classes on
 * top of this ABI, and INTEGRATION.md shows the CMake hook that replaces
 * modules/OpticalFlow (/root/reference/CMakeLists.txt:10,17).
 *
 * Conventions: plain C types, caller owns every buffer, no exceptions cross
 * the boundary.  Functions return 0 on success or a negative errno-style code;
 * aof_last_error() gives the text.  A context is thread-compatible (one
 * caller at a time), which is what the reference guarantees: calcFlow is only
 * called under _mainloop_lock (/root/reference/src/mainloop.cpp:283).
 *
 * There is NO CPU fallback: every entry point that computes flow runs the HIP
 * kernels on a gfx950 device and fails (-ENODEV) when none is present.
 */
#ifndef AOF_H
#define AOF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: these are its exports */
#endif

#define AOF_VERSION 102 /* 0.1.2: ADAPTIVE is the default search mode of 8x8 contexts too, aof_search_stats */

#define AOF_GRID_DENSE 0   /* origin = margin, step = tile */
#define AOF_GRID_PX4FLOW 1 /* published sparse grid: num_blocks tiles per axis */

/* Algorithm parameters (DESIGN.md "Spec").  aof_params_default() gives the
 * configuration BASELINE.json quotes the metric on. */
typedef struct aof_params {
    int32_t width, height;     /* level-0 frame, 8-bit grey, row stride == width
                                  (the caller makes it contiguous, mainloop.cpp:317-320) */
    int32_t tile;              /* B: 8 or 16 */
    int32_t search;            /* S: 1..8 */
    int32_t grid_mode;         /* AOF_GRID_* */
    int32_t num_blocks;        /* AOF_GRID_PX4FLOW only */
    int32_t feature_threshold; /* 4x4 gradient gate */
    int32_t value_threshold;   /* SAD acceptance gate */
    int32_t subpixel;          /* half-pixel refinement */
    int32_t hist_filter;       /* 1: histogram peak filter, 0: plain average */
    int32_t pyramid_levels;    /* 1 or 2 */
    int32_t mean_subtract;     /* equalise cur to prev frame mean per level */
    int32_t min_valid;         /* flow valid iff accepted blocks > min_valid */
} aof_params;

/* Per-block record, 4 bytes: integer shift of the best match and its SAD.
 * sad == 0xFFFF marks a skipped block (gradient gate / window outside frame). */
typedef struct aof_block {
    int8_t dx, dy;
    uint16_t sad;
} aof_block;

#define AOF_SAD_SKIPPED 0xFFFFu
#define AOF_FLAG_FLOW_VALID 1u
#define AOF_FLAG_PRED_VALID 2u

/* Per-pair result, 16 bytes. */
typedef struct aof_flow {
    float flow_x, flow_y; /* level-0 pixels */
    uint32_t count;       /* accepted blocks */
    uint8_t quality;      /* count*255/blocks, 0 when flow invalid (mainloop.cpp:371) */
    uint8_t flags;        /* AOF_FLAG_* */
    int8_t pred_x, pred_y;/* level-1 predictor, level-0 pixels */
} aof_flow;

/* Byte offsets of the intermediates inside the caller's workspace (tests and
 * tools read them; the layout is fixed by aof_workspace_layout()). */
typedef struct aof_ws_layout {
    size_t total_bytes;
    size_t sums;      /* uint32 [n_pairs][2 frames: prev,cur][2 levels] pixel sums */
    size_t l1_prev;   /* u8 [n_pairs][h/2][w/2] */
    size_t l1_cur;    /* u8 [n_pairs][h/2][w/2] */
    size_t l1_blocks; /* aof_block [n_pairs][nb1] */
    size_t l1_subdirs;/* u8 [n_pairs][nb1] */
    size_t l1_flows;  /* aof_flow [n_pairs] (pred_x/pred_y = predictor) */
    size_t l0_blocks; /* aof_block [n_pairs][nb0] when the caller passes none */
    size_t l0_subdirs;/* u8 [n_pairs][nb0] when the caller passes none */
    size_t l0_hist;   /* u32 [n_pairs][chunks0][2][bins0]: per-chunk vote histograms (grids beyond 8 192 blocks) */
    size_t l1_hist;   /* u32 [n_pairs][chunks1][2][bins1] */
    size_t hints;     /* u32 [n_pairs], 16x16 tiles: the adaptive search's per-pair verdict low byte (0 = exhaustive scan; 1 / 2 / 3 / 4 = pruning pays, on two- / one- / four- / eight-row bounds), a diagnostic above it */
} aof_ws_layout;

typedef struct aof_ctx aof_ctx;

/* Kernel ids for aof_kernel_ms(). */
#define AOF_K_PYRAMID 0 /* K1: frame sums + 2x2 pyramid */
#define AOF_K_SEARCH_L1 1
#define AOF_K_REDUCE_L1 2
#define AOF_K_SEARCH 3  /* K2: SAD search, level 0 -- the dominant kernel */
#define AOF_K_REDUCE 4  /* K3: histogram-filtered flow reduction */
#define AOF_K_COUNT 5

int aof_version(void);
const char *aof_strerror(int code);

/* ---- parameters (host only, no GPU needed) ---- */
int aof_params_default(aof_params *p, int width, int height);
/* Published PX4Flow configuration: sparse grid, half-pixel refinement. */
int aof_params_px4flow(aof_params *p, int width, int height, int search,
                       int feature_threshold, int value_threshold);
int aof_params_check(const aof_params *p);
/* Block grid of a pyramid level: origin, step, counts. */
int aof_grid(const aof_params *p, int level, int32_t *x0, int32_t *y0, int32_t *step_x,
             int32_t *step_y, int32_t *nx, int32_t *ny);
int aof_workspace_layout(const aof_params *p, int64_t n_pairs, aof_ws_layout *out);

/* ---- context ---- */
/* device: HIP device ordinal.  Fails with -ENODEV when no gfx950 GPU is usable. */
int aof_create(const aof_params *p, int device, aof_ctx **out);
void aof_destroy(aof_ctx *ctx);
const char *aof_last_error(const aof_ctx *ctx);
int aof_get_params(const aof_ctx *ctx, aof_params *out);
/* Name of the search kernel variant the context selected ("lane8", "tile16_lds", "generic"). */
const char *aof_search_variant(const aof_ctx *ctx);
/* Force the generic search kernel (tests compare the two device paths). */
int aof_set_force_generic(aof_ctx *ctx, int on);
/* Search strategy.  All return bit-identical records.
 * EXHAUSTIVE: all candidates of every block are summed completely -- a data-independent rate.
 * PRUNED: exact partial-distortion elimination (8x8 tiles on grids of more than 256 blocks, and
 *   16x16 tiles).  The dy rows are visited outwards from dy = 0; after a few of a row's tile rows a
 *   wave drops the row when no lane's partial SAD can still beat its best (a partial sum only grows).
 *   The rate then depends on the images: fast when blocks have a clear match near the centre, slower
 *   than the exhaustive search on noise (16x16: up to 1.5x; the 8x8 kernel falls back per wave).
 * ADAPTIVE (the default): PRUNED where it pays.
 *   16x16 tiles: a small probe kernel in front of the search computes the two-row bounds of a sample of every
 *   pair's blocks (1.6 % of them) and the search runs a pair's block rows pruned when the bounds predict that few
 *   candidates survive, exhaustively otherwise (the verdicts live in the workspace, aof_ws_layout.hints).
 *   8x8 tiles (level-0 searches of at least 2 048 x 256 blocks per launch -- 112 VGA pairs --; everything else runs
 *   EXHAUSTIVE): a probe per launch would cost more than it saves, so the CONTEXT learns from its own launches.  The
 *   pruned kernel -- whose waves run a block exhaustively, judge from its SADs whether rows could have been dropped,
 *   and prune the next blocks where they could -- reports the share of blocks that pruned (plain stores into pinned
 *   host memory, read at the next enqueue, never waited for).  While that share is at least 40 % the context keeps
 *   launching it, and its waves prune from their FIRST block on (which votes for the dy row to start in; round 5) --
 *   1 024 VGA pairs per launch, same box (profiles/r05_final_c2_noise.txt): noise-free translations 1.6-1.85x EXHAUSTIVE, +-2 LSB
 *   of noise 1.5x, +-4 LSB 1.4x, +-8 LSB 1.2x --; otherwise it launches the exhaustive kernel, and the pruned one once in 16
 *   launches to look again (+-16 LSB and more: within 1 % of EXHAUSTIVE, where PRUNED alone loses 12 %).  A context's
 *   first launch and a graph captured from it use whatever is known at that moment (aof_set_search_belief tells a fresh
 *   context); half-pixel configurations prune too.  aof_get_search_stats tells what happened. */
#define AOF_SEARCH_EXHAUSTIVE 0
#define AOF_SEARCH_PRUNED 1
#define AOF_SEARCH_ADAPTIVE 2
int aof_set_search_mode(aof_ctx *ctx, int mode);
int aof_get_search_mode(const aof_ctx *ctx);
/* What the ADAPTIVE mode of an 8x8 context has done so far (diagnostics; tests assert on them). */
typedef struct aof_search_stats {
    uint64_t pruned_launches;     /* flat 8x8 searches run by the pruned kernel (it reports back) */
    uint64_t exhaustive_launches; /* ... by the exhaustive kernel because the reports said pruning does not pay */
    uint64_t reports_read;        /* launches' reports evaluated */
    int32_t belief;               /* -1 nothing known yet, 0 pruning does not pay on this context's images, 1 it does */
    int32_t paying_pct;           /* share of the last report's chunks that left with "pruning pays" */
} aof_search_stats;
int aof_get_search_stats(const aof_ctx *ctx, aof_search_stats *out);
/* What an ADAPTIVE 8x8 context believes about its images is learnt from its own launches, so a context that lives for
 * ONE batch never uses it: its first launch lets every wave judge its first block exhaustively (6-10 % slower than either
 * dedicated kernel).  Callers that know their footage -- from aof_get_search_stats of an earlier context over the same
 * camera, or from the sensor -- say so here: 1 = pruning pays (launches prune from the first block on), 0 = it does not
 * (the exhaustive kernel, with one pruned launch in 16 to look again), -1 = forget (judge again).  The context keeps
 * learning from its launches afterwards.  Speed only: the records are the same.  The better cure is to create a
 * context once and reuse it ("Batch callers"). */
int aof_set_search_belief(aof_ctx *ctx, int belief);

/* ---- the hot path, device-resident (batched) ----
 * d_prev/d_cur: device pointers, pair i at +i*pair_stride bytes, each frame
 * width*height bytes.  For a frame SEQUENCE pass d_cur = d_prev + width*height
 * and pair_stride = width*height: frame k is cur of pair k-1 and prev of pair k, and
 * the passes that work per frame (pixel sums, 2x2 pyramid) then run once per FRAME
 * (the workspace's level-1 frames, where the separate kernels write them, are then
 * n_pairs + 1 consecutive frames from offset l1_prev on).
 * d_blocks: [n_pairs][nb0] records (4-byte aligned) or NULL.  d_subdirs: [n_pairs][nb0] or NULL.
 * d_flows: [n_pairs], required.  d_workspace: >= aof_workspace_layout().total_bytes,
 * 256-byte aligned.  stream: hipStream_t (NULL = default stream).
 * Asynchronous: returns after enqueueing; no allocation, no host sync.
 * Calls of at most 128 small pairs (8x8 tiles, every grid 8..256 blocks, width a multiple of 16,
 * frames that fit LDS: the published sparse grid up to about 256x224) run as ONE kernel, a
 * workgroup per pair, whatever the number of levels; the workspace's level-1 frames then stay
 * untouched (aof_set_split_coarse(ctx, 1) selects the separate kernels instead). */
int aof_flow_batch_device(aof_ctx *ctx, const uint8_t *d_prev, const uint8_t *d_cur,
                          int64_t pair_stride, int64_t n_pairs, aof_block *d_blocks,
                          uint8_t *d_subdirs, aof_flow *d_flows, void *d_workspace,
                          size_t workspace_bytes, void *stream);

/* Two-level configurations of 8x8 tiles whose two level-1 frames fit one CU's LDS (VGA: 150 KB)
 * run their coarse passes -- pixel sums, 2x2 pyramid, level-1 search, level-1 reduction -- as
 * ONE kernel, a workgroup per pair, and never write the level-1 frames to memory (the
 * workspace regions l1_prev / l1_cur then stay untouched).  on = 1 runs them as the separate
 * kernels K1 / K2 / K3 instead, which also fills l1_prev / l1_cur (tests compare the two), and
 * keeps small batches (see aof_flow_batch_device) on the separate kernels as well. */
int aof_set_split_coarse(aof_ctx *ctx, int on);

/* 8x8 tiles on grids of more than 256 blocks (C2, C3): the search kernel also reduces -- every wave adds
 * its votes to the pair's record in the CONTEXT's vote memory with integer atomics and the last wave
 * of a pair writes its aof_flow -- so no K3 launch follows (at 128 VGA pairs per call, configs[3]'s
 * per-GPU share, K3 and its launch gap were a quarter of the step).  Integer adds commute: the records
 * are bit-identical to the separate K3's.  Because the vote memory belongs to the context, calls on
 * ONE context must not overlap on the device: eager calls on different streams are ordered behind each
 * other by the library; captured graphs that contain calls on a context must not be replayed
 * concurrently with each other or with eager calls on it (once such a graph has been captured, the
 * library's own eager calls on the context keep to the separate K3).  Both forms of the search have it: the exhaustive
 * scan (k_flow_lane8_flat) and, on dense grids, the pruned column walk (k_flow_lane8_cols, which adds the agreeing votes of
 * a walk once); launches that prune on other grids keep K3.  Launches of more than 2 048 pairs
 * keep K3 as well.
 * on = 0 (THE DEFAULT): K3 runs as a separate kernel behind the search.  on = 1: opt in.
 * A finaliser wave that does not see its pair's votes complete within the deadline (50 ms; a launch in which
 * that happens is broken) writes that pair's record as "nothing measured" -- flow 0, count 0, quality 0,
 * flags 0 -- and raises the context's fault word: every later aof_flow_batch_device / aof_flow_pair_host /
 * aof_stream_push_host on the context returns -EIO (aof_last_error names the pair).  The condition is
 * sticky, like a HIP fault: recover with a new context. */
int aof_set_reduce_fusion(aof_ctx *ctx, int on);
/* Diagnostic knob: the finaliser deadline above, in microseconds (default 50 000; at least 100, -EINVAL below:
 * a deadline no launch can meet would disable the context with one call). */
int aof_set_vote_deadline_us(aof_ctx *ctx, uint32_t microseconds);
/* Fault injection for the tests of that path: the deadline in ticks of the 100 MHz counter, unchecked (0 = every
 * finaliser gives up at once -> zero records, sticky -EIO). */
int aof_debug_vote_deadline_ticks(aof_ctx *ctx, uint32_t ticks);
/* Test hook of the 16x16 adaptive search: no probe runs; pair i gets verdicts[i % count] (each 0..4, as in
 * aof_ws_layout.hints), at both levels.  count = 0 gives the decision back to the probe.  Records do not depend on
 * the verdict.  -EINVAL: NULL ctx, a context whose tile is not 16, count < 0 or > 8, NULL verdicts with count > 0,
 * a verdict above 4. */
int aof_debug_tile16_verdicts(aof_ctx *ctx, const uint8_t *verdicts, int count);

/* ---- host-buffer conveniences (what the C++ facade calls) ----
 * Synchronous: copy in, run the kernels above, copy out.  blocks/subdirs may be NULL. */
int aof_flow_pair_host(aof_ctx *ctx, const uint8_t *prev, const uint8_t *cur, aof_block *blocks,
                       uint8_t *subdirs, aof_flow *flow);
/* Streaming: the context keeps the previous frame on the device.  Returns 1 for
 * the first frame after create/reset (nothing to compare, *flow zeroed), 0 afterwards. */
int aof_stream_push_host(aof_ctx *ctx, const uint8_t *frame, aof_flow *flow);
int aof_stream_reset(aof_ctx *ctx);
/* Opt-in resident form of the streaming entry point for small frames (the one-workgroup kernel's class:
 * 8x8 tiles, grids of 8..256 blocks, frames of at most 64 KB).  Most of the 14 us a call takes through a
 * replayed hipGraph is the launch; with on = 1 ONE workgroup stays on the device
 * between calls, polls a request word in pinned host memory, computes the pair exactly as the one-launch
 * kernel does and posts the 16-byte record and a completion word the host polls -- no launch per frame.
 * The kernel always ends by itself: after 50 ms without a request, after 200 ms in total (so nothing that
 * waits for the device to drain, e.g. a hipFree elsewhere in the process, waits longer), or when the
 * library stops it (aof_destroy, aof_set_*, this call with on = 0); the next call starts it again.  It runs
 * on a stream of its own at the highest stream priority, i.e. on a hardware queue that no normal-priority
 * stream of the process shares.
 * Every host-side wait of this path is bounded.  A request that is not answered within 250 ms of the
 * launch call's return (or of the request, when the kernel was already there) switches the mode off for the
 * context: the kernel is asked to leave and the call, like all later ones, takes the graph path (one line on
 * stderr, aof_stream_stats.resident_fallbacks, .last_report).  A kernel that does not leave within a second
 * either keeps its pinned buffers for good (they are leaked, the context continues on fresh ones and the call
 * returns 1 like the first call of a sequence; aof_destroy then frees no device memory at all).
 * Results are bit-identical in both forms.  on < 0 queries whether the kernel is on the device now. */
int aof_set_stream_resident(aof_ctx *ctx, int on);
/* Counters of the streaming entry point since aof_create (diagnostics; tests assert on them). */
typedef struct aof_stream_stats {
    uint64_t calls;              /* aof_stream_push_host calls that had a previous frame to compare with */
    uint64_t resident_served;    /* ... of them answered by the resident kernel */
    uint32_t resident_launches;  /* resident kernel instances started */
    uint32_t resident_fallbacks; /* requests it did not answer within 250 ms (resident mode switched off) */
    uint32_t resident_lost;      /* instances that did not leave within 1 s of being asked (buffers abandoned) */
    uint32_t tagged_slow;        /* graph path: tagged record not there within 2 ms (the stream was drained instead) */
    float launch_call_us_max;    /* longest hipLaunchKernelGGL call of a resident start (the first loads the code object) */
    float start_latency_us_max;  /* longest launch-return -> first-poll latency of a resident kernel, the host only
                                    spinning on pinned memory in between (no HIP call) */
    char last_report[320];       /* text of the last fallback report, "" if none */
} aof_stream_stats;
int aof_stream_get_stats(const aof_ctx *ctx, aof_stream_stats *out);
/* Fault injection for tests of the path above: resident kernel instances started from now on ignore the request to
 * leave (deaf = 1; they still go on their own 50 ms / 200 ms deadlines), and the library waits stop_wait_us for a
 * kernel to leave instead of one second (0 = the default).  Exercises the "kernel lost" branch: buffers abandoned,
 * the context continues on fresh ones, aof_destroy leaks instead of freeing. */
int aof_debug_resident_fault(aof_ctx *ctx, int deaf, uint32_t stop_wait_us);
/* The streaming entry point replays a captured hipGraph per call (H2D frame, kernels, the result
 * written into pinned host memory; for frames of at most 64 KB served by the one-workgroup kernel:
 * that ONE kernel reading the pinned frames in place and publishing the record with a tag the host
 * polls for, without waiting for the stream); this switches the capture off (1 = on, the default:
 * eager launches and a stream wait otherwise).  Returns whether a graph is currently instantiated
 * for the next call when on < 0 (query). */
int aof_set_stream_graph(aof_ctx *ctx, int on);

/* ---- frame ingest: the caller-side steps the reference runs on
 * the host right before calcFlow, moved next to the data so a full sensor frame is
 * uploaded once: centre crop to the engine's frame size with a contiguous copy
 * (/root/reference/src/mainloop.cpp:295-298,317-319) and the 10-bin histogram of the
 * centred 128x128 region of the cropped image that feeds the auto-exposure loop
 * (mainloop.cpp:203-214; EXPOSURE_MASK_SIZE :52).  Stateless. ---- */
#define AOF_EXPOSURE_BINS 10
#define AOF_EXPOSURE_MASK_SIZE 128
typedef struct aof_ingest_params {
    int32_t camera_width, camera_height; /* Y plane of the sensor frame, stride == width */
    int32_t crop_width, crop_height;     /* engine frame size (getImageWidth/Height) */
} aof_ingest_params;
/* d_camera: frame i at +i*camera_stride bytes.  d_cropped: [n][crop_h][crop_w], frame i at
 * +i*cropped_stride (pass it on to aof_flow_batch_device).  d_hist: uint32 [n][10] or NULL.
 * Either output may be NULL.  Asynchronous on `stream`. */
int aof_ingest_batch_device(const aof_ingest_params *p, const uint8_t *d_camera,
                            int64_t camera_stride, int64_t n_frames, uint8_t *d_cropped,
                            int64_t cropped_stride, uint32_t *d_hist, void *stream);
/* Mean sample value of one histogram, exactly as mainloop.cpp:216-220 computes it. */
float aof_exposure_msv(const uint32_t hist[AOF_EXPOSURE_BINS]);
/* Histogram bin (0..9) of a grey value, -1 if cv::calcHist would drop it (v == 255). */
int aof_exposure_bin(int grey);

/* ---- gyro de-rotation: the output-side neighbour of the path.
 * The reference integrates the gyro between flow outputs and ships it next to the flow
 * for the autopilot to de-rotate (/root/reference/src/mainloop.cpp:383-405, axis swap
 * :364-365: "-y gives x flow, x gives y flow").  This applies the published PX4Flow
 * compensation to a batch of flow records on the device:
 *   if |gy| > threshold*dt:  x' = clamp(flow_x + gy*focal_x, +-max_flow)   else x' = flow_x
 *   if |gx| > threshold*dt:  y' = clamp(flow_y - gx*focal_y, +-max_flow)   else y' = flow_y
 * with gx, gy the gyro angles (rad) integrated over the pair's interval dt (s). ---- */
typedef struct aof_gyro {
    float integ_x, integ_y, integ_z; /* rad, body rates integrated over the frame interval */
    float dt_s;                      /* the interval */
} aof_gyro;
typedef struct aof_derotate_params {
    float focal_x, focal_y;  /* px (main.cpp:60-61) */
    float max_flow;          /* clamp: search radius + 0.5 px */
    float rate_threshold;    /* rad/s below which an axis is left alone */
} aof_derotate_params;
/* d_out: float [n][2] compensated pixel flow.  Asynchronous on `stream`. */
int aof_derotate_batch_device(const aof_derotate_params *p, const aof_flow *d_flows,
                              const aof_gyro *d_gyro, int64_t n, float *d_out, void *stream);

/* ---- a recorded frame SEQUENCE as one device pipeline (the reference's per-frame loop,
 * /root/reference/src/mainloop.cpp:295-373, for all frames of a recording at once) ----
 * n sensor frames, their time stamps and the gyro integrated between them, all resident in device memory, go
 * through, in ONE call that only enqueues (no allocation, no host synchronisation: it can be captured):
 *   1. ingest: centre crop + exposure histogram per frame (aof_ingest_batch_device; mainloop.cpp:295-298,203-214)
 *   2. flow in sequence mode: frame k is `cur` of pair k-1 and `prev` of pair k (aof_flow_batch_device)
 *   3. the rate limiter of calcFlow (flows of frames with quality > 0 summed until
 *      (float)(t - t_last) > 1e6f / output_rate, u32 wrap-around arithmetic; mainloop.cpp:322-331)
 *   4. gyro de-rotation of every pair's pixel flow (aof_derotate_batch_device; an extra output: the message
 *      itself carries the flow and the gyro side by side, as the reference sends them)
 *   5. pixel flow -> angular flow (aof_flow_angle), the OPTICAL_FLOW_RAD field mapping (mainloop.cpp:359-371)
 *      and the MAVLink 2 frame (mavlink_tcp.cpp:142-162) of every published flow.
 * The records and frames are byte-identical to driving the C++ facade frame by frame over the same frames
 * (OpticalFlowOpenCV::calcFlow + fillOpticalFlowRad + packOpticalFlowRad): the float operations are the
 * host's, in the host's order.  The context's parameters must describe the CROPPED frame. */
typedef struct aof_sequence_params {
    aof_ingest_params ingest;        /* sensor frame -> crop; crop size == the context's frame size */
    float focal_x, focal_y;          /* px (main.cpp:60-61) */
    int32_t output_rate;             /* Hz (main.cpp:59); <= 0 publishes every frame */
    uint64_t offset_timestamp_usec;  /* vehicle time of the first frame (mainloop.cpp:360); 0 = not known yet:
                                        records are written, no frame is sent (mainloop.cpp:353-357) */
    uint8_t system_id, component_id; /* MAVLink ids (mavlink_tcp.h:66-67: 1, MAV_COMP_ID_CAMERA = 100) */
    uint8_t first_seq;               /* MAVLink sequence number of the first frame sent */
    uint8_t derotate;                /* 1: also write the de-rotated pixel flow of every pair */
    aof_derotate_params derotate_params;
} aof_sequence_params;

/* What calcFlow returned for a frame it published (quality >= 0), plus the gyro taken with it. */
typedef struct aof_seq_record {
    uint32_t frame;          /* index of the frame */
    int32_t quality;         /* 0..255 */
    int32_t dt_us;           /* integration time */
    float flow_x, flow_y;    /* rad */
    float gyro_x, gyro_y, gyro_z; /* rad, integrated since the previous record (before the axis switch) */
} aof_seq_record;

#define AOF_SEQ_FRAME_BYTES 56     /* room per MAVLink 2 frame: 10 + 44 + 2 */
#define AOF_SEQ_STATUS_STALLED 1u  /* the CHAIN of publications ended with frames left: none of the 4096 frames behind its
                                      last publication (behind the start, where nothing was published) reaches the
                                      output period and the recording goes on beyond them -- the time stamps do not
                                      advance; nothing is published behind that point.  Frames that are not published
                                      never raise it, whatever lies behind them */

/* Byte offsets of the pipeline's outputs and intermediates inside the caller's workspace. */
typedef struct aof_seq_layout {
    size_t total_bytes;
    size_t cropped;    /* u8 [n][crop_h][crop_w]: the frame sequence the flow runs on */
    size_t exposure;   /* u32 [n][10]: exposure histograms */
    size_t flows;      /* aof_flow [n-1]: pair k = frames k, k+1 */
    size_t derotated;  /* float [n-1][2] (params.derotate) */
    size_t count;      /* u32 [4]: records written, frames sent, AOF_SEQ_STATUS_* flags, 0 */
    size_t records;    /* aof_seq_record [n], the first count[0] valid, in frame order */
    size_t frames;     /* u8 [n][AOF_SEQ_FRAME_BYTES]: frame of record m at + 56 m */
    size_t frame_len;  /* u8 [n]: length of frame m (0: not sent) */
    size_t scratch;    /* limiter state and the flow engine's workspace */
} aof_seq_layout;
int aof_sequence_layout(const aof_params *p, const aof_sequence_params *sp, int64_t n_frames, aof_seq_layout *out);
/* d_camera: frame i at + i*camera_stride.  d_time_us: [n] frame times in microseconds relative to the first
 * frame (mainloop.cpp:305-311; calcFlow sees them truncated to 32 bits).  d_gyro: [n], entry k = gyro integrated
 * over the interval that ends at frame k (dt_s: that interval, for the de-rotation), or NULL (zeros).
 * d_workspace: >= aof_sequence_layout().total_bytes, 256-byte aligned. */
int aof_sequence_device(aof_ctx *ctx, const aof_sequence_params *sp, const uint8_t *d_camera, int64_t camera_stride,
                        int64_t n_frames, const uint64_t *d_time_us, const aof_gyro *d_gyro, void *d_workspace,
                        size_t workspace_bytes, void *stream);
/* Pixel flow -> angular flow (rad) exactly as the facade and the device pipeline compute it:
 * atan2(flow_px, focal_px) as a fixed sequence of IEEE double operations (include/aof_math.h).  Host only. */
float aof_flow_angle(float flow_px, float focal_px);

/* ---- a bank of live streams: many cameras per tick from one device launch ----
 * A stream bank is device memory, owned by the caller, that holds for each of S independent live streams what one
 * facade object holds on the host: the previous frame, the rate limiter's sums, the time of the last publication, the
 * gyro sums and the MAVLink sequence number.  One aof_bank_push_device call per tick takes the newest frame of every
 * stream that has one and leaves, per stream, exactly what OpticalFlow::calcFlow() + the reference's message code
 * would have produced for that frame (facade/src/optical_flow.cpp integrate() / limitRate(), mainloop.cpp:322-373):
 *   * a stream's first frame after a reset is stored; its record has quality 0, dt_us 0, flow 0, the tick's gyro
 *     (taken and zeroed) and an all-zero pixel record; the time of the last publication stays 0 (this is what
 *     aof_sequence_device writes for frame 0 and what mainloop.cpp sends after calcFlow() returned 0);
 *   * otherwise: the pixel flow of (stored frame, new frame) -- the aof_flow bytes aof_flow_batch_device gives for that
 *     pair --, then limitRate() on the stream's state, then aof_flow_angle; the new frame replaces the stored one.
 *     Gyro increments are added as doubles every active tick, and taken (cast to float) and zeroed with every record
 *     whose quality is >= 0;
 *   * with d_mavlink and a non-zero offset_timestamp_usec every record with quality >= 0 gets its MAVLink 2
 *     OPTICAL_FLOW_RAD frame (time_usec = offset + t, per-stream sequence number counting from first_seq),
 *     byte-identical to fillOpticalFlowRad + packOpticalFlowRad;
 *   * a stream without a frame in the tick gets AOF_TICK_IDLE and an otherwise zero record; its bank bytes (frame and
 *     state) are not written.
 * Both calls only enqueue: no allocation, no host synchronisation, capturable into a hipGraph.  Small configurations
 * (8x8 tiles, +-4, grids of 8..256 blocks per level, width a multiple of 16, frames that fit LDS: the PX4 64x64 and
 * the OpticalFlowOpenCV 128x128 two-level configurations among them) run a tick as ONE kernel, a workgroup per
 * stream; every other configuration, and banks of more streams than that pays for, run aof_flow_batch_device's plan on
 * (bank frames, tick frames) followed by one commit kernel.  The bytes are the same either way.
 * Calls on one context and one bank must not overlap on the device (the bank is read and written in place, and the
 * context's vote memory may serve the flow): keep them on one stream, or order them with events. */
typedef struct aof_bank_params {
    int32_t n_streams;               /* S >= 1 */
    int64_t frame_stride;            /* bytes between the frames of consecutive streams, in the bank AND in the
                                        caller's tick buffer; 0 = width*height; >= width*height, multiple of 16 */
    float focal_x, focal_y;          /* px */
    int32_t output_rate;             /* Hz; <= 0 publishes every frame */
    uint64_t offset_timestamp_usec;  /* 0: records only, no frame is sent (mainloop.cpp:353-357) */
    uint8_t system_id, component_id, first_seq;
} aof_bank_params;

#define AOF_TICK_HELD (-1)   /* calcFlow returned -1: still integrating */
#define AOF_TICK_IDLE (-2)   /* the stream had no frame in this tick: nothing about it changed */
typedef struct aof_tick_record {     /* 48 bytes, one per stream and tick */
    int32_t quality;                 /* >= 0: published (what calcFlow returned), or AOF_TICK_HELD / AOF_TICK_IDLE */
    int32_t dt_us;                   /* integration time of a published record, else 0 */
    float flow_x, flow_y;            /* rad (aof_flow_angle) of a published record, else 0 */
    float gyro_x, gyro_y, gyro_z;    /* rad, summed since the stream's previous publication, before the axis switch
                                        (published records; else 0) */
    uint32_t frame;                  /* frames this stream has been given, this one included (0 for idle streams) */
    aof_flow pixel;                  /* this tick's pair record (all zero for a stream's first frame and for idle streams) */
} aof_tick_record;

/* Byte offsets of the regions of a bank.  (A struct tag only: C has one name space for typedefs and functions, and the
 * function below carries the name.  Write `struct aof_bank_layout`.) */
struct aof_bank_layout {
    size_t total_bytes;
    size_t frames;   /* u8 [S][frame_stride]: the stored frame of every stream */
    size_t state;    /* one 64-byte record per stream (limiter, gyro sums, counters) */
    size_t scratch;  /* the flow engine's workspace for S pairs and aof_flow [S] */
};
int aof_bank_layout(const aof_params *p, const aof_bank_params *bp, struct aof_bank_layout *out);   /* host only */
/* d_mask: u8 [S] or NULL (= all).  Masked streams go back to "no previous frame", limiter and gyro sums zero,
 * time of the last publication 0, sequence number first_seq, frame counter 0.  A new bank must be reset once.
 * d_bank: >= aof_bank_layout().total_bytes, 256-byte aligned. */
int aof_bank_reset_device(aof_ctx *ctx, const aof_bank_params *bp, const uint8_t *d_mask, void *d_bank,
                          size_t bank_bytes, void *stream);
/* d_frames: stream s at + s*frame_stride.  d_time_us: u64 [S], the limiter sees (uint32_t)t.  d_active: u8 [S] or
 * NULL (= all).  d_gyro: aof_gyro [S] (integrated over the interval that ends at this frame) or NULL (zeros).
 * d_records: aof_tick_record [S].  d_mavlink: u8 [S][AOF_SEQ_FRAME_BYTES] or NULL; d_mavlink_len: u8 [S]
 * (0 = nothing sent), required with d_mavlink.
 * -EINVAL: NULL ctx / params / bank / frames / times / records, n_streams < 1, a bad frame_stride or focal length, a
 * bank that is not 256-byte aligned, d_mavlink without its lengths; -ENOSPC: a bank smaller than its layout; -EIO: the
 * context's sticky fault.  A refused call leaves the bank untouched. */
int aof_bank_push_device(aof_ctx *ctx, const aof_bank_params *bp, const uint8_t *d_frames, const uint64_t *d_time_us,
                         const uint8_t *d_active, const aof_gyro *d_gyro, void *d_bank, size_t bank_bytes,
                         aof_tick_record *d_records, uint8_t *d_mavlink, uint8_t *d_mavlink_len, void *stream);
/* 0 = the library chooses (default), 1 = always the one-launch kernel where the configuration allows it (elsewhere
 * the composed path, not an error), 2 = always the composed path.  Identical bytes either way (tests compare them).
 * -EINVAL: NULL ctx, path outside 0..2. */
int aof_set_bank_path(aof_ctx *ctx, int path);
/* Host only: which path the most recent ACCEPTED push of this context took, whichever of the four push forms it was:
 * 0 = no push yet, 1 = one-launch kernel(s), 2 = the composed launches.  A refused push leaves it as it was.
 * -EINVAL: NULL ctx. */
int aof_bank_last_path(const aof_ctx *ctx);

/* ---- the stream bank with per-stream cameras: focal lengths, output rate, vehicle time and MAVLink identity ----
 * aof_bank_params carries ONE focal length pair, output rate, time offset and MAVLink identity for all S streams: S
 * cameras built with identical arguments.  Real cameras differ in exactly these (the reference takes them per process
 * from its command line), so a caller may bind an array of S records in device memory to the context; while it is
 * bound, stream s of every push takes these six values from record s instead of from aof_bank_params:
 *   * period of the rate limiter: 1.0e6f / (float)output_rate, one correctly rounded float division -- the float the
 *     host computes for aof_bank_params.output_rate; output_rate <= 0 publishes every frame;
 *   * angles: aof_flow_angle(pixel flow, the stream's focal length);
 *   * a frame is packed iff d_mavlink is given and the stream's offset_timestamp_usec is non-zero, with the stream's
 *     system_id and component_id and the sequence number (uint8_t)(first_seq + messages);
 *   * a changed output_rate leaves the limiter's sums as they stand: the new period applies from that tick on.
 * The four pushes (aof_bank_push_device, _camera_device, _burst_device, _camera_burst_device) use the array when
 * bp->n_streams equals the bound count; aof_bank_imu_device with ip->n_streams equal to it takes system_id,
 * component_id and first_seq of stream s from the array (its time offsets are per stream already, in aof_imu_state).
 * The scalars of bp / ip are still checked as without a binding and are otherwise ignored.  A push or IMU call whose
 * stream count differs from the bound one returns -EINVAL and writes nothing.
 * The KERNELS read the array, when they run: the caller may rewrite records between ticks in stream order, and a
 * captured graph replays against whatever the array holds at replay.  The host cannot see device data: the values are
 * used as they are (a focal length that is not > 0 gives whatever aof_flow_angle gives for it).  A burst indexes the
 * array by the stream's number alone, in every round.
 * Contract: stream s's records, frames, lengths, stored frame and state are byte-identical to what a bank of ONE stream
 * produces for the same inputs when its aof_bank_params carries record s's values; and if all S records equal
 * aof_bank_stream_from_params(bp), every output and the whole bank are byte-identical to the unbound call.
 * Not per stream, and as they were: the exposure interval and the exposure-control constants, the engine's frame size
 * (the crop; the sensor's size is per stream through aof_set_bank_sensors, below), the sequence pipeline
 * (aof_sequence_device) and the per-call facade classes. */
typedef struct aof_bank_stream {     /* 32 bytes, 16-byte aligned, one per stream */
    float    focal_x, focal_y;        /* px */
    int32_t  output_rate;             /* Hz; <= 0 publishes every frame */
    uint8_t  system_id, component_id, first_seq, reserved0;
    uint64_t offset_timestamp_usec;   /* 0: records only for THIS stream (mainloop.cpp:353-357) */
    uint64_t reserved1;               /* 0 */
} aof_bank_stream;
/* Host only: the record the scalars of bp mean (reserved fields zero).  -EINVAL: NULL bp or out. */
int aof_bank_stream_from_params(const aof_bank_params *bp, aof_bank_stream *out);
/* Stores the pointer on the context, like aof_set_bank_path: enqueues nothing, allocates nothing, reads nothing.
 * d_streams: aof_bank_stream [n_streams] in device memory owned by the caller, alive and 16-byte aligned for as long
 * as it is bound; NULL (with n_streams 0) unbinds.  -EINVAL: NULL ctx, a non-NULL array with n_streams < 1, an array
 * that is not 16-byte aligned (the binding stays as it was). */
int aof_set_bank_streams(aof_ctx *ctx, const aof_bank_stream *d_streams, int32_t n_streams);

/* ---- the stream bank with sensor frames: crop, exposure statistics and de-rotation in the tick ----
 * The reference's per-frame loop does not begin at calcFlow(): a full sensor frame arrives, is centre-cropped to the
 * engine's size (mainloop.cpp:295-298,317-319), the crop's central 128x128 region goes into the 10-bin histogram whose
 * mean sample value drives the auto-exposure loop at 5 Hz (mainloop.cpp:197-220,273-274), and only then comes
 * calcFlow().  aof_bank_push_camera_device is aof_bank_push_device for S raw sensor frames:
 *   * crop: the frame a stream is given in a tick is the centre crop of its sensor frame, the rectangle of
 *     aof_ingest_batch_device (x0 = camera_width/2 - crop_width/2, y0 likewise).  From there on the tick is exactly
 *     aof_bank_push_device on the cropped frames: d_records, d_mavlink, d_mavlink_len, the stored frames and the
 *     limiter, gyro and counter fields of the state are byte-identical to that call.  Stream s's sensor frame sits at
 *     d_camera + s*camera_stride; it needs no alignment, and its crop origin may fall on any byte;
 *   * exposure gate, per stream (mainloop.cpp:199-201,273-274): the state record holds next_exposure_us, a u64 in the
 *     record's last 8 bytes, 0 after a reset.  An active frame with 64-bit time t is DUE iff t >= next_exposure_us
 *     (the untruncated time, as the reference compares it).  A due frame gets the masked histogram of
 *     aof_ingest_batch_device and its aof_exposure_msv, and sets next_exposure_us = t + exposure_interval_us.  A frame
 *     that is not due, and an idle stream, get an all-zero record.  A stream's first frame is always due.  With
 *     d_exposure == NULL no statistics are computed and the gate does not move; aof_bank_push_device passes the field
 *     through untouched;
 *   * de-rotation, with cam->derotate and d_derotated (float [S][2]): every active frame that is not a first frame gets
 *     the two floats aof_derotate_batch_device gives for (this tick's pixel record, d_gyro[s]); first frames and idle
 *     streams get 0, 0; a NULL d_gyro means zeros.
 * Small configurations (see above) run the whole tick as ONE kernel that reads the crop's rows straight out of the
 * sensor frames; every other configuration, and large banks, crop into the bank's staging region (aof_ingest_batch_device's
 * kernel), run aof_flow_batch_device's plan on (bank frames, staging) and finish with the commit kernel.  Same bytes
 * either way; aof_set_bank_path applies. */
typedef struct aof_bank_camera {
    aof_ingest_params ingest;      /* sensor size -> crop; crop size == the context's frame size */
    int64_t camera_stride;         /* bytes between the sensor frames of consecutive streams; 0 = camera_width*camera_height */
    uint32_t exposure_interval_us; /* mainloop.cpp:274: 200 000; 0 = statistics with every frame */
    uint8_t derotate;              /* 1: d_derotated is written */
    aof_derotate_params derotate_params;
} aof_bank_camera;

typedef struct aof_exposure_record {   /* 48 bytes, one per stream and tick */
    uint32_t hist[AOF_EXPOSURE_BINS];
    float msv;                          /* aof_exposure_msv(hist), bit for bit */
    uint32_t due;                       /* 1: this frame passed the stream's exposure gate; 0: hist and msv are zero */
} aof_exposure_record;

/* The regions of aof_bank_layout at the same offsets, and one region behind them at *staging: u8 [S][frame_stride]
 * and u32 [S][10], for the composed path (out->total_bytes includes it).  A bank sized by it also serves
 * aof_bank_push_device.  -EINVAL: what aof_bank_layout refuses, NULL cam / out / staging, a crop size that is not the
 * frame size of `p`, a crop larger than the sensor frame, a camera_stride below one sensor frame.  Host only. */
int aof_bank_camera_layout(const aof_params *p, const aof_bank_params *bp, const aof_bank_camera *cam,
                           struct aof_bank_layout *out, size_t *staging);
/* d_camera: u8, stream s's sensor frame at + s*camera_stride.  d_exposure: aof_exposure_record [S] or NULL.
 * d_derotated: float [S][2], required with cam->derotate (else not written).  Everything else as aof_bank_push_device.
 * -EINVAL: everything aof_bank_camera_layout and aof_bank_push_device refuse, cam->derotate without d_derotated,
 * d_exposure or d_derotated not 4-byte aligned; -ENOSPC: a bank smaller than aof_bank_camera_layout().total_bytes;
 * -EIO: the context's sticky fault.  A refused call leaves the bank untouched.  Only enqueues; capturable. */
int aof_bank_push_camera_device(aof_ctx *ctx, const aof_bank_params *bp, const aof_bank_camera *cam,
                                const uint8_t *d_camera, const uint64_t *d_time_us, const uint8_t *d_active,
                                const aof_gyro *d_gyro, void *d_bank, size_t bank_bytes, aof_tick_record *d_records,
                                aof_exposure_record *d_exposure, float *d_derotated,
                                uint8_t *d_mavlink, uint8_t *d_mavlink_len, void *stream);

/* ---- the stream bank in bursts: K frame rounds per stream from one launch ----
 * A camera delivers about 75 frames/s and the limiter publishes at 15 Hz (mainloop.cpp:39-44,59): a service that holds
 * many cameras, a stream that catches up after a stall and a replay of many recordings all have several frames per
 * stream at hand.  aof_bank_push_burst_device and aof_bank_push_camera_burst_device take K rounds of frames at once.
 * The layout is round-major, so that round k of a burst is exactly one tick buffer of the single-tick calls:
 *   * stream s's frame of round k sits at d_frames + k*round_stride + s*frame_stride (the camera form: d_camera +
 *     k*round_stride + s*camera_stride);
 *   * d_time_us, d_gyro, d_records, d_mavlink_len and d_exposure are dense [K][S], d_derotated is [K][S][2], d_mavlink
 *     is [K][S][AOF_SEQ_FRAME_BYTES];
 *   * d_count: u8 [S] or NULL (= K everywhere).  Stream s has frames in rounds 0 .. d_count[s]-1 and is idle in the
 *     others; a value above K counts as K (the kernel clamps it: the host cannot see device data).
 * Contract: every output (idle records included) and the bank's frames and state regions after the call are
 * byte-identical to K consecutive calls of the single-tick entry point on the same bank, call k with round k's buffers
 * and d_active[s] = (k < d_count[s]).  Everything the single tick defines therefore carries over round by round: first
 * frames, the limiter's u32 wrap, AOF_TICK_HELD / AOF_TICK_IDLE, gyro sums taken with each published record,
 * per-stream MAVLink sequence numbers, the 64-bit exposure gate, de-rotation of every non-first active frame.  The
 * scratch, flows and staging regions are unspecified, as they are after a tick.
 * A bank sized by aof_bank_layout / aof_bank_camera_layout serves bursts.  Small configurations run a burst as ONE
 * kernel, a workgroup per stream that keeps the newest frame (with its level-1 image and pixel sums) in LDS from round
 * to round, reads the stored frame once and writes it once: (K+2) W H bytes per stream instead of 3 K W H.  Every other
 * configuration, and large banks, run K rounds of the single tick's composed launches in order.  Same bytes either
 * way; aof_set_bank_path applies.  Both calls only enqueue: no allocation, no host synchronisation, capturable. */
#define AOF_BANK_BURST_MAX 16
typedef struct aof_bank_burst {
    int32_t n_rounds;        /* K: 1 .. AOF_BANK_BURST_MAX */
    int64_t round_stride;    /* bytes between round k and round k+1 of the frame buffer; 0 = dense: n_streams *
                                frame_stride (the camera form: n_streams * camera_stride).  It must hold one round
                                (>= that product); for pre-cropped frames a multiple of 16 */
} aof_bank_burst;
/* -EINVAL: everything aof_bank_push_device refuses, a NULL burst, n_rounds outside 1..AOF_BANK_BURST_MAX, a bad
 * round_stride; -ENOSPC, -EIO as there.  A call refused for its arguments or for the context's sticky fault leaves the bank
 * untouched.  On the composed path a launch that fails in round k > 0 (-EIO, or what aof_flow_batch_device returns) comes
 * back after rounds 0 .. k-1 have been enqueued: the bank then holds those rounds, as after k single ticks. */
int aof_bank_push_burst_device(aof_ctx *ctx, const aof_bank_params *bp, const aof_bank_burst *burst,
                               const uint8_t *d_frames, const uint64_t *d_time_us, const uint8_t *d_count,
                               const aof_gyro *d_gyro, void *d_bank, size_t bank_bytes, aof_tick_record *d_records,
                               uint8_t *d_mavlink, uint8_t *d_mavlink_len, void *stream);
/* -EINVAL: everything aof_bank_push_camera_device refuses, a NULL burst, n_rounds outside 1..AOF_BANK_BURST_MAX, a
 * round_stride below one round of sensor frames; -ENOSPC, -EIO as there.  What a refused or failed call leaves: as
 * aof_bank_push_burst_device. */
int aof_bank_push_camera_burst_device(aof_ctx *ctx, const aof_bank_params *bp, const aof_bank_camera *cam,
                                      const aof_bank_burst *burst, const uint8_t *d_camera, const uint64_t *d_time_us,
                                      const uint8_t *d_count, const aof_gyro *d_gyro, void *d_bank, size_t bank_bytes,
                                      aof_tick_record *d_records, aof_exposure_record *d_exposure, float *d_derotated,
                                      uint8_t *d_mavlink, uint8_t *d_mavlink_len, void *stream);

/* ---- the stream bank with per-stream sensors: size, row pitch, crop origin and place of every camera's frame ----
 * aof_bank_camera carries ONE sensor size for all S streams, rows exactly camera_width bytes apart, frames camera_stride
 * apart and the reference's centre crop.  Real fleets mix resolutions, drivers pad rows (V4L2 bytesperline), a
 * calibrated camera is cropped around its principal point, and a frame sits wherever its capture buffer is.  A caller
 * may therefore bind an array of S sensor records in device memory to the context; while it is bound, stream s of the
 * camera pushes (aof_bank_push_camera_device, aof_bank_push_camera_burst_device) takes its new frame from
 *     d_camera + k*round_stride + offset + (y0 + y)*pitch + x0 + x,   0 <= y < crop_height, 0 <= x < crop_width
 * (k: the round of a burst, 0 for a tick).  From the cropped frame on nothing changes.
 * Validity is decided on the device, per stream and round (the host cannot see device data).  A record is valid iff
 *     width >= 1, height >= 1, pitch >= width;  x0 >= 0, y0 >= 0, x0 + crop_width <= width, y0 + crop_height <= height;
 *     k*round_stride + offset + (height-1)*pitch + width <= camera_bytes     (in 64 bits, nothing wraps),
 * camera_bytes being the number of bytes the caller guarantees readable from the d_camera of the pushes.  A stream with
 * an invalid record is treated exactly as an idle stream in that round: not one byte of its sensor frame is read, its
 * bank bytes are not written, its exposure record, de-rotated pair and MAVLink length are the idle ones -- only the tick
 * record's quality is AOF_TICK_BAD_SENSOR instead of AOF_TICK_IDLE.  aof_bank_collect_device and aof_bank_imu_device need
 * no change: they pass or skip every record with quality < 0.
 * Contract (a bank of one): stream s's records, wire frames, exposure records, de-rotated pairs, stored frame and state
 * (exposure gate included) are byte-identical to those of a one-stream camera bank whose aof_bank_camera has
 * camera_width = pitch_s, camera_height = height_s, whose d_camera points at offset_s and whose crop sits at (x0_s, y0_s)
 * where the unbound form would have centred it.  S records equal to aof_bank_sensor_from_camera(p, cam, s) change no byte
 * of any output or of the bank.  With an array bound, cam->ingest.camera_width / camera_height and cam->camera_stride
 * are checked exactly as without one and used by no kernel (a burst's round_stride 0 still means n_streams *
 * camera_stride); the exposure mask depends on the crop size only.  With nothing bound every kernel runs on its
 * arguments as before.  A burst indexes the array by the stream alone, its outputs by round * S + stream.
 * The KERNELS read the array when they run: records may be rewritten between ticks in stream order (a ring of capture
 * buffers: a new offset every tick), and a captured graph replays against the current contents.
 * Still not per stream: the ENGINE's frame size (the crop) is the context's. */
#define AOF_TICK_BAD_SENSOR (-5)     /* the stream's sensor record does not describe memory inside the camera buffer */
typedef struct aof_bank_sensor {     /* 32 bytes, 16-byte aligned, one per stream */
    uint64_t offset;                 /* bytes from d_camera (round k of a burst: + k*round_stride) to the frame's first byte */
    int32_t  pitch;                  /* bytes between rows, >= width */
    int32_t  width, height;          /* the grey (Y) plane, pixels */
    int32_t  x0, y0;                 /* crop origin inside it; the crop is the context's width x height */
    uint32_t reserved;               /* 0 */
} aof_bank_sensor;
/* Stores the pointer and camera_bytes on the context, like aof_set_bank_streams: enqueues nothing, allocates nothing,
 * reads nothing.  d_sensors: aof_bank_sensor [n_streams] in device memory owned by the caller, alive and 16-byte aligned
 * for as long as it is bound; NULL (with n_streams 0) unbinds.  A camera push whose bp->n_streams differs from the bound
 * count returns -EINVAL and writes nothing; the pushes of pre-cropped frames do not look at the binding.
 * -EINVAL: NULL ctx, a non-NULL array with n_streams < 1, an array that is not 16-byte aligned, camera_bytes == 0 with
 * an array (the binding stays as it was). */
int aof_set_bank_sensors(aof_ctx *ctx, const aof_bank_sensor *d_sensors, int32_t n_streams, uint64_t camera_bytes);
/* Host only: the record the scalars of cam mean for stream `stream`: offset = stream * camera_stride (camera_width *
 * camera_height where camera_stride is 0), pitch = width = camera_width, height = camera_height, the centre crop of
 * p->width x p->height.  -EINVAL: NULL p / cam / out, stream < 0, a crop that is not inside the sensor frame. */
int aof_bank_sensor_from_camera(const aof_params *p, const aof_bank_camera *cam, int32_t stream, aof_bank_sensor *out);
/* Host only: the same centre rule (x0 = width/2 - p->width/2, y0 likewise) for a caller's own place, pitch and size.
 * -EINVAL: NULL p / out, pitch < width, a crop that is not inside width x height. */
int aof_bank_sensor_centred(const aof_params *p, uint64_t offset, int32_t pitch, int32_t width, int32_t height, aof_bank_sensor *out);
/* Host only: the kernels' validity rule (the same function, compiled for the host) on one record: 1 valid, 0 not, for a
 * crop of crop_width x crop_height, the round's base = k*round_stride and camera_bytes.  -EINVAL: NULL rec. */
int aof_bank_sensor_valid(const aof_bank_sensor *rec, int32_t crop_width, int32_t crop_height, uint64_t base, uint64_t camera_bytes);
/* aof_ingest_batch_device for frames that sensor records describe: frame i is the crop_width x crop_height rectangle at
 * (x0_i, y0_i) of the frame at d_camera + offset_i with rows pitch_i apart; d_cropped, cropped_stride and d_hist as
 * there (either output may be NULL).  A frame whose record is not valid against camera_bytes (base 0) is not read;
 * d_ok: u8 [n_frames] or NULL: 1 for a valid record, 0 for an invalid one, whose cropped frame and histogram are then
 * unspecified (with crops of more than 128 rows its histogram is zero).  Stateless, asynchronous on `stream`.
 * -EINVAL: crop_width or crop_height < 1, n_frames < 0, NULL d_camera or d_sensors, d_sensors not 16-byte aligned,
 * camera_bytes 0, both outputs NULL, a cropped_stride below one crop. */
int aof_ingest_sensors_device(int32_t crop_width, int32_t crop_height, const uint8_t *d_camera, uint64_t camera_bytes,
                              const aof_bank_sensor *d_sensors, int64_t n_frames, uint8_t *d_cropped, int64_t cropped_stride,
                              uint32_t *d_hist, uint8_t *d_ok, void *stream);

/* ---- the stream bank with packed sensor pixels: YUYV, UYVY and Y16 buffers as the driver filled them ----
 * The sensor records above describe one byte per pixel.  Most UVC cameras deliver YUYV (packed 4:2:2, the luma in the
 * even bytes), many CSI bridges UYVY (the luma in the odd bytes), mono global-shutter sensors Y16 (the grey value the
 * engine wants is the high byte of each little-endian 16-bit pixel).  A caller may therefore bind, next to the sensor
 * records, an array of S pixel formats in device memory; stream s's crop is then fetched from pixels of bpp bytes whose
 * grey value is byte `phase`:
 *     format               bpp  phase
 *     AOF_PIXEL_GREY8       1     0      exactly the records alone
 *     AOF_PIXEL_LUMA16_LO   2     0      YUYV, YVYU, Y16_BE
 *     AOF_PIXEL_LUMA16_HI   2     1      UYVY, VYUY, Y16 (little endian: its high byte)
 * Pixel (x, y) of the crop is the byte at
 *     d_camera + k*round_stride + offset + (y0 + y)*pitch + (x0 + x)*bpp + phase.
 * width, x0 and the crop size stay in pixels, offset and pitch in bytes.  From the cropped frame on nothing changes
 * (exposure mask, histogram, MSV, flow, limiter, wire frame, de-rotation).  The kernels fetch the 32 source bytes of a
 * 16-pixel piece and pack every pixel's byte 0 or byte 1 (a uniform shift, then v_perm_b32): no de-interleave pass, no
 * second buffer.
 * A record with its format is valid iff, in 64 bits so that nothing wraps,
 *     format <= 2 (4 .. 8: "raw mono pixels" below);  width >= 1, height >= 1, pitch >= width*bpp;  the crop inside width x height;
 *     k*round_stride + offset + (height-1)*pitch + width*bpp <= camera_bytes.
 * An invalid record or format is treated as an invalid record is today: AOF_TICK_BAD_SENSOR for that round, not one byte
 * of the stream's frame read, its bank bytes untouched.
 * Binding: the formats are used by the two camera pushes, and only with a sensor array bound as well -- formats bound
 * without sensors make those pushes return -EINVAL; bp->n_streams must equal the bound format count (else -EINVAL, and
 * nothing is written); the pushes of pre-cropped frames ignore the binding; a burst indexes the array by the stream
 * alone.  The KERNELS read the array when they run: it may be rewritten between ticks, and a replayed graph sees the
 * current contents.
 * Contracts: (a) stream s's outputs and bank bytes equal those of the grey sensor path fed the de-interleaved plane
 * (a grey record of the same width, height, x0, y0 and the grey buffer's own pitch); (b) an array of all
 * AOF_PIXEL_GREY8 changes no byte against sensors bound alone. */
#define AOF_PIXEL_GREY8     0   /* one byte per pixel: exactly the behaviour without formats */
#define AOF_PIXEL_LUMA16_LO 1   /* two bytes per pixel, grey value = first byte: YUYV, YVYU, Y16_BE */
#define AOF_PIXEL_LUMA16_HI 2   /* two bytes per pixel, grey value = second byte: UYVY, VYUY, Y16 (LE: its high byte) */
/* Stores the pointer on the context, like aof_set_bank_streams: enqueues nothing, allocates nothing, reads nothing.
 * d_formats: u8 [n_streams] in device memory owned by the caller, alive for as long as it is bound; any alignment; the
 * kernels read nothing outside d_formats[0..n_streams).  NULL (with n_streams 0) unbinds.
 * -EINVAL: NULL ctx, a non-NULL array with n_streams < 1 (the binding stays as it was). */
int aof_set_bank_pixel_formats(aof_ctx *ctx, const uint8_t *d_formats, int32_t n_streams);
/* Host only: aof_bank_sensor_valid for a record of pixel format `format` (the same function the kernels decide with,
 * compiled for the host): 1 valid, 0 not (a value that is no format -- 3, 9..255 -- included).  -EINVAL: NULL rec. */
int aof_bank_sensor_valid_format(const aof_bank_sensor *rec, uint8_t format, int32_t crop_width, int32_t crop_height,
                                 uint64_t base, uint64_t camera_bytes);
/* aof_ingest_sensors_device with frame i's pixel format d_formats[i] (u8 [n_frames], device memory, any alignment);
 * d_formats NULL: every frame AOF_PIXEL_GREY8 -- aof_ingest_sensors_device is this call with NULL.  A frame whose record
 * or format is not valid is not read (d_ok 0).  -EINVAL as there. */
int aof_ingest_sensor_formats_device(int32_t crop_width, int32_t crop_height, const uint8_t *d_camera, uint64_t camera_bytes,
                                     const aof_bank_sensor *d_sensors, const uint8_t *d_formats, int64_t n_frames,
                                     uint8_t *d_cropped, int64_t cropped_stride, uint32_t *d_hist, uint8_t *d_ok, void *stream);

/* ---- the stream bank with binned sensor pixels: 2x2 and 4x4 binning per stream, inside the crop ----
 * An 8x8 / +-4 search measures at most +-4 pixels per frame pair (+-9 on two levels).  A faster vehicle or a wider lens
 * bins its sensor, as the published PX4Flow pipeline does (4x, in front of its 64x64 window).  A caller may bind, next
 * to the sensor records and the formats, an array of S bins in device memory: b = d_bins[s] is 1, 2 or 4
 * (AOF_BANK_BIN_MAX); any other value makes the stream's record invalid.  With g(X, Y) the grey byte of sensor pixel
 * (X, Y) -- the byte at d_camera + k*round_stride + offset + Y*pitch + X*bpp + phase, as above -- pixel (x, y) of the
 * crop is
 *     (sum over j < b, i < b of g(x0 + b*x + i, y0 + b*y + j) + b*b/2) >> (2*log2 b).
 * b = 2 is the pyramid's box (a+b+c+d+2)>>2; b = 4 is ONE rounding of the sixteen-pixel sum, (sum + 8) >> 4, not the
 * box applied twice (quadrant sums 2, 2, 2, 1 give 0 here, 1 there); b = 1 is the crop as it was.
 * Units: width, height, x0, y0 stay in SENSOR pixels, pitch and offset in bytes; the context's width x height is the
 * size of the BINNED crop, whose footprint is b*width x b*height sensor pixels at (x0, y0).
 * A record with its format and bin is valid iff, in 64 bits so that nothing wraps,
 *     b in {1, 2, 4};  x0 >= 0, y0 >= 0, x0 + b*crop_width <= width, y0 + b*crop_height <= height;
 * and everything else as above (pitch >= width*bpp, the extent against camera_bytes).  An invalid record or bin is
 * treated as an invalid record is: AOF_TICK_BAD_SENSOR for that round, not one byte of the stream's frame read.
 * Contract (a bank of one): stream s's records, wire frames, exposure records (histogram and MSV: those of the binned
 * crop), de-rotated pairs, stored frame and state, exposure gate included, equal byte for byte those of a grey stream
 * (AOF_PIXEL_GREY8, bin 1) whose sensor frame is the binned crop computed on the host.  The exposure mask depends on
 * the crop size only.  An array of all ones changes no byte against sensors (and formats) bound alone; with nothing
 * bound every kernel runs as before.
 * Binding: used by the two camera pushes, with sensor records bound -- a binning bound without records, or a bound
 * count that differs from bp->n_streams, makes those pushes return -EINVAL before anything is enqueued.  It combines
 * with every format, bound or not.  The KERNELS read the array when they run: values may be rewritten between ticks, a
 * captured graph replays against the current contents, a burst indexes the array by the stream alone.
 * The focal length is the caller's: a binned pixel subtends b sensor pixels, so a caller binds focal / b through
 * aof_bank_stream (aof_set_bank_streams).  The library does not scale it. */
#define AOF_BANK_BIN_MAX 4
/* Stores the pointer on the context, like aof_set_bank_pixel_formats: enqueues nothing, allocates nothing, reads
 * nothing.  d_bins: u8 [n_streams] in device memory owned by the caller, alive for as long as it is bound; any
 * alignment; the kernels read nothing outside d_bins[0..n_streams).  NULL (with n_streams 0) unbinds.
 * -EINVAL: NULL ctx, a non-NULL array with n_streams < 1 (the binding stays as it was). */
int aof_set_bank_binning(aof_ctx *ctx, const uint8_t *d_bins, int32_t n_streams);
/* Host only: aof_bank_sensor_valid_format for a record binned `bin` times (the same function the kernels decide with,
 * compiled for the host): 1 valid, 0 not (a bin that is none of 1, 2, 4 included).  -EINVAL: NULL rec. */
int aof_bank_sensor_valid_binned(const aof_bank_sensor *rec, uint8_t format, uint8_t bin, int32_t crop_width, int32_t crop_height,
                                 uint64_t base, uint64_t camera_bytes);
/* Host only: aof_bank_sensor_centred for a binned stream: x0 = width/2 - (bin*p->width)/2, y0 likewise.
 * For the MIPI-packed forms ("raw mono pixels" below) x0 is rounded down to a multiple of G.
 * -EINVAL: NULL p / out, and wherever the record would be invalid (a value that is no format, a bin that is none of
 * 1, 2, 4, pitch < row_bytes, a footprint that is not inside width x height); *out is then not written. */
int aof_bank_sensor_centred_binned(const aof_params *p, uint64_t offset, int32_t pitch, int32_t width, int32_t height,
                                   uint8_t format, uint8_t bin, aof_bank_sensor *out);
/* aof_ingest_sensor_formats_device with frame i binned d_bins[i] times (u8 [n_frames], device memory, any alignment);
 * d_bins NULL: 1 everywhere -- aof_ingest_sensor_formats_device is this call with NULL.  crop_width x crop_height is
 * the size of the binned crop.  A frame whose record, format or bin is not valid is not read (d_ok 0).  -EINVAL as there. */
int aof_ingest_sensors_binned_device(int32_t crop_width, int32_t crop_height, const uint8_t *d_camera, uint64_t camera_bytes,
                                     const aof_bank_sensor *d_sensors, const uint8_t *d_formats, const uint8_t *d_bins,
                                     int64_t n_frames, uint8_t *d_cropped, int64_t cropped_stride, uint32_t *d_hist, uint8_t *d_ok,
                                     void *stream);

/* ---- the stream bank with raw mono pixels: Y10, Y12, Y14, Y10P and Y12P buffers as the CSI receiver filled them ----
 * Mono global-shutter flow sensors (OV7251, OV9281, MT9V034) are 10- or 12-bit parts, and without an ISP in front the
 * V4L2 buffer holds their samples right-justified in 16-bit little-endian words (Y10, Y12, Y14) or MIPI-packed (Y10P:
 * four pixels in five bytes, Y12P: two pixels in three).  Five more values of a stream's format byte describe them.  A
 * row is groups of G pixels in Bg bytes; the grey value of sensor pixel X of a row is the top eight bits of its
 * sample, truncated -- what the sensor's own 8-bit mode gives:
 *     code  format          Bg / G   grey value of pixel X (row: the row's first byte)
 *       3   (none)                   no format, as are 9..255
 *       4   AOF_PIXEL_Y10   2 / 1    (v >> 2) & 0xFF, v the little-endian 16-bit word at row + 2*X
 *       5   AOF_PIXEL_Y12   2 / 1    (v >> 4) & 0xFF
 *       6   AOF_PIXEL_Y14   2 / 1    (v >> 6) & 0xFF
 *       7   AOF_PIXEL_Y10P  5 / 4    the byte at row + (X/4)*5 + X%4 (MIPI RAW10: the four high bytes lead, the fifth
 *                                    byte holds the low bits)
 *       8   AOF_PIXEL_Y12P  3 / 2    the byte at row + (X/2)*3 + X%2
 * with row = d_camera + k*round_stride + offset + Y*pitch.  Bits above the sample and the low-bit bytes of the packed
 * forms are never looked at.  AOF_PIXEL_LUMA16_LO and _HI are the 16-bit form with shifts 0 and 8, AOF_PIXEL_GREY8 is
 * 1 / 1.  Everything behind the crop is unchanged, and binning composes as written above: the once-rounded mean of
 * bin x bin grey values g(X, Y).  The kernels fetch exactly the 32, 20 or 24 source bytes of a 16-pixel piece -- whole
 * groups of the crop's own pixels -- and select bytes in registers: no unpack pass, no second buffer.
 * With row_bytes = (width / G) * Bg, a record with one of these formats (and its bin) is valid iff, in 64 bits so that
 * nothing wraps,
 *     width % G == 0 and x0 % G == 0;  width >= 1, height >= 1, pitch >= row_bytes;
 *     the crop's footprint (bin*crop_width x bin*crop_height at x0, y0) inside width x height;
 *     k*round_stride + offset + (height-1)*pitch + row_bytes <= camera_bytes.
 * (For G = 1 this is the rule above.)  An invalid record is treated as any invalid record is: AOF_TICK_BAD_SENSOR for
 * that round, not one byte of the stream's frame read, its bank bytes untouched.  Binding and rewriting: as for every
 * format byte.  Contract (a) holds for these forms as well: stream s's outputs and bank bytes equal those of the grey
 * sensor path fed the plane of grey values defined by the table (a grey record of the same width, height, x0, y0 and
 * the grey buffer's own pitch), byte for byte.
 * Not served: big-endian samples, Y14P, Bayer mosaics, rounding, an x0 that is no multiple of G. */
#define AOF_PIXEL_Y10  4   /* 16-bit little-endian word, sample in bits 9..0 */
#define AOF_PIXEL_Y12  5   /* 16-bit little-endian word, sample in bits 11..0 */
#define AOF_PIXEL_Y14  6   /* 16-bit little-endian word, sample in bits 13..0 */
#define AOF_PIXEL_Y10P 7   /* MIPI RAW10: four pixels in five bytes */
#define AOF_PIXEL_Y12P 8   /* MIPI RAW12: two pixels in three bytes */
/* Host only: the bytes of a row of `width` pixels of `format`, (width / G) * Bg, into *out; 0.
 * -EINVAL: a value that is no format, width < 1, width % G != 0, NULL out (*out is then not written). */
int aof_bank_pixel_row_bytes(uint8_t format, int32_t width, int64_t *out);

/* ---- the stream bank with a lens: per-stream undistortion (a warp mesh) in place of the plain crop ----
 * The reference crops the centre "because optical flow assumes narrow field of view" (mainloop.cpp:294) and has nothing
 * for the lens itself; upstream's OpticalFlowOpenCV takes a camera matrix and distortion coefficients.  Short, cheap
 * lenses bend the crop's edge by several percent.  A caller may make resampling through a lens model a property of a
 * stream: a MESH of one node every AOF_WARP_CELL = 8 crop pixels on both axes,
 *     nx = (width + 7) / 8 + 1,  ny = (height + 7) / 8 + 1   nodes, row-major (aof_warp_mesh_size),
 * for the context's width x height crop.  Node (cx, cy) is the sensor-plane coordinate of the CENTRE of crop pixel
 * (8 cx, 8 cy), in 1/32 pixel (AOF_WARP_FRAC_BITS = 5), relative to pixel (0, 0) of the stream's grey plane: the plane of
 * width x height pixels of the stream's sensor record (with nothing bound: cam->ingest's camera_width x camera_height
 * frame of the stream).  With xmax = min(width - 1, 32767), ymax likewise, the grey value of crop pixel (x, y) is, all in
 * 32-bit integers of which none can wrap:
 *     every node coordinate is first clamped to [0, xmax*32] / [0, ymax*32] (never invalid: the border replicates);
 *     cx = x >> 3, cy = y >> 3, i = x & 7, j = y & 7;  A, B, C, D the clamped nodes (cx, cy), (cx+1, cy), (cx, cy+1),
 *     (cx+1, cy+1);  per axis  N = (8-i)(8-j) A + i (8-j) B + (8-i) j C + i j D,  X = (N + 32) >> 6;
 *     xi = X >> 5, fx = X & 31, x1 = min(xi + 1, xmax); the same for y;
 *     v = (p(xi,yi)(32-fx)(32-fy) + p(x1,yi) fx (32-fy) + p(xi,y1)(32-fx) fy + p(x1,y1) fx fy + 512) >> 10,
 * with p the plane's grey value read through the stream's pixel format (the tables above, every AOF_PIXEL_*).  An
 * identity mesh, node = ((x0 + 8 cx)*32, (y0 + 8 cy)*32), gives the plain crop byte for byte wherever its nodes lie inside
 * the plane (x0 + 8 (nx - 1) <= width - 1, likewise y: a node beyond the last pixel is clamped, which compresses the last
 * cell of a crop that ends on the plane's last column or row).  A stream whose FIRST node has x == AOF_WARP_NONE is not
 * warped: it takes the plain crop of its record, wherever that lies.
 * Approximation: the mesh is piecewise bilinear.  Between nodes a lens model's curve is replaced by its chord; the error
 * per axis is at most (8^2 / 8) * |second derivative by the crop pixel|: for k1 = -0.3 at the edge of a 128-pixel crop
 * of focal length 100 (xn = 0.64), fx * |k1| * 6 xn / out_fx^2 = 0.0115 per pixel^2, so 0.09 pixel, three units of the
 * 1/32 grid, and a quarter of that at half the radius.  The mesh is exact at its nodes.
 * A stream's sensor record must be valid by the rule above -- its x0, y0 and the crop size included, whatever the mesh
 * says: that rule alone decides AOF_TICK_BAD_SENSOR, and of a stream so refused not one byte is read or written.
 * Contract: with warps bound, every camera push (tick and burst) computes a warped stream's new frame by the rule above;
 * the exposure histogram and MSV are those of the warped crop; records, wire frames, de-rotated pairs, stored frame and
 * state equal byte for byte those of a grey stream whose sensor frame is the warped crop computed on the host
 * (aof_warp_host).  aof_set_bank_path applies as it does without a lens.  The one-launch form is the tick kernel with the
 * warp inside it: one workgroup per stream clamps the stream's mesh into LDS, gathers the warped crop straight into the
 * new frame's LDS buffer and goes on as the camera tick does; a burst of K rounds is K such launches, one per round.  It
 * is taken iff the path is not 2, the configuration is of the one-workgroup class (as for every one-launch tick), the
 * frames, the mesh's nx*ny*8 bytes of nodes and the kernels' static arrays fit LDS (aof_bank_warp_one_launch below says
 * so for a configuration), and the path is 1 or n_streams is at most the warped form's crossover
 * (aof_bank_warp_crossover).  The one-launch warped push NEITHER READS NOR WRITES the staging region of the bank.
 * Otherwise the push takes the composed path: the warp launch into the staging region (with the raw histograms),
 * aof_flow_batch_device, the commit kernel; per round of a burst.  Identical bytes either way (tests compare them).  With
 * nothing bound not one launch changes.
 * Measured (profiles/bank_warp_one_launch_ab.txt; 640x480 grey frames, a barrel lens, us per tick, one-launch / composed as
 * the build before the kernel ran it): 64x64 crops 17.1 / 23.8 at 64 streams, 30.4 / 43.7 at 1 024, 56.2 / 60.0 at 2 048,
 * 89.2 / 95.2 at 4 096; two-level 128x128 33.8 / 46.2, 81.0 / 96.6, 135.8 / 137.2, 262.6 / 236.9: the crossover is 2 048
 * streams.  A lens costs 1.35 to 2.17 times the one-launch tick without one.  Not measured: the gather alone (a kernel
 * trace), the source footprint staged in LDS against taps from L2, formats other than grey, other meshes, bursts other than
 * K = 5 (LAB_LOG.md, "Stream bank warp, one launch").
 * Binding: used by the two camera pushes.  A bound count that differs from bp->n_streams, or a binning bound at the same
 * time (aof_set_bank_binning: the composition of binning and warp is not served; bin the mesh instead, nodes 2 or 4
 * times as far apart), makes those pushes return -EINVAL before anything is enqueued.  The KERNELS read the array when
 * they run: nodes may be rewritten between ticks, a captured graph replays against the current contents.
 * The focal length is the caller's: a warped crop has the focal lengths of the virtual camera (aof_lens.out_fx, out_fy),
 * which the caller binds through aof_bank_stream.  The library does not touch it. */
#define AOF_WARP_CELL 8
#define AOF_WARP_FRAC_BITS 5
#define AOF_WARP_NONE INT32_MIN
typedef struct aof_warp_point {      /* 8 bytes: a node, 1/32 sensor pixel */
    int32_t x, y;
} aof_warp_point;
typedef struct aof_lens {            /* Brown-Conrady, OpenCV's order of coefficients */
    double fx, fy, cx, cy;           /* the sensor camera, in plane pixels */
    double k1, k2, p1, p2, k3;
    double out_fx, out_fy, out_cx, out_cy;   /* the virtual pinhole camera of the crop, in crop pixels */
} aof_lens;
/* Host only: the mesh of p->width x p->height.  -EINVAL: NULL p / nx / ny, a size below 1. */
int aof_warp_mesh_size(const aof_params *p, int32_t *nx, int32_t *ny);
/* Host only: out[ny][nx] = the identity mesh of the crop at (x0, y0).  -EINVAL: NULL, or a coordinate that leaves int32. */
int aof_warp_mesh_identity(const aof_params *p, int32_t x0, int32_t y0, aof_warp_point *out);
/* Host only, all in double: for node (u, v) = (8 cx, 8 cy)
 *     xn = (u - out_cx) / out_fx, yn = (v - out_cy) / out_fy, r2 = xn^2 + yn^2, rad = 1 + r2 (k1 + r2 (k2 + r2 k3)),
 *     xd = xn rad + 2 p1 xn yn + p2 (r2 + 2 xn^2),  yd = yn rad + p1 (r2 + 2 yn^2) + 2 p2 xn yn,
 *     x = floor((fx xd + cx) * 32 + 0.5),  y = floor((fy yd + cy) * 32 + 0.5),  saturated to int32 (a NaN: 0); a first
 * node that would be AOF_WARP_NONE becomes AOF_WARP_NONE + 1.  -EINVAL: NULL, out_fx or out_fy zero or not finite. */
int aof_warp_mesh_from_lens(const aof_params *p, const aof_lens *lens, aof_warp_point *out);
/* Stores the pointer on the context, like aof_set_bank_sensors: enqueues nothing, allocates nothing, reads nothing.
 * d_points: aof_warp_point [n_streams][ny][nx] in device memory owned by the caller, alive for as long as it is bound,
 * 16-byte aligned.  NULL (with n_streams 0) unbinds.  -EINVAL: NULL ctx, a non-NULL array with n_streams < 1, a
 * misaligned array (the binding stays as it was). */
int aof_set_bank_warps(aof_ctx *ctx, const aof_warp_point *d_points, int32_t n_streams);
/* Host only: 1 if a camera push of configuration p with warps bound can run as one launch per round (the one-workgroup
 * class's verdict, and frames + nodes + static arrays inside LDS), else 0 (an invalid p included).  *lds_bytes (may be
 * NULL): the dynamic LDS a workgroup of it would ask for -- the one-workgroup plan's bytes plus 8 nx ny.  -EINVAL: NULL p. */
int aof_bank_warp_one_launch(const aof_params *p, int64_t *lds_bytes);
/* Host only: the largest n_streams at which the library's own choice (aof_set_bank_path 0) takes the one-launch kernel
 * for a push with warps bound; 0: never (path 1 still does). */
int aof_bank_warp_crossover(void);
/* aof_ingest_sensor_formats_device with frame i resampled through mesh d_points[i] (aof_warp_point [n_frames][ny][nx] of
 * the crop size, 16-byte aligned): any crop size up to 16 384 pixels wide, 16-byte stores where crop_width % 16 == 0 and
 * d_cropped, cropped_stride are multiples of 16.  d_ok[i] = 0: frame i's record is not valid; nothing of it is read and
 * no byte of its crop written (its histogram: untouched, or ten zeros where a frame is made in several strips, which add
 * to words zeroed in front of them: a crop higher than 128 rows, or higher than the 64 .. 8 rows a strip keeps from 1 920
 * pixels of width on).  -EINVAL as there, for NULL or misaligned d_points, and for a crop wider than 30 712 pixels (the
 * nodes of one cell row no longer fit a workgroup's 60 KiB: nothing is launched or written). */
int aof_ingest_warped_device(int32_t crop_width, int32_t crop_height, const uint8_t *d_camera, uint64_t camera_bytes,
                             const aof_bank_sensor *d_sensors, const uint8_t *d_formats, const aof_warp_point *d_points,
                             int64_t n_frames, uint8_t *d_cropped, int64_t cropped_stride, uint32_t *d_hist, uint8_t *d_ok,
                             void *stream);
/* Host only, no device and no context: the same for ONE frame in host memory, by the header the kernel compiles.
 * camera: camera_bytes readable bytes; sensor: the frame's record; points: [ny][nx]; cropped: crop_width * crop_height
 * bytes or NULL; hist: 10 words or NULL (the masked histogram of the warped crop).  Returns 1, or 0 where the record is
 * not valid (nothing read, nothing written), or -EINVAL: NULL camera / sensor / points, both outputs NULL, a size below 1. */
int aof_warp_host(int32_t crop_width, int32_t crop_height, const uint8_t *camera, uint64_t camera_bytes,
                  const aof_bank_sensor *sensor, uint8_t format, const aof_warp_point *points, uint8_t *cropped, uint32_t *hist);

/* ---- the stream bank's outbox: the published messages of a push as one dense, ordered, host-pollable list ----
 * A push leaves [K][S] records of which most say "nothing to do": the limiter publishes at 15 Hz from 75 Hz cameras, the
 * exposure gate opens at 5 Hz, idle streams get AOF_TICK_IDLE.  aof_bank_collect_device, enqueued behind any of the four
 * push calls (a tick is K = 1), reads only the push's output arrays and writes an OUTBOX: a 64-byte header, then one
 * 128-byte entry per published record -- what mainloop.cpp:322-373 would send: stream, round, the MAVLink frame, the
 * tick record, the de-rotated pair --, then one 64-byte entry per exposure record that is due.
 * Selection and order, with o = round * n_streams + stream:
 *   * a message entry for every o with d_records[o].quality >= 0 (first frames have quality 0 and are published, as
 *     mainloop.cpp sends them), in increasing o;
 *   * an exposure entry for every o with d_exposure[o].due != 0, in increasing o;
 *   * messages_found / exposures_found count all selected records, n_messages / n_exposures the stored ones: the first
 *     capacity_messages / capacity_exposures of them.  Of the entries behind the stored ones not one byte is written;
 *   * d_mavlink, d_mavlink_len, d_exposure, d_derotated may each be NULL: mavlink_len 0 (and an all-zero frame),
 *     mavlink_len 0, no exposure list (both counts 0), derotated 0, 0.
 * The outbox is a pure function of the input arrays.  It may be device memory, or memory of aof_outbox_alloc_host.
 * Tag: the header's first 8 bytes, the kernel's LAST store (released at system scope behind every other byte of the
 * outbox).  `tag` must be non-zero; with d_tag the kernel reads the tag from that device word (u64) instead, so that a
 * captured graph carries a fresh tag on every replay.  A host that polls an outbox in aof_outbox_alloc_host memory and
 * sees the tag it asked for may read the counts and the n_* entries at once, without any stream synchronisation (write
 * a different value over the tag, or pass another tag, before the next call).
 * One launch, no device-side waiting; only enqueues: no allocation, no host synchronisation, capturable.  Calls on one
 * context must not overlap on the device (they share the context's arrival counter, as the pushes share its vote
 * memory). */
typedef struct aof_outbox_entry {            /* 128 bytes */
    uint32_t stream;
    uint16_t round;                          /* 0 for a tick */
    uint8_t  mavlink_len;                    /* 0: no frame (no d_mavlink, or nothing was sent) */
    uint8_t  reserved0;                      /* 0 */
    uint8_t  mavlink[AOF_SEQ_FRAME_BYTES];   /* the first mavlink_len bytes of the frame, the rest 0 */
    aof_tick_record record;                  /* the 48 bytes of d_records[round][stream] */
    float    derotated[2];                   /* d_derotated[round][stream], or 0, 0 without it */
    uint8_t  reserved1[8];                   /* 0 */
} aof_outbox_entry;
typedef struct aof_outbox_exposure {         /* 64 bytes */
    uint32_t stream;
    uint16_t round;
    uint16_t reserved0;                      /* 0 */
    aof_exposure_record exposure;            /* the 48 bytes of d_exposure[round][stream]: due == 1 */
    uint8_t  reserved1[8];                   /* 0 */
} aof_outbox_exposure;
typedef struct aof_outbox_header {           /* 64 bytes, at offset 0 of the outbox */
    uint64_t tag;                            /* written LAST */
    uint32_t n_messages, messages_found;     /* stored (<= capacity_messages) / present in the input */
    uint32_t n_exposures, exposures_found;
    uint8_t  reserved[40];                   /* 0 */
} aof_outbox_header;
/* Byte offsets inside an outbox: the header at 0, aof_outbox_entry [capacity_messages] at `messages`,
 * aof_outbox_exposure [capacity_exposures] at `exposures`, each a multiple of 64.  (A struct tag only, as aof_bank_layout.) */
struct aof_outbox_layout {
    size_t total_bytes;
    size_t messages;
    size_t exposures;
};
/* -EINVAL: NULL out, a capacity above 2^31 - 1.  Host only. */
int aof_outbox_layout(uint32_t capacity_messages, uint32_t capacity_exposures, struct aof_outbox_layout *out);
/* d_records: aof_tick_record [n_rounds][n_streams]; d_mavlink u8 [K][S][AOF_SEQ_FRAME_BYTES], d_mavlink_len u8 [K][S],
 * d_exposure aof_exposure_record [K][S], d_derotated float [K][S][2]: what the push wrote, or NULL.  outbox: >=
 * aof_outbox_layout().total_bytes, 64-byte aligned, valid on the device.  d_tag: u64 device word, or NULL.
 * -EINVAL: NULL ctx, records or outbox; n_streams < 1; n_rounds outside 1..AOF_BANK_BURST_MAX (or more than 2^31 - 1
 * records in all); an outbox that is not 64-byte aligned; d_mavlink without its lengths; tag 0 with no d_tag; records,
 * exposure records or de-rotated pairs that are not 4-byte aligned; -ENOSPC: an outbox smaller than its layout; -EIO:
 * the context's sticky fault.  A refused call writes nothing. */
int aof_bank_collect_device(aof_ctx *ctx, int32_t n_streams, int32_t n_rounds, const aof_tick_record *d_records,
                            const uint8_t *d_mavlink, const uint8_t *d_mavlink_len, const aof_exposure_record *d_exposure,
                            const float *d_derotated, uint32_t capacity_messages, uint32_t capacity_exposures,
                            void *outbox, size_t outbox_bytes, uint64_t tag, const uint64_t *d_tag, void *stream);
/* Pinned, coherent, device-mapped host memory whose pointer is valid on both sides (what the per-call path's tagged
 * record lives in): an outbox the host can poll.  The calling thread's current device maps it.  -EINVAL: NULL out,
 * bytes 0; -ENOMEM.  aof_outbox_free_host(NULL) is allowed; free only once the work that writes it has drained. */
int aof_outbox_alloc_host(size_t bytes, void **out);
int aof_outbox_free_host(void *p);

/* ---- the stream bank's auto-exposure control: the PID step per stream behind a camera push ----
 * The second half of the reference's _exposure_update (mainloop.cpp:222-271): a PID controller turns the mean sample
 * value of a frame that passed the exposure gate into new exposure and gain values and decides whether the camera is
 * told about them.  aof_bank_exposure_control_device, enqueued behind a camera push (K = 1) or a camera burst, reads
 * `due` and `msv` of the push's [K][S] exposure records, steps one aof_exposure_state per stream and writes one
 * aof_exposure_command per stream and round.  The state array is the caller's device memory and no part of the bank.
 * One step per record with due != 0, in increasing round, per stream; all arithmetic IEEE float32, nothing fused:
 *     err = msv_target - msv;   d = err - msv_error_old;   msv_error_int += err
 *     ce = (float)exposure;     cg = (float)gain
 *     e  = ce + ((exposure_p*err + exposure_i*msv_error_int) + exposure_d*d)
 *     if cg > 1 or (e > exposure_max-1 and ce > exposure_max-1):              the gain branch
 *         g = cg + ((gain_p*err + gain_i*msv_error_int) + gain_d*d);  g > gain_max: g = gain_max, else g < 1: g = 1
 *         if |g - cg| > gain_change_threshold or (g < 2 and cg > 1) or (g > gain_max-1 and cg < gain_max):
 *             gain = (uint8_t)g;  flags |= AOF_EXPOSURE_SET_GAIN
 *     else:                                                                   the exposure branch
 *         e > exposure_max: e = exposure_max, else e < 1: e = 1
 *         if |e - ce| > exposure_change_threshold or (e < 2 and ce > 1) or (e > exposure_max-1 and ce < exposure_max):
 *             exposure = (uint16_t)e;  flags |= AOF_EXPOSURE_SET_EXPOSURE
 *     msv_error_old = err;  updates += 1;  flags |= AOF_EXPOSURE_UPDATED
 * This is the reference with its quirks: the integral has no anti-windup, the gain branch never touches the exposure,
 * the controller restarts from the integer the camera holds (fractions are carried by the integral only), and a NaN
 * sets nothing (every comparison with it is false).  The msv values are specified as finite. */
typedef struct aof_exposure_control {   /* the constants of mainloop.cpp:53-63 */
    float msv_target;                                   /* 5 */
    float exposure_p, exposure_i, exposure_d;           /* 100, 0.5, 0.5 */
    float gain_p, gain_i, gain_d;                       /* 50, 0.5, 0.5 */
    float exposure_change_threshold, exposure_max;      /* 30, 1727 */
    float gain_change_threshold, gain_max;              /* 15, 127 */
} aof_exposure_control;
/* -EINVAL: NULL ec.  Host only. */
int aof_exposure_control_default(aof_exposure_control *ec);

typedef struct aof_exposure_state {     /* 16 bytes, one per stream, caller-owned device memory */
    float msv_error_old, msv_error_int;
    uint16_t exposure;                  /* what the camera is running with: the last value commanded */
    uint8_t gain, reserved;             /* likewise; reserved = 0 */
    uint32_t updates;                   /* controller steps so far */
} aof_exposure_state;

#define AOF_EXPOSURE_UPDATED      1u    /* the record was due: the controller stepped */
#define AOF_EXPOSURE_SET_EXPOSURE 2u    /* tell the camera `exposure` (mainloop.cpp:266) */
#define AOF_EXPOSURE_SET_GAIN     4u    /* tell the camera `gain` (mainloop.cpp:249) */
typedef struct aof_exposure_command {   /* 16 bytes, one per stream and round */
    uint16_t exposure; uint8_t gain; uint8_t flags;   /* state values behind this step */
    float msv_error, msv_error_int;                    /* behind this step */
    uint32_t update;                                   /* the state's `updates` behind this step */
} aof_exposure_command;                 /* all zero for a record that was not due */

/* Masked streams (d_mask: u8 [S], or NULL = all) start over: both errors 0, updates 0, reserved 0, exposure and gain
 * from d_exposure0 (u16 [S]) / d_gain0 (u8 [S]) where given, else from the scalars.  The layout of the state is
 * public: a host whose camera refused a value may also overwrite a state record directly.
 * -EINVAL: NULL ctx or state, n_streams < 1, a state array that is not 4-byte aligned, d_exposure0 not 2-byte aligned;
 * -EIO: the context's sticky fault.  Only enqueues. */
int aof_bank_exposure_reset_device(aof_ctx *ctx, int32_t n_streams, const uint8_t *d_mask, uint16_t exposure0,
                                   uint8_t gain0, const uint16_t *d_exposure0, const uint8_t *d_gain0,
                                   aof_exposure_state *d_state, void *stream);
/* d_exposure: aof_exposure_record [n_rounds][n_streams], exactly what a camera push (n_rounds = 1) or a camera burst
 * wrote; only `due` and `msv` of each record are read.  d_state: [n_streams], updated in place.  d_commands:
 * aof_exposure_command [n_rounds][n_streams]; every element is written.  The kernel ends with a system-scope release
 * behind its stores: a host that has seen the tag of an aof_bank_collect_device enqueued behind it on the same stream
 * may read commands kept in aof_outbox_alloc_host memory without a synchronise.
 * -EINVAL: NULL ctx, ec, records, state or commands; n_streams < 1; n_rounds outside 1..AOF_BANK_BURST_MAX; pointers
 * that are not 4-byte aligned; a non-finite constant, exposure_max outside 1..65535, gain_max outside 1..255; -EIO:
 * the context's sticky fault.  A refused call writes nothing.  One launch; only enqueues: no allocation, no host
 * synchronisation, capturable. */
int aof_bank_exposure_control_device(aof_ctx *ctx, const aof_exposure_control *ec, int32_t n_streams, int32_t n_rounds,
                                     const aof_exposure_record *d_exposure, aof_exposure_state *d_state,
                                     aof_exposure_command *d_commands, void *stream);
/* The same function on host memory, a plain loop: no device, no context (single-camera users of OpticalFlowOpenCV,
 * and the check of the device's bytes).  -EINVAL: a NULL pointer, the counts and constants refused above. */
int aof_exposure_control_host(const aof_exposure_control *ec, int32_t n_streams, int32_t n_rounds,
                              const aof_exposure_record *records, aof_exposure_state *states,
                              aof_exposure_command *commands);

/* ---- the stream bank's IMU: raw HIGHRES_IMU samples in, gyro sums and the send gates behind a push ----
 * The gyro integrator of highres_imu_msg_callback (mainloop.cpp:383-405) and the two gates behind calcFlow() that
 * decide whether a published record is really sent: the stale-gyro drop (mainloop.cpp:336-342) and "no vehicle time
 * yet", with a time offset the first IMU message sets (mainloop.cpp:353-357, 403-404).  aof_bank_imu_device is a launch
 * of its own, enqueued behind any of the four pushes (a tick is K = 1).  That push is called with d_gyro = NULL and
 * for records only (offset_timestamp_usec = 0, no d_mavlink): the IMU call completes its records with the gyro sums,
 * turns the quality of the records the reference would not send into AOF_TICK_STALE_GYRO / AOF_TICK_NO_OFFSET and packs
 * the frames of the others.  The state array is the caller's device memory and no part of the bank.
 * Each stream walks rounds k = 0 .. K-1 in order; in a round it first takes the round's samples j = 0 .. n-1 in order,
 * then the round's record.  All arithmetic is IEEE double, every operation rounded on its own, nothing fused.
 *   sample (t, x, y, z):
 *     dt = (double)(uint64_t)(t - prev_time_usec) / 1e6          (u64 wrap: a time that runs backwards gives a huge dt;
 *                                                                  a true division)
 *     accepted iff prev_time_usec != 0 and dt < 0.05 and fabsf(x) < 20 and fabsf(y) < 20 and fabsf(z) < 20, each
 *       compared as double (NaN and infinities fail; the reference's unqualified abs is read as the float overload):
 *         gyro_x += (double)x * dt, likewise y and z;  samples_integrated++
 *     rejected: samples_rejected++
 *     prev_time_usec = t in every case;  if offset_timestamp_usec == 0: offset_timestamp_usec = t
 *     Samples are taken in rounds in which the stream is idle, too.
 *   record with quality < 0 (AOF_TICK_HELD, AOF_TICK_IDLE): copied unchanged, mavlink_len 0, the state untouched.
 *   record with quality >= 0 (first frames included, as mainloop.cpp sends them):
 *     g = (gyro_x, gyro_y, gyro_z); the sums are zeroed; the out record is the in record with gyro_x/y/z = (float)g
 *     if last_taken_time_usec == prev_time_usec: quality = AOF_TICK_STALE_GYRO, dropped++
 *     else: last_taken_time_usec = prev_time_usec; then
 *       if offset_timestamp_usec == 0: quality = AOF_TICK_NO_OFFSET, dropped++
 *       else the record is sent, its quality kept: the OPTICAL_FLOW_RAD frame of the push with time_usec =
 *         offset_timestamp_usec + d_time_us[k][s], the record's dt_us, flows and quality, the doubles g and sequence
 *         number (uint8_t)(first_seq + messages); messages++
 *   A dropped or unsent record has mavlink_len 0.  As with the push, the bytes of a frame behind its length are not
 *   written, and neither are frames of length 0.  Without d_mavlink decisions and counters are the same; only the
 *   packing is skipped.
 * aof_bank_collect_device runs unchanged on d_records_out, d_mavlink and d_mavlink_len: it selects quality >= 0, so the
 * outbox then holds what the reference would send.  `messages` counts packed frames, as a MAVLink channel's sequence
 * number does (the push's own counter counts every published record). */
#define AOF_IMU_SLOTS_MAX 16
#define AOF_TICK_STALE_GYRO (-3)  /* published by calcFlow, dropped: no IMU sample since the previous take (mainloop.cpp:337-341) */
#define AOF_TICK_NO_OFFSET  (-4)  /* published, dropped: the stream has no vehicle time yet (mainloop.cpp:353-357) */

typedef struct aof_imu_sample {   /* 24 bytes: the fields of HIGHRES_IMU the reference reads */
    uint64_t time_usec; float xgyro, ygyro, zgyro; uint32_t reserved;
} aof_imu_sample;

typedef struct aof_imu_state {    /* 64 bytes, one per stream, caller-owned device memory beside the bank */
    double gyro_x, gyro_y, gyro_z;      /* _gyro_integrated */
    uint64_t prev_time_usec;            /* _gyro_prev_timestamp */
    uint64_t last_taken_time_usec;      /* _gyro_last_usec_timestamp */
    uint64_t offset_timestamp_usec;     /* _offset_timestamp_usec; 0 = not known yet */
    uint32_t messages;                  /* frames packed so far: seq = first_seq + messages */
    uint32_t samples_integrated, samples_rejected, dropped;
} aof_imu_state;

typedef struct aof_imu_params {
    int32_t n_streams, n_rounds /* 1..AOF_BANK_BURST_MAX */, max_samples /* M: 1..AOF_IMU_SLOTS_MAX */;
    uint8_t system_id, component_id, first_seq;
} aof_imu_params;

/* Masked streams (d_mask: u8 [S], or NULL = all) are zeroed and get offset_timestamp_usec = offset0; offset0 == 0: the
 * stream learns the offset from its first sample.  A new state array must be reset once.
 * -EINVAL: NULL ctx or state, n_streams < 1, a state array that is not 8-byte aligned; -EIO: the context's sticky
 * fault.  Only enqueues. */
int aof_bank_imu_reset_device(aof_ctx *ctx, int32_t n_streams, const uint8_t *d_mask, uint64_t offset0,
                              aof_imu_state *d_state, void *stream);
/* d_samples: aof_imu_sample [K][M][S], stream fastest: sample (k, j, s) at ((k*M + j)*S + s)*24 bytes.
 * d_sample_count: u8 [K][S], the samples that arrived for stream s since its previous round and before round k's frame;
 * NULL = M everywhere; a value above M counts as M (the kernel clamps it: the host cannot see device data).
 * d_time_us: the u64 [K][S] array the push was given.  d_records_in: aof_tick_record [K][S], what the push wrote.
 * d_records_out: [K][S], d_records_in itself or disjoint from it.  d_state: [S], updated in place.  d_mavlink: u8
 * [K][S][AOF_SEQ_FRAME_BYTES] and d_mavlink_len: u8 [K][S]; both NULL, or neither.  The kernel ends with a system-scope
 * release behind its stores: a host that has seen the tag of an aof_bank_collect_device enqueued behind it on the same
 * stream may read outputs kept in aof_outbox_alloc_host memory without a synchronise.
 * -EINVAL: NULL ctx, params, samples, times, records or state; n_streams < 1; n_rounds outside 1..AOF_BANK_BURST_MAX;
 * max_samples outside 1..AOF_IMU_SLOTS_MAX; d_mavlink without its lengths or the reverse; samples, state or times not
 * 8-byte aligned, records not 4-byte aligned; -EIO: the context's sticky fault.  A refused call writes nothing.  One
 * launch; only enqueues: no allocation, no host synchronisation, capturable. */
int aof_bank_imu_device(aof_ctx *ctx, const aof_imu_params *ip, const aof_imu_sample *d_samples,
                        const uint8_t *d_sample_count, const uint64_t *d_time_us, const aof_tick_record *d_records_in,
                        aof_imu_state *d_state, aof_tick_record *d_records_out, uint8_t *d_mavlink,
                        uint8_t *d_mavlink_len, void *stream);
/* The same function on host memory, a plain loop: no device, no context (what one camera's host would call, and the
 * check of the device's bytes).  -EINVAL as above. */
int aof_bank_imu_host(const aof_imu_params *ip, const aof_imu_sample *samples, const uint8_t *sample_count,
                      const uint64_t *time_us, const aof_tick_record *records_in, aof_imu_state *states,
                      aof_tick_record *records_out, uint8_t *mavlink, uint8_t *mavlink_len);

/* ---- the stream bank's MAVLink receive: the autopilots' byte streams in, HIGHRES_IMU samples out ----
 * What mavlink_tcp.cpp:100-129 does for one connection (recvfrom fills a buffer, mavlink_parse_char runs byte by byte,
 * _handle decodes HIGHRES_IMU) for S connections in one launch in front of aof_bank_imu_device: the call turns the bytes
 * each connection received into exactly the two arrays that call takes, aof_imu_sample [K][M][S] and u8 [K][S].
 * THE CONTRACT IS THE TEXT BELOW, not the MAVLink C library: its headers were not at hand when this was written, so
 * parity with mavlink_parse_char is not pinned by any test.  The text follows the library in what matters for a healthy
 * stream: both wire versions are accepted, a frame is consumed whole by its declared length whether or not it is
 * wanted, a signature is consumed and not verified, a MAVLink 2 payload is zero-extended.  HIGHRES_IMU is message 105
 * with CRC_EXTRA 93 (MAVLink's common message set; quoted from memory of the set); its payload is 62 bytes, 63 with the
 * `id` extension, little-endian: time_usec u64 at 0, xgyro / ygyro / zgyro f32 at 20 / 24 / 28.  Nothing else is read.
 * Per stream the bytes are taken strictly in order by a state machine that survives the end of a call (TCP reads cut
 * frames anywhere):
 *   idle:      0xFD starts a MAVLink 2 frame, 0xFE a MAVLink 1 frame; any other byte: skipped++.
 *   header:    v2: 9 bytes len, incompat, compat, seq, sysid, compid, msgid[0..2]; v1: 5 bytes len, seq, sysid, compid,
 *              msgid.  A v2 incompat byte with any bit other than bit 0 set: rejected_flags++, the parser is idle at
 *              once; the byte is consumed and not rescanned, what follows is scanned in idle.
 *   payload:   len bytes (0 is allowed).     check: 2 bytes.     signature: 13 bytes, if v2 and incompat & 1.
 *   at the frame's last byte: frames++.  If msgid == 105 the checksum (X.25 as MAVLink accumulates it: start 0xFFFF,
 *              over the header bytes behind the start byte, the payload, then the byte 93) is compared, low byte
 *              first, with the two check bytes.  Mismatch: bad_check++, the frame is dropped, its bytes are never
 *              rescanned.  Match: imu_samples++; the payload's first 32 bytes, zero-extended if len < 32, give
 *              (time_usec, xgyro, ygyro, zgyro); if the round's count for the stream is below M the sample is written
 *              to slot `count` with reserved = 0 and the count rises, otherwise overflowed++ and the sample is lost.
 *              Frames of any other message are consumed by their length and never checked.
 *   bytes counts every byte taken.  No system or component filter is applied; the reference has none.
 * A sample is delivered at its frame's last byte, signature included: a frame that ends in a later round or call
 * delivers there. */
#define AOF_MAVLINK_RX_BYTES_MAX 4096
typedef struct aof_mavlink_rx_state {          /* 128 bytes per stream, caller-owned device memory */
    uint64_t bytes;
    uint32_t frames, imu_samples, bad_check, overflowed, skipped, rejected_flags;   /* the public 32 bytes */
    uint8_t  in_progress[96];                  /* the frame being received; all zero when idle; layout private */
} aof_mavlink_rx_state;
typedef struct aof_mavlink_rx_params {
    int32_t n_streams, n_rounds /* 1..AOF_BANK_BURST_MAX */, max_bytes /* B: 16..4096, a multiple of 16 */,
            max_samples /* M: 1..AOF_IMU_SLOTS_MAX */;
} aof_mavlink_rx_params;
/* Masked streams (d_mask: u8 [S], or NULL = all) are zeroed: idle, every counter 0.  A new state array must be reset
 * once.  -EINVAL: NULL ctx or state, n_streams < 1, a state array that is not 8-byte aligned; -EIO: the context's sticky
 * fault.  Only enqueues. */
int aof_bank_mavlink_rx_reset_device(aof_ctx *ctx, int32_t n_streams, const uint8_t *d_mask, aof_mavlink_rx_state *d_state,
                                     void *stream);
/* d_bytes: u8 [K][S][B], stream-major within a round (what S recv() calls into slots s*B produce), 16-byte aligned;
 * bytes of a slot behind its length may be loaded and are never interpreted.  d_len: u16 [K][S], the bytes stream s
 * received for round k; NULL = B everywhere; a value above B counts as B.  d_state: [S], updated in place.  d_samples:
 * aof_imu_sample [K][M][S] and d_sample_count: u8 [K][S], as aof_bank_imu_device takes them: the count is written for
 * every (k, s), sample slots at and behind the count are not written.  The kernel ends with a system-scope release
 * behind its stores.
 * -EINVAL: NULL ctx, params, bytes, state, samples or counts; n_streams < 1; n_rounds outside 1..AOF_BANK_BURST_MAX;
 * max_bytes outside 16..AOF_MAVLINK_RX_BYTES_MAX or no multiple of 16; max_samples outside 1..AOF_IMU_SLOTS_MAX; bytes
 * not 16-byte aligned, state or samples not 8-byte aligned, lengths not 2-byte aligned; -EIO: the context's sticky
 * fault.  A refused call writes nothing.  One launch; only enqueues: no allocation, no host synchronisation,
 * capturable. */
int aof_bank_mavlink_rx_device(aof_ctx *ctx, const aof_mavlink_rx_params *rp, const uint8_t *d_bytes, const uint16_t *d_len,
                               aof_mavlink_rx_state *d_state, aof_imu_sample *d_samples, uint8_t *d_sample_count,
                               void *stream);
/* The same function on host memory, a plain loop: no device, no context (what one camera's host would call on its
 * receive buffer, and the check of the device's bytes).  -EINVAL as above. */
int aof_bank_mavlink_rx_host(const aof_mavlink_rx_params *rp, const uint8_t *bytes, const uint16_t *len,
                             aof_mavlink_rx_state *states, aof_imu_sample *samples, uint8_t *sample_count);

/* ---- the motion FIELD of a batch: zoom, rotation and the flow at the frame centre, fitted to the block records ----
 * aof_flow holds one translation, the histogram-filtered mean of the block shifts.  A downward camera also climbs,
 * descends and yaws: the block field is then not constant, the votes spread over several bins and the peak window keeps
 * an arbitrary part of them.  This call fits, per pair, the least-squares SIMILARITY to the same block records --
 * nothing looks at the images again -- and gives the translation at the frame centre, the relative scale change and the
 * rotation.  DESIGN.md ("The motion field") is the normative text; in short, with the level-0 grid of aof_grid,
 * B = tile, S = search, W x H the frame and vthr = min(value_threshold, 0xFFFF), block k = by*nx + bx
 *   is ACCEPTED iff sad != 0xFFFF && sad < vthr (Reduce's rule: accepted == aof_flow.count),
 *   is AT REACH iff accepted and |dx - pred_x| == S or |dy - pred_y| == S (pred of the pair's aof_flow, whatever its flags say),
 *   sits at X = 2*(x0 + bx*step_x) + B - W, Y = 2*(y0 + by*step_y) + B - H (half-pixels from the frame centre to the block centre)
 *   and moved by U = 2*dx + hx, V = 2*dy + hy (half-pixels; (hx, hy) from the sub-direction as in Reduce, (0, 0) without subdirs).
 * Over a set M of blocks the exact integer sums n, SX, SY, SU, SV, Q = sum(X*X + Y*Y), A = sum(X*U + Y*V),
 * C = sum(X*V - Y*U) give D = n*Q - SX*SX - SY*SY, Na = n*A - SX*SU - SY*SV, Nb = n*C - SX*SV + SY*SU; M FITS iff
 * n >= min_blocks and D > 0.  The model, in double, every operation rounded on its own (no fused multiply-add), integers
 * converted to double first:  a = Na / D,  b = Nb / D,  tU = ((SU - a*SX) + b*SY) / n,  tV = ((SV - b*SX) - a*SY) / n;
 * it says U ~ tU + a*X - b*Y and V ~ tV + b*X + a*Y.
 * M1 = the accepted blocks, without those at reach when exclude_reach is set.  With passes == 2, M2 = the blocks of M1
 * with fabs(U - ((tU + a*X) - b*Y)) <= g and fabs(V - ((tV + b*X) + a*Y)) <= g, g = 2.0 * (double)gate_px; if M2 fits,
 * its model is published and AOF_FIELD_REFIT set, else M1's.  If M1 does not fit the record is all zero except
 * `accepted` and `at_reach`.
 * The stream bank publishes the same fit per stream and limiter window ("the stream bank's motion field", below;
 * OpticalFlowBank::enableField), and the sequence pipeline per record of a recording ("the sequence pipeline's motion
 * field", below).  Not here: the per-call path (aof_flow_pair_host, aof_stream_push_host) and the per-call facade classes
 * publish no field. */
typedef struct aof_field_params {
    int32_t min_blocks;     /* >= 3, default 8 */
    int32_t passes;         /* 1 | 2, default 2 */
    int32_t exclude_reach;  /* 0 | 1, default 1 */
    float gate_px;          /* > 0, finite, default 1.0 */
} aof_field_params;
#define AOF_FIELD_VALID 1u
#define AOF_FIELD_REFIT 2u
typedef struct aof_field {              /* 64 bytes, 8-byte aligned, one per pair */
    int64_t det, num_zoom, num_rot;     /* D, Na, Nb of the published set */
    uint32_t accepted, at_reach, fitted /* |M1| */, used /* |published set| */;
    float zoom, rotation;               /* (float)a, (float)b: relative scale change, radians (small angle) */
    float centre_x, centre_y;           /* (float)(tU*0.5), (float)(tV*0.5): level-0 pixels at the frame centre */
    uint32_t flags, reserved;           /* AOF_FIELD_*; reserved = 0 */
} aof_field;
int aof_field_params_default(aof_field_params *fp);
/* 0 where the fit serves the geometry of `p`; -EINVAL for parameters aof_params_check refuses and for a level-0 grid with
 * nb*nb * (Xmax*Xmax + Ymax*Ymax) >= 2^62 (nb blocks, Xmax / Ymax the largest |X| / |Y| of the grid): below that bound every
 * sum and product above fits int64 (the proof stands in csrc/aof_field.cpp).  Host only. */
int aof_field_supported(const aof_params *p);
/* d_blocks: [n_pairs][nb0] as aof_flow_batch_device wrote them; d_subdirs: [n_pairs][nb0] or NULL; d_flows: [n_pairs], the
 * pairs' records (read for pred_x / pred_y); d_fields: [n_pairs], written.  Only enqueues on `stream`: no allocation, no
 * host synchronisation, capturable; the inputs are only read.  -EINVAL with nothing enqueued: NULL ctx, fp, d_blocks,
 * d_flows or d_fields, n_pairs < 0 or >= 2^31, parameters outside the ranges above, a geometry aof_field_supported refuses,
 * d_blocks or d_flows not 4-byte aligned, d_fields not 8-byte aligned; -EIO: the context's sticky fault. */
int aof_field_batch_device(aof_ctx *ctx, const aof_field_params *fp, const aof_block *d_blocks, const uint8_t *d_subdirs,
                           const aof_flow *d_flows, int64_t n_pairs, aof_field *d_fields, void *stream);
/* The same function on host memory, a plain loop: no device, no context.  -EINVAL as above (alignment aside). */
int aof_field_host(const aof_params *p, const aof_field_params *fp, const aof_block *blocks, const uint8_t *subdirs,
                   const aof_flow *flows, int64_t n_pairs, aof_field *out);

/* ---- the stream bank's motion field: zoom, rotation and centre flow per stream, integrated over the limiter's window ----
 * aof_bank_field_reset_device, aof_bank_field_device and aof_bank_field_host with their two records: declared, with the
 * normative text of the rule, in aof_bank_field.h beside this file, which is part of this header and comes in with it.  It is
 * a file of its own for as long as the Python package does not bind the three calls: the package's EXPORTS is the census of
 * the functions THIS file declares (tests/test_abi.py), and tests/bank_field_rig.py carries their binding until the package
 * takes it over with a re-recorded surface -- then the text moves here. */
#include "aof_bank_field.h"

/* ---- the sequence pipeline's IMU: raw HIGHRES_IMU samples in, gyro sums and the send gates for a whole recording ----
 * The sequence form of the stream bank's IMU call, enqueued behind a records-only sequence call on the same workspace: two
 * calls and one record, declared with their normative text in aof_sequence_imu.h beside this file, which is part of this
 * header and comes in with it.  A file of its own for the reason above: tests/sequence_imu_rig.py carries the binding. */
#include "aof_sequence_imu.h"

/* ---- the sequence pipeline's motion field: zoom, rotation and centre flow per published message of a recording ----
 * The sequence form of the stream bank's motion field, enqueued behind a sequence call on the same workspace: two calls over
 * the records above, declared with their normative text in aof_sequence_field.h beside this file, which is part of this
 * header and comes in with it.  A file of its own for the reason above: tests/sequence_field_rig.py carries the binding. */
#include "aof_sequence_field.h"

/* ---- the sequence pipeline's MAVLink receive: a recorded connection's bytes in, HIGHRES_IMU samples out ----
 * The sequence form of the stream bank's MAVLink receive, enqueued in front of aof_sequence_imu_device: the recorded bytes
 * and the byte count at every frame become that call's samples and sample_end on the device.  Three functions and one
 * record, declared with their normative text in aof_sequence_mavlink_rx.h beside this file, which is part of this header
 * and comes in with it.  A file of its own for the reason above: tests/sequence_rx_rig.py carries the binding. */
#include "aof_sequence_mavlink_rx.h"

/* ---- measurement ----
 * With profiling on, every launch is bracketed by HIP events on the stream it
 * is launched on; the last AOF_PROFILE_RING launches of each kernel are kept.
 * aof_kernel_ms() synchronises on the newest pair and returns its duration;
 * aof_profile_count()/aof_profile_ms() walk the ring (index 0 = oldest kept)
 * so a benchmark can average a kernel over its whole timed region.
 * Turning profiling on resets the ring. */
#define AOF_PROFILE_RING 256
int aof_set_profiling(aof_ctx *ctx, int on);
/* Same, for a subset: bit k of `mask` times kernel id k (events cost a few microseconds of
 * stream serialisation each, so a benchmark times only the kernel it prices). */
int aof_set_profiling_mask(aof_ctx *ctx, uint32_t mask);
int aof_kernel_ms(aof_ctx *ctx, int kernel_id, float *ms);
int aof_profile_count(const aof_ctx *ctx, int kernel_id);
int aof_profile_ms(aof_ctx *ctx, int kernel_id, int index, float *ms);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
