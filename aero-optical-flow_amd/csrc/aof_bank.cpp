// The stream bank (include/aof.h, "a bank of live streams"): S live streams per tick from one device launch.  Host
// side only: the layout and ONE push path (bank_push) behind the four push entry points -- pre-cropped or sensor
// frames, one tick or a burst of K rounds: the argument checks, the path choice and the launches of k_bank.hip /
// k_bank_burst.hip -- the one-launch kernel (with meshes bound: the tick with the warp inside it, k_bank_tick_warp.hip,
// once per round), or per round (the ingest kernel, or with meshes bound the warp kernel of k_bank_warp.hip,)
// aof_flow_batch_device's own plan on (bank frames, new frames) and the commit kernel.  An entry point only packs its
// arguments.  Nothing here allocates or synchronises.
#include <cerrno>
#include <cstdint>
#include <cstring>

#include "aof_bank_args.hpp"
#include "aof_bank_sensor_rule.hpp"
#include "aof_bank_tables.hpp"
#include "aof_engine_args.hpp"
#include "aof_host.hpp"
#include "aof_ingest_args.hpp"
#include "aof_small_plan.hpp"
#include "aof_warp_step.hpp"

using namespace aof;

namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Can the tick with the warp inside it serve the plan `sm`: the plan's verdict, and frames + the mesh's nodes + the
// kernels' static arrays inside kSmallLdsLimit (small_warp_plan_make, next to small_plan_make in aof_small_plan.hpp).
SmallWarpPlan warp_one_launch_fits(const SmallArgs &sm)
{
    return small_warp_plan_make(sm, (int64_t)warp_nodes(sm.l0.w > 0 ? sm.l0.w : 1) * warp_nodes(sm.l0.h > 0 ? sm.l0.h : 1));
}

// Largest bank the one-launch tick kernel serves under aof_set_bank_path(ctx, 0).  Measured (tools/bench_bank.py,
// profiles/bank_tick_sweep.txt; us per tick, one-launch kernel / composed path): PX4 64x64 1 024 streams 13.0 / 17.2,
// 1 536: 16.2 / 18.1, 2 048: 20.8 / 19.2, 4 096: 33.8 / 26.7; 128x128 on two levels 1 024: 39.9 / 48.3, 1 536: 50.1 /
// 54.6, 2 048: 69.5 / 62.3, 4 096: 126.0 / 94.3.  A workgroup per stream wins until the grid is six rounds of the
// device's 256 compute units; beyond that the grouped flow kernels make up for the commit kernel's second pass over
// the new frames.  (Flow alone crosses at 128 pairs, kSmallMaxPairs of aof_batch_plan.hpp: the tick's write-back and tail
// ride along in the one launch and cost a launch and a pass of their own on the composed path.)
constexpr int32_t kBankFusedMaxStreams = 1536;
// The same for aof_bank_push_camera_device, whose composed path carries a third launch (the ingest kernel into the
// staging region) and a crop written and read again.  Measured (tools/bench_bank.py --camera, legs K1 / K2,
// profiles/bank_camera_tick_sweep.txt; us per tick, one-launch kernel / composed path): 320x240 -> PX4 64x64 1 024
// streams 16.4 / 25.8, 1 536: 19.9 / 28.7, 2 048: 25.4 / 30.5, 3 072: 32.1 / 40.5, 4 096: 40.7 / 45.0; 640x480 -> 128x128 on
// two levels 1 024: 44.1 / 63.1, 1 536: 55.7 / 71.5, 2 048: 74.9 / 80.8, 3 072: 103.2 / 107.5, 4 096: 133.9 / 127.9.  (With the
// plain tick's 1 536 the library's own choice lost 18 % and 7 % at 2 048 streams.)  The two-level configuration crosses
// between 3 072 and 4 096 streams, the small frames beyond 4 096; 3 072 was measured only in the sweep that ran with this
// constant at 2 048, which therefore stays: the largest size at which the library's own choice was measured and tested.
constexpr int32_t kBankCameraFusedMaxStreams = 2048;

// The same two for a burst (aof_bank_push_burst_device / aof_bank_push_camera_burst_device).  A burst workgroup lives K
// times as long as a tick workgroup and, with the loop over the rounds, needs 128 VGPRs where the tick needs 77: four
// workgroups per compute unit instead of six, so the one-launch burst falls off at 1 536 streams of 64x64, where the
// tick still holds.  Measured (tools/bench_bank.py --burst 2,5,16, legs B1 / B2, profiles/bank_burst_sweep.txt; us per
// burst of K = 5 rounds, one-launch kernel / composed path): PX4 64x64 1 024 streams 70.4 / 87.9, 1 536: 116.8 / 92.4,
// 2 048: 135.7 / 98.6; 128x128 on two levels 1 024: 191.7 / 245.2, 1 536: 240.8 / 276.0, 2 048: 325.3 / 304.8 (K = 2 and
// K = 16 cross at the same sizes).  1 024 is the largest swept size at which the one-launch burst wins in both
// configurations; the two-level configuration gives up 13 % at 1 536 streams for it.
constexpr int32_t kBankBurstFusedMaxStreams = 1024;
// Camera form (legs B1 / B2 of the same file, K = 5): 320x240 -> PX4 64x64 1 024 streams 78.1 / 122.4, 1 536: 131.2 /
// 136.1, 2 048: 148.8 / 145.4, 4 096: 286.8 / 211.2; 640x480 -> 128x128 on two levels 1 536: 263.8 / 343.1, 2 048: 355.9 /
// 390.1, 4 096: 685.5 / 633.9.  (K = 2: 64x64 1 536: 53.4 / 54.6, 2 048: 62.0 / 58.1; K = 16: 1 536: 396.2 / 436.7, 2 048:
// 503.6 / 471.5.)  The small frames cross between 1 536 and 2 048 streams at every K; the two-level configuration
// gives up 9 % at 2 048 for it.
constexpr int32_t kBankCameraBurstFusedMaxStreams = 1536;
// The same for a camera push with meshes bound (aof_set_bank_warps), tick or burst: the one-launch form is the tick with
// the warp inside it (k_bank_tick_warp.hip; a burst of K rounds is K launches of it on either path, so the tick's crossover
// is the burst's), the composed form three launches per round.  Measured (tools/bench_bank.py --warp, 640x480 frames, a
// barrel lens; profiles/bank_warp_one_launch_ab.txt; us per tick, leg W: this kernel / leg L of the build before it, the
// composed path, loaded in the same session: median (p10)): PX4 64x64 64 streams 17.1 / 23.8 (23.7), 256: 17.3 / 30.4
// (30.2), 1 024: 30.4 / 43.7 (43.7), 2 048: 56.2 / 60.0 (59.7), 4 096: 89.2 / 95.2 (95.1); 128x128 on two levels 64: 33.8 /
// 46.2 (46.2), 256: 34.9 / 73.2 (73.0), 1 024: 81.0 / 96.6 (96.4), 2 048: 135.8 / 137.2 (137.1), 4 096: 262.6 / 236.9
// (236.9).  2 048 is the largest swept size at which W is below the p10 of L in both configurations -- by 0.9 % on the
// two-level one, where identity meshes (WI 147.0) already lose 7 %: the gather's cost follows the mesh a little, the
// composed path's does not.  Bursts of K = 5 (WB1 / WB2 of this build) cross at the same place: 681.2 / 682.0 at 2 048,
// 1 308.7 / 1 178.6 at 4 096.
constexpr int32_t kBankWarpFusedMaxStreams = 2048;
// The four by form: [sensor frames][burst].
constexpr int32_t kFusedMaxStreams[2][2] = {{kBankFusedMaxStreams, kBankBurstFusedMaxStreams},
                                            {kBankCameraFusedMaxStreams, kBankCameraBurstFusedMaxStreams}};

}  // namespace

// (declared in aof_bank_args.hpp: the stream bank's motion field, aof_bank_field.cpp, finds the scratch region with it)
int aof::bank_layout(const aof_params *p, const aof_bank_params *bp, BankLayout *L)
{
    if (!p || !bp) return -EINVAL;
    const int rc = aof_params_check(p);
    if (rc) return rc;
    if (bp->n_streams < 1) return -EINVAL;
    const int64_t frame = (int64_t)p->width * p->height;
    const int64_t stride = bp->frame_stride ? bp->frame_stride : frame;
    if (stride < frame || (bp->frame_stride && stride % 16)) return -EINVAL;
    if (!(bp->focal_x > 0.0f) || !(bp->focal_y > 0.0f)) return -EINVAL;
    aof_ws_layout W;
    const int rw = aof_workspace_layout(p, bp->n_streams, &W);
    if (rw) return rw;
    const size_t S = (size_t)bp->n_streams;
    std::memset(L, 0, sizeof(*L));
    size_t off = 0;
    L->pub.frames = off;  off = align_up(off + S * (size_t)stride, 256);
    L->pub.state = off;   off = align_up(off + S * sizeof(BankState), 256);
    L->pub.scratch = off; off = align_up(off + W.total_bytes, 256);
    L->flows = off;       off = align_up(off + S * sizeof(aof_flow), 256);
    L->pub.total_bytes = off;
    L->flow_ws_bytes = W.total_bytes;
    L->stride = stride;
    L->frame = frame;
    return 0;
}

namespace {

// The bank layout plus the staging region of the camera push; also everything about `cam` that needs no context.
int camera_layout(const aof_params *p, const aof_bank_params *bp, const aof_bank_camera *cam, BankLayout *L)
{
    if (!cam) return -EINVAL;
    const int rc = bank_layout(p, bp, L);
    if (rc) return rc;
    const aof_ingest_params &g = cam->ingest;
    if (g.crop_width != p->width || g.crop_height != p->height) return -EINVAL;
    if (g.crop_width > g.camera_width || g.crop_height > g.camera_height) return -EINVAL;
    if (cam->camera_stride && cam->camera_stride < (int64_t)g.camera_width * g.camera_height) return -EINVAL;
    const size_t S = (size_t)bp->n_streams;
    size_t off = L->pub.total_bytes;
    L->staging = off;
    L->staging_hist = align_up(off + S * (size_t)L->stride, 256);
    L->pub.total_bytes = align_up(L->staging_hist + S * AOF_EXPOSURE_BINS * sizeof(uint32_t), 256);
    return 0;
}

// Everything all entry points check about the bank itself (cam: the camera push, whose bank has a staging region).
int check_bank(aof_ctx *ctx, const aof_bank_params *bp, const void *d_bank, size_t bank_bytes, BankLayout *L,
               const aof_bank_camera *cam = nullptr, bool camera = false)
{
    if (!ctx) return -EINVAL;
    aof_params p;
    int rc = aof_get_params(ctx, &p);
    if (rc) return rc;
    if (!bp) return ctx_fail(ctx, -EINVAL, "null bank parameters");
    if (camera && !cam) return ctx_fail(ctx, -EINVAL, "null bank camera parameters");
    rc = camera ? camera_layout(&p, bp, cam, L) : bank_layout(&p, bp, L);
    if (rc) return ctx_fail(ctx, rc, camera ? "bad bank parameters (n_streams, frame_stride, focal length) or bank camera parameters (crop, camera_stride)"
                                            : "bad bank parameters (n_streams, frame_stride, focal length)");
    if (!d_bank) return ctx_fail(ctx, -EINVAL, "null bank pointer");
    if (!aligned(d_bank, 256)) return ctx_fail(ctx, -EINVAL, "bank must be 256-byte aligned");
    if (bank_bytes < L->pub.total_bytes)
        return ctx_fail(ctx, -ENOSPC, camera ? "bank smaller than aof_bank_camera_layout().total_bytes" : "bank smaller than aof_bank_layout().total_bytes");
    return 0;
}

// What the plain and the camera push check about their shared arguments.
int check_tick(aof_ctx *ctx, const void *d_frames, const uint64_t *d_time_us, const aof_gyro *d_gyro, const aof_tick_record *d_records,
               const uint8_t *d_mavlink, const uint8_t *d_mavlink_len)
{
    if (!d_frames || !d_time_us || !d_records) return ctx_fail(ctx, -EINVAL, "null frame, time stamp or record pointer");
    if (d_mavlink && !d_mavlink_len) return ctx_fail(ctx, -EINVAL, "MAVLink frames need their length array");
    if (!aligned(d_time_us, 8) || !aligned(d_records, 4) || !aligned(d_gyro, 4))
        return ctx_fail(ctx, -EINVAL, "time stamps must be 8-byte aligned, records and gyro samples 4-byte aligned");
    return 0;
}

// The tick's arguments for the kernels of k_bank.hip (frames: the caller's tick buffer, or the staging region).
BankArgs bank_args(const aof_bank_params *bp, const BankLayout &L, uint8_t *bank, const uint8_t *frames, const uint64_t *d_time_us,
                   const uint8_t *d_active, const aof_gyro *d_gyro, aof_tick_record *d_records, uint8_t *d_mavlink,
                   uint8_t *d_mavlink_len, const aof_bank_stream *d_streams)
{
    BankArgs a;
    std::memset(&a, 0, sizeof(a));   // (cam.camera == nullptr: a plain tick)
    a.n_streams = bp->n_streams;
    a.frame_stride = L.stride;
    a.frame_bytes = L.frame;
    a.frames = frames;
    a.time_us = d_time_us;
    a.active = d_active;
    a.gyro = d_gyro;
    a.bank_frames = bank + L.pub.frames;
    a.state = reinterpret_cast<BankState *>(bank + L.pub.state);
    a.flows = reinterpret_cast<aof_flow *>(bank + L.flows);
    a.output_rate = bp->output_rate;
    a.period_us = limiter_period_us(bp->output_rate);
    a.focal_x = bp->focal_x; a.focal_y = bp->focal_y;
    a.offset_timestamp_usec = bp->offset_timestamp_usec;
    a.system_id = bp->system_id; a.component_id = bp->component_id; a.first_seq = bp->first_seq;
    a.streams = d_streams;           // (bound: the kernels take the six values above from record s instead)
    a.records = d_records;
    a.mavlink = d_mavlink;
    a.mavlink_len = d_mavlink_len;
    return a;
}

// What the camera forms add to the tick's arguments: the crop rectangle, the exposure mask, the outputs.
void camera_args(BankArgs *args, const aof_bank_camera *cam, const uint8_t *d_camera, const uint32_t *hist,
                 aof_exposure_record *d_exposure, float *d_derotated)
{
    BankArgs &a = *args;
    const aof_ingest_params &g = cam->ingest;
    const int x0 = g.camera_width / 2 - g.crop_width / 2, y0 = g.camera_height / 2 - g.crop_height / 2;   // mainloop.cpp:295-296
    a.cam.camera = d_camera;
    a.cam.camera_stride = cam->camera_stride ? cam->camera_stride : (int64_t)g.camera_width * g.camera_height;
    a.cam.pitch = g.camera_width;
    a.cam.origin = y0 * g.camera_width + x0;
    a.cam.crop_w = g.crop_width; a.cam.crop_h = g.crop_height;
    const int mx0 = g.crop_width / 2 - AOF_EXPOSURE_MASK_SIZE / 2, my0 = g.crop_height / 2 - AOF_EXPOSURE_MASK_SIZE / 2;   // :203-206
    a.cam.mx0 = mx0 < 0 ? 0 : mx0; a.cam.my0 = my0 < 0 ? 0 : my0;
    a.cam.mx1 = mx0 + AOF_EXPOSURE_MASK_SIZE > g.crop_width ? g.crop_width : mx0 + AOF_EXPOSURE_MASK_SIZE;
    a.cam.my1 = my0 + AOF_EXPOSURE_MASK_SIZE > g.crop_height ? g.crop_height : my0 + AOF_EXPOSURE_MASK_SIZE;
    a.cam.hist = hist;
    a.cam.exposure = d_exposure;
    a.cam.interval_us = cam->exposure_interval_us;
    a.cam.derotated = cam->derotate ? d_derotated : nullptr;
    a.cam.derotate = cam->derotate_params;
}

// What a burst adds to the checks of a tick.  round: bytes of one round of the frame buffer.
int check_burst(aof_ctx *ctx, const aof_bank_burst *burst, int64_t round, bool pitched, int64_t *round_stride)
{
    if (!burst) return ctx_fail(ctx, -EINVAL, "null bank burst parameters");
    if (burst->n_rounds < 1 || burst->n_rounds > AOF_BANK_BURST_MAX)
        return ctx_fail(ctx, -EINVAL, "bank burst: n_rounds outside 1..AOF_BANK_BURST_MAX");
    const int64_t stride = burst->round_stride ? burst->round_stride : round;
    if (stride < round || (!pitched && stride % 16))
        return ctx_fail(ctx, -EINVAL, "bank burst: round_stride must hold one round (pre-cropped frames: and be a multiple of 16)");
    *round_stride = stride;
    return 0;
}

// Round k of a burst as a tick of its own (the composed path): every per-round pointer moved k rounds on.
BankArgs round_args(const BankArgs &a, int k, const uint8_t *frames)
{
    BankArgs r = a;
    const size_t o = (size_t)k * (size_t)a.n_streams;
    r.frames = frames;
    r.time_us = a.time_us + o;
    r.active = nullptr;
    if (a.gyro) r.gyro = a.gyro + o;
    r.records = a.records + o;
    if (a.mavlink) r.mavlink = a.mavlink + o * AOF_SEQ_FRAME_BYTES;
    if (a.mavlink_len) r.mavlink_len = a.mavlink_len + o;
    if (a.cam.exposure) r.cam.exposure = a.cam.exposure + o;
    if (a.cam.derotated) r.cam.derotated = a.cam.derotated + 2 * o;
    return r;
}

// What the four push entry points differ in.  `camera` / `burst` name the form; the form's own parameter block may
// still be NULL and is refused where the order of the checks has it.
struct Push {
    bool camera, burst;                  // sensor frames (else pre-cropped frames); K rounds (else one tick)
    const aof_bank_camera *cam;          // camera forms
    const aof_bank_burst *rounds;        // burst forms
    const uint8_t *src;                  // the caller's frames: pre-cropped or sensor frames, round 0
    const uint64_t *time_us;
    const uint8_t *select;               // per stream: d_active of a tick, d_count of a burst (or NULL: every stream, every round)
    const aof_gyro *gyro;
    aof_tick_record *records;
    aof_exposure_record *exposure;       // camera forms, optional
    float *derotated;                    // camera forms, needed iff cam->derotate
    uint8_t *mavlink, *mavlink_len;
};

// The one push path behind aof_bank_push_device, _camera_device, _burst_device and _camera_burst_device: the checks in
// their order, the kernels' arguments, the path choice and the launches.  A tick is a burst of one round that keeps its
// `active` mask and has no `count`.
int bank_push(aof_ctx *ctx, const aof_bank_params *bp, void *d_bank, size_t bank_bytes, const Push &p, void *stream)
{
    BankLayout L;
    int rc = check_bank(ctx, bp, d_bank, bank_bytes, &L, p.cam, p.camera);
    if (rc) return rc;
    int64_t round_stride = 0;
    if (p.burst) {
        // one round: S pre-cropped frames frame_stride apart (16-byte chunks), or S sensor frames camera_stride apart (any byte)
        int64_t frame = L.stride;
        if (p.camera) frame = p.cam->camera_stride ? p.cam->camera_stride : (int64_t)p.cam->ingest.camera_width * p.cam->ingest.camera_height;
        if ((rc = check_burst(ctx, p.rounds, (int64_t)bp->n_streams * frame, p.camera, &round_stride))) return rc;
    }
    if ((rc = check_tick(ctx, p.src, p.time_us, p.gyro, p.records, p.mavlink, p.mavlink_len))) return rc;
    if (p.camera) {
        if (p.cam->derotate && !p.derotated) return ctx_fail(ctx, -EINVAL, "bank camera: derotate needs d_derotated");
        if (!aligned(p.exposure, 4) || !aligned(p.derotated, 4))
            return ctx_fail(ctx, -EINVAL, "bank camera: exposure records and de-rotated pairs must be 4-byte aligned");
    }
    // the bound per-stream arrays this push uses (aof_bank_tables.hpp)
    BankCtx &bc = bank_ctx(ctx);
    BankTablesUsed tables;
    if (const char *what = bank_tables_for_push(bc.tables, bp->n_streams, p.camera, round_stride, &tables))
        return ctx_fail(ctx, -EINVAL, what);
    // the meshes, if the push is on sensor frames and some are bound (aof_set_bank_warps)
    const aof_warp_point *warps = nullptr;
    if (p.camera)
        if (const char *what = bank_warps_for_push(bc.warps, bp->n_streams, tables, &warps)) return ctx_fail(ctx, -EINVAL, what);
    // before the first launch: a faulted or wedged context, or a thread on another device, must not touch the bank
    if ((rc = precheck(ctx))) return rc;

    uint8_t *bank = static_cast<uint8_t *>(d_bank);
    uint8_t *staging = bank + L.staging;                                     // (camera forms only)
    uint32_t *hist = reinterpret_cast<uint32_t *>(bank + L.staging_hist);
    // what the flow kernels pair with the stored frames: the caller's frames, or the crops in the staging region
    const uint8_t *cur = p.camera ? staging : p.src;
    BankArgs a = bank_args(bp, L, bank, cur, p.time_us, p.burst ? nullptr : p.select, p.gyro, p.records, p.mavlink, p.mavlink_len,
                           tables.streams);
    if (p.camera) camera_args(&a, p.cam, p.src, hist, p.exposure, p.derotated);
    // (bound: the kernels that take this argument read the crop's place, pitch and origin from record s instead)
    const BankSensors sen = bank_sensors_of_round(tables, 0);
    aof_flow *flows = reinterpret_cast<aof_flow *>(bank + L.flows);
    const BankBurst b = {p.burst ? p.rounds->n_rounds : 1, round_stride, p.burst ? p.select : nullptr};

    // which path: the one-launch kernel where the configuration (and these buffers) allow it and the bank is small
    // enough for a workgroup per stream to pay, or because the caller asked for it.  With warps bound the one-launch
    // kernel is the tick with the warp inside it, which also needs the mesh's nodes in LDS (warp_one_launch_fits)
    const int path = bc.path;
    SmallArgs sm;
    const bool fused = path != 2 &&
                       plan_small_batch(ctx, a.bank_frames, cur, L.stride, bp->n_streams, flows, bank + L.pub.scratch, &sm) &&
                       (!warps || warp_one_launch_fits(sm).ok) &&
                       (path == 1 || bp->n_streams <= (warps ? kBankWarpFusedMaxStreams : kFusedMaxStreams[p.camera][p.burst]));
    if (fused && warps) {
        // a round is one launch; the staging region is neither read nor written
        for (int k = 0; k < b.n_rounds; k++) {
            const uint64_t base = (uint64_t)k * (uint64_t)round_stride;
            BankArgs r = a;   // (a tick keeps its `active` mask: round_args drops it for the burst's `count`)
            if (p.burst) r = round_args(a, k, staging);
            r.cam.camera = p.src + (int64_t)k * round_stride;
            if (launch_bank_tick_warped(sm, r, bank_sensors_of_round(tables, base), warps, p.cam->ingest.camera_height, stream, b.count,
                                        b.count ? k : 0))
                return ctx_fail(ctx, -EIO, "bank warped tick launch failed");
        }
        bc.last_path = 1;
        return 0;
    }
    if (fused) {
        if (p.burst ? launch_bank_burst(sm, a, b, stream, sen) : launch_bank_tick(sm, a, stream, sen))
            return ctx_fail(ctx, -EIO, p.burst ? "bank burst launch failed" : "bank tick launch failed");
        bc.last_path = 1;
        return 0;
    }
    // composed, per round and in order on the one stream: (camera forms) the crops and raw histograms of all S sensor
    // frames into the staging region; the flows of (stored frame, new frame) for all S streams -- those of idle and
    // first-frame streams are cropped, computed and ignored --; then the tails and the masked copy
    for (int k = 0; k < b.n_rounds; k++) {
        const uint8_t *src = p.src + (int64_t)k * round_stride;
        const uint64_t base = (uint64_t)k * (uint64_t)round_stride;
        BankArgs r = a;   // (a tick keeps its `active` mask: round_args drops it for the burst's `count`)
        if (p.burst) r = round_args(a, k, p.camera ? staging : src);
        if (p.camera) {
            r.cam.camera = src;
            if (warps) {   // the warped crops (and the plain ones of unwarped streams) in place of the ingest kernel's
                WarpArgs w = {};
                w.crop_w = p.cam->ingest.crop_width; w.crop_h = p.cam->ingest.crop_height;
                w.camera = src;
                w.recs = tables.sensors; w.base = base; w.camera_bytes = tables.camera_bytes; w.formats = tables.formats;
                w.camera_stride = a.cam.camera_stride;
                w.plane_w = p.cam->ingest.camera_width; w.plane_h = p.cam->ingest.camera_height;
                w.points = warps;
                w.cropped = staging; w.cropped_stride = L.stride;
                w.hist = p.exposure ? hist : nullptr;
                if (launch_warp(w, bp->n_streams, stream)) return ctx_fail(ctx, -EIO, "bank camera warp launch failed");
            } else if (launch_ingest(p.cam->ingest, src, a.cam.camera_stride, bp->n_streams, staging, L.stride, p.exposure ? hist : nullptr, stream,
                              ingest_sensors_of_round(tables, base)))
                return ctx_fail(ctx, -EIO, "bank camera ingest launch failed");
        }
        rc = aof_flow_batch_device(ctx, a.bank_frames, r.frames, L.stride, bp->n_streams, nullptr, nullptr, flows,
                                   bank + L.pub.scratch, L.flow_ws_bytes, stream);
        if (rc) return rc;
        if (launch_bank_commit(r, stream, b.count, b.count ? k : 0, bank_sensors_of_round(tables, base))) return ctx_fail(ctx, -EIO, "bank commit launch failed");
    }
    bc.last_path = 2;
    return 0;
}

// The four binding calls: the rules are bank_tables_bind's (aof_bank_tables.hpp); a refused call leaves the binding as it was.
int bind_table(aof_ctx *ctx, BankTable which, const void *array, int32_t n_streams, uint64_t camera_bytes = 0)
{
    if (!ctx) return -EINVAL;
    if (const char *what = bank_tables_bind(&bank_ctx(ctx).tables, which, array, n_streams, camera_bytes)) return ctx_fail(ctx, -EINVAL, what);
    return 0;
}

}  // namespace

extern "C" {

int aof_bank_layout(const aof_params *p, const aof_bank_params *bp, struct aof_bank_layout *out)
{
    if (!out) return -EINVAL;
    BankLayout L;
    const int rc = bank_layout(p, bp, &L);
    if (rc) return rc;
    *out = L.pub;
    return 0;
}

int aof_set_bank_path(aof_ctx *ctx, int path)
{
    if (!ctx || path < 0 || path > 2) return -EINVAL;
    bank_ctx(ctx).path = path;
    return 0;
}

int aof_bank_last_path(const aof_ctx *ctx)
{
    if (!ctx) return -EINVAL;
    return bank_ctx(const_cast<aof_ctx *>(ctx)).last_path;
}

int aof_bank_warp_one_launch(const aof_params *p, int64_t *lds_bytes)
{
    if (!p) return -EINVAL;
    SmallArgs sm;
    const bool small = plan_small_params(p, &sm);
    const SmallWarpPlan plan = warp_one_launch_fits(sm);
    if (lds_bytes) *lds_bytes = (int64_t)plan.lds;
    return small && plan.ok ? 1 : 0;
}

int aof_bank_warp_crossover(void) { return kBankWarpFusedMaxStreams; }

int aof_bank_stream_from_params(const aof_bank_params *bp, aof_bank_stream *out)
{
    if (!bp || !out) return -EINVAL;
    std::memset(out, 0, sizeof(*out));
    out->focal_x = bp->focal_x; out->focal_y = bp->focal_y;
    out->output_rate = bp->output_rate;
    out->system_id = bp->system_id; out->component_id = bp->component_id; out->first_seq = bp->first_seq;
    out->offset_timestamp_usec = bp->offset_timestamp_usec;
    return 0;
}

int aof_set_bank_streams(aof_ctx *ctx, const aof_bank_stream *d_streams, int32_t n_streams)
{
    return bind_table(ctx, kBankStreams, d_streams, n_streams);
}

int aof_set_bank_sensors(aof_ctx *ctx, const aof_bank_sensor *d_sensors, int32_t n_streams, uint64_t camera_bytes)
{
    return bind_table(ctx, kBankSensors, d_sensors, n_streams, camera_bytes);
}

int aof_set_bank_pixel_formats(aof_ctx *ctx, const uint8_t *d_formats, int32_t n_streams)
{
    return bind_table(ctx, kBankFormats, d_formats, n_streams);
}

int aof_set_bank_binning(aof_ctx *ctx, const uint8_t *d_bins, int32_t n_streams)
{
    return bind_table(ctx, kBankBins, d_bins, n_streams);
}

int aof_bank_sensor_centred_binned(const aof_params *p, uint64_t offset, int32_t pitch, int32_t width, int32_t height, uint8_t format,
                                   uint8_t bin, aof_bank_sensor *out)
{
    if (!p || !out) return -EINVAL;
    if (bin != 1 && bin != 2 && bin != 4) return -EINVAL;
    aof_bank_sensor rec = {};
    rec.offset = offset;
    rec.pitch = pitch;
    rec.width = width; rec.height = height;
    rec.x0 = width / 2 - (int32_t)((int64_t)bin * p->width / 2); rec.y0 = height / 2 - (int32_t)((int64_t)bin * p->height / 2);
    const BankPixelLayout l = bank_pixel_layout(format);
    if (l.group_px > 1 && rec.x0 > 0) rec.x0 -= rec.x0 % l.group_px;   // (a packed form's crop starts on a group)
    // (the rule against a buffer that ends with the frame: everything but the place in a camera buffer)
    if (p->width < 1 || p->height < 1 || width < 1 || height < 1 ||
        !bank_sensor_valid_format(0, pitch, width, height, rec.x0, rec.y0, p->width, p->height, 0, UINT64_MAX, format, bin))
        return -EINVAL;
    *out = rec;
    return 0;
}

int aof_bank_sensor_centred(const aof_params *p, uint64_t offset, int32_t pitch, int32_t width, int32_t height, aof_bank_sensor *out)
{
    if (!p || !out) return -EINVAL;
    if (p->width < 1 || p->height < 1 || pitch < width || p->width > width || p->height > height) return -EINVAL;
    std::memset(out, 0, sizeof(*out));
    out->offset = offset;
    out->pitch = pitch;
    out->width = width; out->height = height;
    out->x0 = width / 2 - p->width / 2; out->y0 = height / 2 - p->height / 2;   // mainloop.cpp:295-296
    return 0;
}

int aof_bank_sensor_from_camera(const aof_params *p, const aof_bank_camera *cam, int32_t stream, aof_bank_sensor *out)
{
    if (!p || !cam || !out || stream < 0) return -EINVAL;
    const aof_ingest_params &g = cam->ingest;
    if (g.camera_width < 1 || g.camera_height < 1 || cam->camera_stride < 0) return -EINVAL;
    const uint64_t stride = cam->camera_stride ? (uint64_t)cam->camera_stride : (uint64_t)g.camera_width * (uint64_t)g.camera_height;
    return aof_bank_sensor_centred(p, (uint64_t)stream * stride, g.camera_width, g.camera_width, g.camera_height, out);
}

int aof_bank_sensor_valid_binned(const aof_bank_sensor *rec, uint8_t format, uint8_t bin, int32_t crop_width, int32_t crop_height,
                                 uint64_t base, uint64_t camera_bytes)
{
    if (!rec) return -EINVAL;
    return bank_sensor_valid_format(rec->offset, rec->pitch, rec->width, rec->height, rec->x0, rec->y0, crop_width, crop_height, base,
                                    camera_bytes, format, bin) ? 1 : 0;
}

int aof_bank_pixel_row_bytes(uint8_t format, int32_t width, int64_t *out)
{
    const BankPixelLayout l = bank_pixel_layout(format);
    if (!out || l.group_px == 0 || width < 1 || width % l.group_px != 0) return -EINVAL;
    *out = (int64_t)(width / l.group_px) * l.group_bytes;
    return 0;
}

int aof_bank_sensor_valid_format(const aof_bank_sensor *rec, uint8_t format, int32_t crop_width, int32_t crop_height, uint64_t base,
                                 uint64_t camera_bytes)
{
    return aof_bank_sensor_valid_binned(rec, format, 1, crop_width, crop_height, base, camera_bytes);
}

int aof_bank_sensor_valid(const aof_bank_sensor *rec, int32_t crop_width, int32_t crop_height, uint64_t base, uint64_t camera_bytes)
{
    return aof_bank_sensor_valid_format(rec, AOF_PIXEL_GREY8, crop_width, crop_height, base, camera_bytes);
}

int aof_ingest_sensors_binned_device(int32_t crop_width, int32_t crop_height, const uint8_t *d_camera, uint64_t camera_bytes,
                                     const aof_bank_sensor *d_sensors, const uint8_t *d_formats, const uint8_t *d_bins, int64_t n_frames,
                                     uint8_t *d_cropped, int64_t cropped_stride, uint32_t *d_hist, uint8_t *d_ok, void *stream)
{
    if (crop_width < 1 || crop_height < 1 || n_frames < 0) return -EINVAL;
    if (n_frames == 0) return 0;
    if (!d_camera || !d_sensors || !aligned(d_sensors, 16) || camera_bytes == 0 || (!d_cropped && !d_hist)) return -EINVAL;
    if (d_cropped && cropped_stride < (int64_t)crop_width * crop_height && n_frames > 1) return -EINVAL;
    if (n_frames * ((crop_height + 15) / 16) > 0x7FFFFFFF) return -EINVAL;
    const aof_ingest_params g = {crop_width, crop_height, crop_width, crop_height};   // (the sensor size: the records')
    const BankTablesUsed tables = {nullptr, d_sensors, camera_bytes, d_formats, d_bins};
    return launch_ingest(g, d_camera, 0, n_frames, d_cropped, cropped_stride, d_hist, stream, ingest_sensors_of_round(tables, 0, d_ok)) ? -EIO : 0;
}

int aof_ingest_sensor_formats_device(int32_t crop_width, int32_t crop_height, const uint8_t *d_camera, uint64_t camera_bytes,
                                     const aof_bank_sensor *d_sensors, const uint8_t *d_formats, int64_t n_frames, uint8_t *d_cropped,
                                     int64_t cropped_stride, uint32_t *d_hist, uint8_t *d_ok, void *stream)
{
    return aof_ingest_sensors_binned_device(crop_width, crop_height, d_camera, camera_bytes, d_sensors, d_formats, nullptr, n_frames,
                                            d_cropped, cropped_stride, d_hist, d_ok, stream);
}

int aof_ingest_sensors_device(int32_t crop_width, int32_t crop_height, const uint8_t *d_camera, uint64_t camera_bytes,
                              const aof_bank_sensor *d_sensors, int64_t n_frames, uint8_t *d_cropped, int64_t cropped_stride,
                              uint32_t *d_hist, uint8_t *d_ok, void *stream)
{
    return aof_ingest_sensor_formats_device(crop_width, crop_height, d_camera, camera_bytes, d_sensors, nullptr, n_frames, d_cropped,
                                            cropped_stride, d_hist, d_ok, stream);
}

int aof_bank_reset_device(aof_ctx *ctx, const aof_bank_params *bp, const uint8_t *d_mask, void *d_bank, size_t bank_bytes,
                          void *stream)
{
    BankLayout L;
    int rc = check_bank(ctx, bp, d_bank, bank_bytes, &L);
    if (rc) return rc;
    if ((rc = precheck(ctx))) return rc;
    uint8_t *bank = static_cast<uint8_t *>(d_bank);
    if (launch_bank_reset(reinterpret_cast<BankState *>(bank + L.pub.state), d_mask, bp->n_streams, stream))
        return ctx_fail(ctx, -EIO, "bank reset launch failed");
    return 0;
}

int aof_bank_camera_layout(const aof_params *p, const aof_bank_params *bp, const aof_bank_camera *cam,
                           struct aof_bank_layout *out, size_t *staging)
{
    if (!out || !staging) return -EINVAL;
    BankLayout L;
    const int rc = camera_layout(p, bp, cam, &L);
    if (rc) return rc;
    *out = L.pub;
    *staging = L.staging;
    return 0;
}

int aof_bank_push_device(aof_ctx *ctx, const aof_bank_params *bp, const uint8_t *d_frames, const uint64_t *d_time_us,
                         const uint8_t *d_active, const aof_gyro *d_gyro, void *d_bank, size_t bank_bytes,
                         aof_tick_record *d_records, uint8_t *d_mavlink, uint8_t *d_mavlink_len, void *stream)
{
    const Push p = {false, false, nullptr, nullptr, d_frames, d_time_us, d_active, d_gyro, d_records, nullptr, nullptr, d_mavlink, d_mavlink_len};
    return bank_push(ctx, bp, d_bank, bank_bytes, p, stream);
}

int aof_bank_push_camera_device(aof_ctx *ctx, const aof_bank_params *bp, const aof_bank_camera *cam, const uint8_t *d_camera,
                                const uint64_t *d_time_us, const uint8_t *d_active, const aof_gyro *d_gyro, void *d_bank,
                                size_t bank_bytes, aof_tick_record *d_records, aof_exposure_record *d_exposure,
                                float *d_derotated, uint8_t *d_mavlink, uint8_t *d_mavlink_len, void *stream)
{
    const Push p = {true, false, cam, nullptr, d_camera, d_time_us, d_active, d_gyro, d_records, d_exposure, d_derotated, d_mavlink, d_mavlink_len};
    return bank_push(ctx, bp, d_bank, bank_bytes, p, stream);
}

int aof_bank_push_burst_device(aof_ctx *ctx, const aof_bank_params *bp, const aof_bank_burst *burst, const uint8_t *d_frames,
                               const uint64_t *d_time_us, const uint8_t *d_count, const aof_gyro *d_gyro, void *d_bank,
                               size_t bank_bytes, aof_tick_record *d_records, uint8_t *d_mavlink, uint8_t *d_mavlink_len,
                               void *stream)
{
    const Push p = {false, true, nullptr, burst, d_frames, d_time_us, d_count, d_gyro, d_records, nullptr, nullptr, d_mavlink, d_mavlink_len};
    return bank_push(ctx, bp, d_bank, bank_bytes, p, stream);
}

int aof_bank_push_camera_burst_device(aof_ctx *ctx, const aof_bank_params *bp, const aof_bank_camera *cam,
                                      const aof_bank_burst *burst, const uint8_t *d_camera, const uint64_t *d_time_us,
                                      const uint8_t *d_count, const aof_gyro *d_gyro, void *d_bank, size_t bank_bytes,
                                      aof_tick_record *d_records, aof_exposure_record *d_exposure, float *d_derotated,
                                      uint8_t *d_mavlink, uint8_t *d_mavlink_len, void *stream)
{
    const Push p = {true, true, cam, burst, d_camera, d_time_us, d_count, d_gyro, d_records, d_exposure, d_derotated, d_mavlink, d_mavlink_len};
    return bank_push(ctx, bp, d_bank, bank_bytes, p, stream);
}

}  // extern "C"
