// The stream bank's tick: the layout of a bank, the arguments of its kernels and their launchers (aof_bank.cpp,
// k_bank.hip, k_bank_burst.hip, k_bank_tick_warp.hip).
#pragma once

#include <cstddef>
#include <cstdint>

#include "aof.h"
#include "aof_engine_args.hpp"   // SmallArgs

namespace aof {

// The stream bank (aof_bank.cpp, k_bank.hip; include/aof.h "a bank of live streams").  Layout of a bank:
//   frames   u8 [S][frame_stride]     the stored (previous) frame of every stream
//   state    BankState [S]            what one facade object keeps between calcFlow() calls, 64 bytes per stream
//   scratch  aof_workspace_layout(p, S) bytes (block records, sub-pixel directions, pixel sums and, on the composed
//            path, everything the batch plan needs), then aof_flow [S]: the tick's pixel records
//   staging  (aof_bank_camera_layout only) u8 [S][frame_stride]: the tick's cropped frames on the composed path of
//            aof_bank_push_camera_device, then u32 [S][10]: their raw exposure histograms
// every region at a multiple of 256 bytes.
struct BankState {
    uint32_t has_prev;         // 0 after a reset: the next frame is the stream's first
    uint32_t time_last_pub;    // OpticalFlow::time_last_pub
    float sum_flow_x, sum_flow_y;   // the limiter's sums (initLimitRate)
    int32_t sum_flow_quality, valid_frame_count;
    double gyro_x, gyro_y, gyro_z;  // summed since the last publication (mainloop.cpp:383-405)
    uint32_t messages;         // records published so far: the next MAVLink sequence number is first_seq + messages
    uint32_t frames;           // frames the stream has been given
    uint64_t next_exposure_us; // aof_bank_push_camera_device: the stream's exposure gate (mainloop.cpp:273-274); 0 after a
                               // reset.  The plain push passes it through.
};
static_assert(sizeof(BankState) == 64, "one bank state record is 64 bytes");
// The regions of a bank (aof_bank.cpp): aof_bank_layout's offsets and what the library keeps to itself.  -EINVAL for
// parameters a push refuses (n_streams, frame_stride, focal lengths), or what aof_params_check / aof_workspace_layout say.
struct BankLayout {
    struct aof_bank_layout pub;
    size_t flow_ws_bytes, flows;   // inside the bank: the engine's workspace is at pub.scratch, the pixel records at `flows`
    int64_t stride, frame;
    size_t staging, staging_hist;  // camera layout only: the tick's cropped frames and their raw histograms
};
int bank_layout(const aof_params *p, const aof_bank_params *bp, BankLayout *L);
// What aof_bank_push_camera_device adds to a tick (include/aof.h, "sensor frames").  camera == nullptr: a plain tick.
struct BankCamera {
    const uint8_t *camera;         // [S] sensor frames, stream s at + s * camera_stride; its crop starts `origin` bytes in
    int64_t camera_stride;
    int32_t pitch, origin;         // bytes between sensor rows; y0 * pitch + x0 of the crop rectangle
    int32_t crop_w, crop_h;
    int32_t mx0, my0, mx1, my1;    // the exposure mask inside the crop (mainloop.cpp:203-206, clipped)
    const uint32_t *hist;          // composed path: [S][10] raw histograms of the tick's crops (k_ingest)
    aof_exposure_record *exposure; // [S] or nullptr (no statistics, the gate does not move)
    uint32_t interval_us;
    float *derotated;              // [S][2] or nullptr
    aof_derotate_params derotate;
};
struct BankArgs {
    int32_t n_streams;
    int64_t frame_stride, frame_bytes;
    const uint8_t *frames;         // the tick's frames, stream s at + s * frame_stride
    const uint64_t *time_us;       // [S]
    const uint8_t *active;         // [S] or nullptr (= all)
    const aof_gyro *gyro;          // [S] or nullptr (zeros)
    uint8_t *bank_frames;          // [S][frame_stride]
    BankState *state;              // [S]
    const aof_flow *flows;         // [S] the tick's pixel records (composed path: written by the batch plan)
    int32_t output_rate;
    float period_us;               // limiter_period_us(output_rate)
    float focal_x, focal_y;
    uint64_t offset_timestamp_usec;
    uint8_t system_id, component_id, first_seq;
    // [S] per-stream values in place of output_rate .. first_seq (aof_set_bank_streams), or nullptr.  Here, beside the
    // scalars it replaces, and not behind `cam`: measured there, the UNBOUND tick lost 0.3 us (LAB_LOG.md, "Stream bank
    // per-stream cameras")
    const aof_bank_stream *streams;
    aof_tick_record *records;      // [S]
    uint8_t *mavlink;              // [S][AOF_SEQ_FRAME_BYTES] or nullptr
    uint8_t *mavlink_len;          // [S]
    BankCamera cam;                // (last: the plain kernels' argument offsets stay)
};
// Per-stream sensor records in place of cam.camera_stride, cam.pitch and cam.origin (aof_set_bank_sensors): a kernel
// argument of its own that only the instantiations for a bound array have -- with nothing bound the launched kernels
// and their BankArgs are the ones without it, argument for argument.  recs: [S]; camera_bytes: what the records are
// valid against; camera_base: bytes between the caller's d_camera and cam.camera (a burst's composed path: round k's
// launches see cam.camera = d_camera + k * round_stride).  recs == nullptr: nothing bound.
// formats: [S] the streams' pixel formats (aof_set_bank_pixel_formats), or nullptr: one grey byte per pixel.
// bins: [S] the streams' binning (aof_set_bank_binning), or nullptr: 1 everywhere.
struct BankSensors {
    const aof_bank_sensor *recs;
    uint64_t camera_bytes, camera_base;
    const uint8_t *formats;
    const uint8_t *bins;
};
// One launch per tick: a workgroup per stream computes the pair with flow_small_pair, runs the stream's tail and
// stores the new frame (sm: the small-pair plan of (bank frames, tick frames), small_plan_make).  With
// a.cam.camera the workgroup fetches the crop's rows from the stream's sensor frame itself (a.frames is not read).
int launch_bank_tick(const SmallArgs &sm, const BankArgs &a, void *stream, const BankSensors &sen = BankSensors{nullptr, 0, 0, nullptr, nullptr});
// Behind aof_flow_batch_device on (bank frames, tick frames): the tail of every stream and the masked copy of the
// active streams' frames into the bank.  With a.cam.camera: a.frames is the staging region, and the exposure gate,
// the exposure record and the de-rotated pair come from here as well.
// A burst's composed path runs it once per round: `a` carries the round's buffers, and stream s is active iff
// round < count[s] (count NULL: a.active decides, as in a tick).
int launch_bank_commit(const BankArgs &a, void *stream, const uint8_t *count = nullptr, int32_t round = 0,
                       const BankSensors &sen = BankSensors{nullptr, 0, 0, nullptr, nullptr});
// K frame rounds per stream (aof_bank_push_burst_device, k_bank_burst.hip).  Round k's frame of stream s sits
// round_stride bytes behind round k - 1's; time_us, gyro, records, mavlink_len, mavlink, cam.exposure and
// cam.derotated of a BankArgs are then dense [K][S] arrays, a.active is not read.
struct BankBurst {
    int32_t n_rounds;              // K, 1..AOF_BANK_BURST_MAX
    int64_t round_stride;          // bytes between the rounds of a.frames (a.cam.camera for the camera form)
    const uint8_t *count;          // [S] frames per stream (values above K count as K), or nullptr (= K)
};
// One launch per burst: a workgroup per stream walks its rounds with one frame resident in LDS (same configuration
// class and same `sm` as launch_bank_tick).
int launch_bank_burst(const SmallArgs &sm, const BankArgs &a, const BankBurst &b, void *stream,
                      const BankSensors &sen = BankSensors{nullptr, 0, 0, nullptr, nullptr});
int launch_bank_reset(BankState *state, const uint8_t *mask, int32_t n_streams, void *stream);
// The one-launch tick with the warp inside it (k_bank_tick_warp.hip): launch_bank_tick's camera form with stream s's mesh
// (points: [S][ny][nx]) in front of the new frame; sen.recs may be nullptr (the plane is then the call's grey frame of
// cam.pitch x plane_h), sen.bins must be.  (count, round): launch_bank_commit's -- a burst's round k is one launch with
// round_args' pointers.  Needs small_warp_plan_make(sm, nodes).ok (aof_small_plan.hpp); the staging region is not touched.
int launch_bank_tick_warped(const SmallArgs &sm, const BankArgs &a, const BankSensors &sen, const aof_warp_point *points, int32_t plane_h,
                            void *stream, const uint8_t *count = nullptr, int32_t round = 0);

}  // namespace aof
