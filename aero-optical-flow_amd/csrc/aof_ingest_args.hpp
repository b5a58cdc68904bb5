// From sensor frames to crops: the ingest kernels (k_ingest.hip) and the warp through a lens mesh (k_bank_warp.hip),
// their arguments and launchers.
#pragma once

#include <cstdint>

#include "aof.h"

namespace aof {

// sensors.recs (or nullptr: the kernel without the argument): frame i's place, pitch and crop origin come from record i, valid against camera_bytes with
// `camera` `base` bytes into the caller's buffer (bank_sensor, aof_bank_stream.hpp); p.camera_width / camera_height and
// camera_stride are then not used.  ok: u8 [n_frames] or nullptr, 1 where the record let the frame be read.
struct IngestSensors {
    const aof_bank_sensor *recs;
    uint64_t base, camera_bytes;
    uint8_t *ok;
    const uint8_t *formats;   // [n_frames] AOF_PIXEL_* of frame i, or nullptr: one grey byte per pixel
    const uint8_t *bins;      // [n_frames] binning of frame i (1, 2, 4), or nullptr: 1
};
int launch_ingest(const aof_ingest_params &p, const uint8_t *camera, int64_t camera_stride,
                  int64_t n_frames, uint8_t *cropped, int64_t cropped_stride, uint32_t *hist,
                  void *stream, const IngestSensors &sensors = IngestSensors{nullptr, 0, 0, nullptr, nullptr, nullptr});
// The sequence pipeline's ingest: the same pass also leaves every frame's level-1 image (l1: [n_frames] frames, or
// nullptr) and adds its byte sums to the pixel-sum records of the pairs it belongs to (sums: [n_frames - 1][2][2],
// zeroed here; or nullptr) -- what K1 would otherwise compute in a second pass over the cropped frames.
bool ingest_pyramid_supported(const aof_ingest_params &p, const uint8_t *cropped, int64_t cropped_stride);
int launch_ingest_pyramid(const aof_ingest_params &p, const uint8_t *camera, int64_t camera_stride, int64_t n_frames,
                          uint8_t *cropped, int64_t cropped_stride, uint32_t *hist, uint8_t *l1, uint32_t *sums, void *stream);

// The warp of n_frames crops through their meshes (k_bank_warp.hip; include/aof.h "the stream bank with a lens"): where
// launch_ingest stands in a camera push with aof_set_bank_warps bound, and behind aof_ingest_warped_device.  Frame i's
// plane is record i's (recs, formats, base, camera_bytes as IngestSensors), or with recs == nullptr the grey frame of
// plane_w x plane_h at camera + i * camera_stride (then the crop of an unwarped frame is the centred one).
struct WarpArgs {
    int32_t crop_w, crop_h;
    const uint8_t *camera;
    const aof_bank_sensor *recs;
    uint64_t base, camera_bytes;
    const uint8_t *formats;
    int64_t camera_stride;
    int32_t plane_w, plane_h;
    const aof_warp_point *points;  // [n_frames][ny][nx], 16-byte aligned
    uint8_t *cropped;              // [n_frames] crops cropped_stride apart, or nullptr
    int64_t cropped_stride;
    uint32_t *hist;                // [n_frames][10] raw masked histograms, or nullptr
    uint8_t *ok;                   // u8 [n_frames] or nullptr
    int32_t nstrips, strip_rows, vec, nx, ny;   // filled by the launcher
};
int launch_warp(const WarpArgs &a, int64_t n_frames, void *stream);   // hipErrorInvalidValue: a crop too wide for a strip's nodes

}  // namespace aof
