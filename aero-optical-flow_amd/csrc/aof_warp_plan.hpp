// The launch plan of the warp kernel (k_bank_warp.hip: launch_warp calls warp_plan_make and does nothing else on the
// host): the mesh's node counts, the strip of up to 128 rows -- halved while its node rows would not fit 32 KiB of LDS --,
// what the first and the last strip hold, whether a lane makes 16 pixels or one, the dynamic LDS and whether the kernel's
// limit has to be raised for it, whether the histograms are zeroed in front of the launch, and the verdict.  Host only, no
// HIP: tests/native/host_selftest.cpp holds it to the model of tests/warp_plan_ref.py.  The kernel's own address
// arithmetic stays in the kernel.
#pragma once

#include <cstddef>
#include <cstdint>

#include "aof_small_plan.hpp"   // (kThreads, kSmallAttrAbove)
#include "aof_warp_step.hpp"    // (warp_nodes, kWarpCell)

namespace aof {

constexpr int kStripRows = 128;          // (k_ingest's kRowsPerBlock; a multiple of the cell)
constexpr int kNodeBytesWanted = 32768;  // a strip is halved until its nodes fit this ...
constexpr int kNodeBytesMax = 61440;     // ... and a crop whose 8-row strip needs more than this is refused: W >= 30 720
constexpr int kLaneItems = 255;          // 16-pixel items of a lane between two flushes: 255 * 16 < 4096 (12-bit fields)

// Why launch_warp cannot serve a call: the FIRST condition that fails, in the order they are tested.
enum WarpVerdict : int32_t {
    WARP_OK = 0,
    WARP_TOO_WIDE,         // the nodes of an 8-row strip beyond kNodeBytesMax
    WARP_TOO_MANY,         // frames * strips beyond 31 bits of workgroups
};

struct WarpPlan {
    WarpVerdict verdict;
    int32_t nx, ny;                // warp_nodes of the crop's width and height
    int32_t strip_rows, nstrips;   // crop rows of a full strip; strips of a frame
    int32_t rows[2];               // crop rows of the first and of the last strip (one strip: the same)
    int32_t node_rows[2];          // node rows the first and the last strip clamp into LDS
    int64_t node_bytes[2];         // ... and their bytes
    int32_t vec;                   // a lane makes 16 pixels and stores 16 bytes (else: a lane per pixel)
    size_t lds;                    // dynamic LDS bytes of a workgroup: the first strip's nodes
    int32_t attr;                  // the launcher raises the kernel's dynamic-LDS limit first
    int32_t zero_hist;             // several strips add to a frame's histogram: the launcher zeroes the words first
    int64_t items[2];              // items of the first and of the last strip: 16-pixel pieces (vec) or pixels
    int32_t trips[2];              // ... and their rounds of kThreads
    int64_t wgs;                   // workgroups of the launch
};

// cropped: the destination's address (0: none), cropped_stride its bytes between frames; hist: a histogram is asked for.
// Everything is filled whatever the verdict says (the arithmetic of a launch that would run).  crop_w, crop_h >= 1.
inline WarpPlan warp_plan_make(int32_t crop_w, int32_t crop_h, int64_t n_frames, uintptr_t cropped, int64_t cropped_stride, bool hist)
{
    WarpPlan p = {};
    p.nx = warp_nodes(crop_w); p.ny = warp_nodes(crop_h);
    // the strip: k_ingest's 128 rows, halved while its node rows would not fit
    auto node_bytes = [&](int rows) { return (int64_t)(rows / kWarpCell + 1) * p.nx * (int64_t)sizeof(aof_warp_point); };
    p.strip_rows = kStripRows;
    while (p.strip_rows > kWarpCell && node_bytes(p.strip_rows) > kNodeBytesWanted) p.strip_rows /= 2;
    p.nstrips = (crop_h + p.strip_rows - 1) / p.strip_rows;
    p.rows[0] = crop_h < p.strip_rows ? crop_h : p.strip_rows;
    p.rows[1] = crop_h - (p.nstrips - 1) * p.strip_rows;
    p.vec = (crop_w % 16 == 0) && (!cropped || (cropped % 16 == 0 && cropped_stride % 16 == 0));
    for (int i = 0; i < 2; i++) {
        // a strip begins on a cell: the cells its rows touch and one node row behind the last
        p.node_rows[i] = (p.rows[i] - 1) / kWarpCell + 2;
        p.node_bytes[i] = (int64_t)p.node_rows[i] * p.nx * (int64_t)sizeof(aof_warp_point);
        p.items[i] = p.vec ? (int64_t)p.rows[i] * (crop_w / 16) : (int64_t)p.rows[i] * crop_w;
        p.trips[i] = (int32_t)small_plan_trips(p.items[i], kThreads);
    }
    p.lds = (size_t)p.node_bytes[0];
    p.attr = p.lds > kSmallAttrAbove ? 1 : 0;
    p.zero_hist = hist && p.nstrips > 1 ? 1 : 0;
    p.wgs = n_frames * p.nstrips;
    p.verdict = node_bytes(p.strip_rows) > kNodeBytesMax ? WARP_TOO_WIDE : (p.wgs > 0x7FFFFFFF ? WARP_TOO_MANY : WARP_OK);
    return p;
}

}  // namespace aof
