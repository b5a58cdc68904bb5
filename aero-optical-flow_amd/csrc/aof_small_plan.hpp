// The launch plans of the small-pair kernels: the one-workgroup class that runs flow_small_pair (aof_flow_small.hpp:
// k_flow_small, its tagged and resident forms, the stream bank's tick and burst) and the grouped lane-per-block search
// k_flow_lane8 (k_search_lane8.hip launches it).  Host only, no HIP: tests/native/host_selftest.cpp holds both to the
// model of tests/small_plan_ref.py.  The kernels' own address arithmetic stays in the kernels.
#pragma once

#include <cstddef>
#include <cstdint>

#include "aof_engine_args.hpp"

namespace aof {

constexpr int kThreads = 256;
constexpr int kMaxBins = 64;   // n = 2(2R+1)+1: 19 at level 1 (and for one level), 55 at level 0 of two (S = 4)
constexpr int kLoads = 8;      // 16-byte chunks a thread has in flight in pass A
constexpr int kPad = 16;       // bytes after each LDS frame: the dword reads of the last row may run past it
constexpr size_t kSmallStaticLds = 4096;             // room kept for the kernels' static arrays
constexpr size_t kSmallLdsLimit = 160 * 1024;        // dynamic + static
constexpr size_t kSmallAttrAbove = 48 * 1024;        // dynamic LDS beyond this needs the function attribute

// Why flow_small_pair cannot serve a configuration: the FIRST condition that fails, in the order they are tested.
enum SmallVerdict : int32_t {
    SMALL_OK = 0,
    SMALL_NO_LEVELS,       // neither one level nor two
    SMALL_NO_TILE,         // tile != 8 or search != 4
    SMALL_NO_PAIRS,        // no pair, or pair * 256 beyond 31 bits
    SMALL_NO_GRID0,        // level-0 grid of no block or more than 256
    SMALL_NO_BINS0,        // more vote bins at level 0 than the histograms hold
    SMALL_NO_WIDTH,        // w % 16 (16-byte chunks of a contiguous frame)
    SMALL_NO_STRIDE,       // more than one pair and pair_stride % 16
    SMALL_NO_PREV,         // prev off 16 bytes
    SMALL_NO_CUR,          // cur off 16 bytes
    SMALL_NO_SUBDIRS0,     // half-pixel refinement without a place for level 0's directions
    SMALL_NO_HEIGHT,       // two levels: odd height, or level 1 is not half of level 0
    SMALL_NO_GRID1,        // level-1 grid of no block or more than 256
    SMALL_NO_BINS1,        // more vote bins at level 1 than the histograms hold
    SMALL_NO_SUBDIRS1,     // half-pixel refinement without a place for level 1's directions
    SMALL_NO_LDS,          // the frames do not fit LDS beside the static arrays
};

struct SmallPlan {
    SmallVerdict verdict;
    size_t lds;                    // dynamic LDS bytes of a workgroup
    size_t f0[2], f1[2];           // byte offsets of the two level-0 and the two level-1 buffers (f1: two levels)
    int32_t attr;                  // the launcher raises the instantiation's dynamic-LDS limit first
    int32_t trips_a[3];            // pass A, `load` 1, 2, 3: rounds of kLoads * kThreads 16-byte chunks
    int32_t trips_b[2];            // pass B, one buffer / both: rounds of kThreads 8-byte pieces (two levels)
    int32_t trips_c[2];            // pass C per level: rounds of kThreads (block, dy) items
    int32_t trips_d1[2];           // D1 per level: rounds of kThreads lanes, four per block in whole waves (half-pixel)
};

inline int64_t small_plan_trips(int64_t items, int64_t per_trip) { return items <= 0 ? 0 : (items + per_trip - 1) / per_trip; }

// The verdict is today's flow_small_supported, condition by condition; the rest is filled whatever it says (the
// arithmetic of a workgroup that would run), but for the trips of a level whose grid has no block.
inline SmallPlan small_plan_make(const SmallArgs &a)
{
    const SearchArgs &l0 = a.l0, &l1 = a.l1;
    const bool two = a.levels == 2;
    SmallPlan p = {};
    const int64_t w = l0.w > 0 ? l0.w : 0, h = l0.h > 0 ? l0.h : 0;
    const size_t frame0 = (size_t)(w * h), frame1 = (size_t)((w / 2) * (h / 2));
    p.lds = 2 * (frame0 + kPad);
    if (two) p.lds += 2 * ((frame1 + kPad + 15) & ~(size_t)15);
    p.f0[0] = 0;
    p.f0[1] = frame0 + kPad;
    if (two) {
        p.f1[0] = 2 * (frame0 + kPad);
        p.f1[1] = p.f1[0] + ((frame1 + kPad + 15) & ~(size_t)15);
    }
    p.attr = p.lds > kSmallAttrAbove ? 1 : 0;
    const int64_t per_frame = (int64_t)(frame0 / 16);
    p.trips_a[0] = p.trips_a[1] = (int32_t)small_plan_trips(per_frame, kLoads * kThreads);
    p.trips_a[2] = (int32_t)small_plan_trips(2 * per_frame, kLoads * kThreads);
    if (two) {
        const int64_t pieces = (h / 2) * (w / 16);
        p.trips_b[0] = (int32_t)small_plan_trips(pieces, kThreads);
        p.trips_b[1] = (int32_t)small_plan_trips(2 * pieces, kThreads);
    }
    const SearchArgs *lv[2] = {&l0, &l1};
    for (int l = 0; l < (two ? 2 : 1); l++) {
        const int64_t nb = (int64_t)lv[l]->grid.nx * lv[l]->grid.ny;
        if (nb < 1 || nb > kThreads) continue;
        p.trips_c[l] = (int32_t)small_plan_trips(nb * 9, kThreads);
        if (l0.subpixel) p.trips_d1[l] = (int32_t)small_plan_trips((4 * nb + 63) / 64 * 64, kThreads);
    }

    auto verdict = [&]() {
        if (a.levels != 1 && a.levels != 2) return SMALL_NO_LEVELS;
        if (l0.tile != 8 || l0.search != 4) return SMALL_NO_TILE;
        if (l0.n_pairs < 1 || l0.n_pairs > 0x7FFFFFFF / kThreads) return SMALL_NO_PAIRS;
        if (l0.grid.blocks() < 1 || l0.grid.blocks() > kThreads) return SMALL_NO_GRID0;
        if (2 * (2 * a.t0.range + 1) + 1 > kMaxBins) return SMALL_NO_BINS0;
        // 16-byte chunks of a contiguous frame
        if (l0.w % 16) return SMALL_NO_WIDTH;
        if (l0.n_pairs > 1 && l0.pair_stride % 16) return SMALL_NO_STRIDE;
        if (reinterpret_cast<uintptr_t>(l0.prev) % 16) return SMALL_NO_PREV;
        if (reinterpret_cast<uintptr_t>(l0.cur) % 16) return SMALL_NO_CUR;
        if (l0.subpixel && !l0.subdirs) return SMALL_NO_SUBDIRS0;
        if (two) {
            if (l0.h % 2 || l1.w != l0.w / 2 || l1.h != l0.h / 2) return SMALL_NO_HEIGHT;
            if (l1.grid.blocks() < 1 || l1.grid.blocks() > kThreads) return SMALL_NO_GRID1;
            if (2 * (2 * a.t1.range + 1) + 1 > kMaxBins) return SMALL_NO_BINS1;
            if (l0.subpixel && !l1.subdirs) return SMALL_NO_SUBDIRS1;
        }
        return p.lds + kSmallStaticLds <= kSmallLdsLimit ? SMALL_OK : SMALL_NO_LDS;   // frames + the kernels' static arrays
    };
    p.verdict = verdict();
    return p;
}

// The tick with the warp inside it (k_bank_tick_warp.hip): the plan's workgroup plus the stream's clamped mesh, `nodes`
// (warp_nodes of the width times warp_nodes of the height, aof_warp_step.hpp: the callers' header) nodes of 8 bytes behind
// the plan's dynamic LDS (648 B at 64 x 64, 2 312 B at 128 x 128; the plan's bytes are a multiple of 16, so the nodes
// start on one).  ok: the plan's verdict is SMALL_OK and frames + nodes + the kernels' static arrays fit LDS; the rest is
// filled whatever it says.
struct SmallWarpPlan {
    bool ok;
    size_t nodes_at;               // byte offset of the nodes in the dynamic LDS
    size_t lds;                    // dynamic LDS bytes of a workgroup: the plan's and the nodes
    int32_t attr;                  // the launcher raises the instantiation's dynamic-LDS limit first
};

inline SmallWarpPlan small_warp_plan_make(const SmallArgs &a, int64_t nodes)
{
    const SmallPlan p = small_plan_make(a);
    SmallWarpPlan q = {};
    q.nodes_at = p.lds;
    q.lds = p.lds + (size_t)(nodes > 0 ? nodes : 0) * sizeof(aof_warp_point);
    q.attr = q.lds > kSmallAttrAbove ? 1 : 0;
    q.ok = p.verdict == SMALL_OK && q.lds + kSmallStaticLds <= kSmallLdsLimit;
    return q;
}

// ---- the grouped lane-per-block search (k_flow_lane8): a workgroup owns ppw whole pairs ----

// The lane-per-block kernels serve B = 8, S = 4 on any grid, within their 24-bit multiplies and 32-bit offsets.
inline bool lane8_plan_supported(const SearchArgs &a)
{
    if (a.tile != 8 || a.search != 4) return false;
    const int64_t frame = (int64_t)a.w * a.h;
    const int nb = a.grid.blocks();
    if (frame > (1 << 24) || nb < 1 || nb >= (1 << 24)) return false;   // 24-bit multiplies in the kernels
    // a wave's lanes address their frames with 32-bit offsets from the wave's first pair
    const int64_t span = 64 / nb + 2;
    if (a.n_pairs > 1 && (a.pair_stride < 0 || span * a.pair_stride + frame > 0xFFFFFFFFll)) return false;
    return true;
}

struct Lane8GroupPlan {
    int32_t ppw;                   // whole pairs per workgroup, 1 .. 32; 0 = the grid does not qualify
    int64_t wgs;                   // workgroups of a launch of a.n_pairs pairs
    int32_t last_live;             // lanes of the last workgroup that own a block
    size_t lds;                    // vote histograms: [ppw][2][bins] words
};

inline Lane8GroupPlan lane8_group_plan(const SearchArgs &a)
{
    Lane8GroupPlan g = {};
    const int nb = a.grid.blocks();
    if (!lane8_plan_supported(a) || nb < 8 || nb > kThreads) return g;
    g.ppw = kThreads / nb;
    const int n = 2 * (2 * a.hist_range + 1) + 1;
    g.lds = (size_t)g.ppw * 2 * (size_t)(n > 0 ? n : 0) * sizeof(uint32_t);
    if (a.n_pairs < 1) return g;
    g.wgs = (a.n_pairs + g.ppw - 1) / g.ppw;
    g.last_live = (int32_t)(a.n_pairs - (g.wgs - 1) * g.ppw) * nb;
    return g;
}

}  // namespace aof
