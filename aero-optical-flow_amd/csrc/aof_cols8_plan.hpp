// Segment plan and launch constants of the column walk (k_search_cols8.hip fills the plan, aof_cols8_kernels.hpp walks it).
#pragma once

#include <cstdint>

#include "aof_engine_args.hpp"
#include "aof_fastdiv.hpp"
#include "aof_small_plan.hpp"   // lane8_plan_supported

namespace aof {

// The pruned search on dense grids as a column walk (k_search_cols8.hip): a lane keeps the lower half of its window for
// the block below.  Same modes (a.prune 1 / 2), same report as the chunk walk.
inline bool lane8_cols_supported(const SearchArgs &a)
{
    // a dense grid whose next block row is the same window eight rows further down; one unit per column and segment
    return lane8_plan_supported(a) && a.grid.step_y == 8 && a.grid.nx >= 16 && a.grid.ny >= 2 && a.grid.blocks() > 256;
}

// tail + votes: the reduction in the same launch (k_flow_lane8_cols), as launch_search_lane8 does for the exhaustive scan
inline bool lane8_cols_votes_supported(const SearchArgs &a, const VoteMem &votes, int64_t capacity_pairs)
{
    const int n = 2 * (2 * a.hist_range + 1) + 1;
    if (!lane8_cols_supported(a) || !votes.base || !votes.fault || n > 62 || votes.stride < (uint32_t)(2 + 2 * n)) return false;
    return a.n_pairs <= capacity_pairs;   // (one launch: capacity is far below the 31-bit unit index)
}

// (outside the anonymous namespace: profilers print kernel names with their parameter types, and the tools cut the
//  name at the first "(anonymous namespace)::")
struct ColsSegments {
    int32_t segs, len;          // segments per column, block rows per segment
    uint32_t units_per_pair;    // segs * nx padded to a multiple of 64
    FastDiv div_units;
};
// The launch's pairs [0, head_pairs) are cut into `head` segments; the pairs behind them -- the part of the launch that
// would fill the device's wave slots only partly, at the end -- into segments half as long (`tail`), so that the last
// waves to start are the short ones and the launch does not end on a third of the device (workgroups run in launch order).
struct ColsPlan {
    ColsSegments head, tail;
    uint32_t head_pairs, head_units;   // head_units = head_pairs * head.units_per_pair
    FastDiv div_nx;
    uint32_t aligned;                  // rows, pair strides and frame bases are multiples of four bytes (window_row)
};
// VOTE: the reduction in the same launch (aof_reduce.hpp: vote_and_arrive / await_votes_and_finalise, as in
// k_flow_lane8_flat).  Workgroups [0, search_wgs) search and vote, the ones behind them are finalisers, one wave per pair.
struct ColsVotes {
    uint32_t search_wgs;
    FlowTail tail;
    VoteMem votes;
};


constexpr int kColsThreads = 256;
// Block rows a lane walks: as many as leave the launch three quarters of a generation of waves (256 CUs x 16), between 2
// and 8.  Longer segments load less (a segment's first block loads a whole window) and carry their hints further; shorter
// ones fill the device on small launches (256 VGA pairs, two batches in flight: 6 rows 38.9 us per step, 8: 41.2, 2: 45.3;
// 1 024 pairs: 8 rows 148 us, 3: 160; profiles/r04_p8_column_walk.txt).
constexpr int kColsMaxRows = 8, kColsMinRows = 2;
constexpr int64_t kColsWavesWanted = 3072;
constexpr int64_t kWaveSlots = 4096;   // 256 CUs x 4 SIMDs x 4 waves of this kernel
constexpr int64_t kColsMaxUnits = 0x7FFF0000ll;   // units are indexed with 31 bits

// One launch of the walk as the host plans it: the plan the kernel decodes its units with, and the launch's geometry.
// Host only, no HIP: tests/native/host_selftest.cpp holds it to the model of tests/cols_plan_ref.py.
struct ColsLaunch {
    ColsPlan plan;
    int64_t per;          // pairs one launch can hold (a call of more pairs is cut into several launches)
    int64_t pairs;        // pairs of this launch
    int64_t tail_pairs;   // of which the last ones get the short segments
    int64_t units, wgs;   // units (threads that decode one) and workgroups of kColsThreads
};

inline ColsSegments cols_segments(const Grid &g, int len)
{
    ColsSegments s;
    s.len = len > g.ny ? g.ny : len;
    s.segs = (g.ny + s.len - 1) / s.len;
    s.units_per_pair = (uint32_t)((s.segs * g.nx + 63) / 64 * 64);
    s.div_units = fastdiv_make(s.units_per_pair);
    return s;
}

// The launch that starts at pair `done` of a call of n_pairs pairs (w, h, pair_stride, cur: what `aligned` depends on).
inline ColsLaunch cols_plan_make(const Grid &g, int w, int h, int64_t pair_stride, uintptr_t cur, int64_t n_pairs, int64_t done = 0)
{
    auto waves = [&](int len) { return n_pairs * (int64_t)(cols_segments(g, len).units_per_pair / 64); };
    int len = kColsMaxRows;
    while (len > kColsMinRows && waves(len) < kColsWavesWanted) len--;
    ColsLaunch l;
    ColsPlan &plan = l.plan;
    plan.head = cols_segments(g, len);
    plan.tail = cols_segments(g, len / 2 < kColsMinRows ? kColsMinRows : len / 2);
    plan.div_nx = fastdiv_make((uint32_t)g.nx);
    // (columns eight bytes apart: every lane of a pair is misaligned alike and finds its last bytes in the next column's load)
    plan.aligned = (g.step_x == 8 && w % 4 == 0 && pair_stride % 4 == 0 && cur % 4 == 0 && ((int64_t)w * h) % 4 == 0) ? 1u : 0u;
    l.per = kColsMaxUnits / plan.tail.units_per_pair;   // (the tail's units per pair are the larger)
    l.pairs = n_pairs - done < l.per ? n_pairs - done : l.per;
    // pairs beyond the last full generation of wave slots (256 CUs x 16 waves) get the short segments
    const int64_t wpp = plan.head.units_per_pair / 64, all = l.pairs * wpp, rest = all % kWaveSlots;
    l.tail_pairs = 0;
    if (rest != 0 && rest * 5 < kWaveSlots * 4 && plan.tail.len < plan.head.len && all > kWaveSlots) l.tail_pairs = (rest + wpp - 1) / wpp;
    plan.head_pairs = (uint32_t)(l.pairs - l.tail_pairs);
    plan.head_units = plan.head_pairs * plan.head.units_per_pair;
    l.units = (int64_t)plan.head_units + l.tail_pairs * plan.tail.units_per_pair;
    l.wgs = (l.units + kColsThreads - 1) / kColsThreads;
    return l;
}

}  // namespace aof
