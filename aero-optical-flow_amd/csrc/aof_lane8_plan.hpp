// The launch plan of the flat lane-per-block 8x8 kernels (DESIGN.md "Kernels": K2): k_search_lane8 (K3 behind it),
// k_flow_lane8_flat (the reduction in the launch) and the chunk walk k_search_lane8_pruned, all of which run
// search_chunks (aof_lane8_kernels.hpp) and are launched by launch_search_lane8 (k_search_lane8.hip).  Host only, no HIP:
// tests/native/host_selftest.cpp holds lane8_flat_plan to the model of tests/lane8_plan_ref.py.  The kernels' own address
// arithmetic stays in the kernels.
#pragma once

#include <cstdint>

#include "aof_engine_args.hpp"
#include "aof_small_plan.hpp"   // kThreads: block size of the chunk walk and of large flat launches; lane8_plan_supported

namespace aof {

// One launch indexes its (pair, block) items with 31 bits; larger batches are cut into several.
constexpr int64_t kMaxItems = 0x7FFF0000ll;
// Workgroup size of the flat kernels.  Large launches: 64, 128 and 256 threads measure the same (512 is
// 4 % slower).  A launch of only a few generations of waves (configs[3]'s per-GPU share: 128 VGA pairs
// are 2.3 generations) ends sooner with one-wave workgroups, whose slots free up wave by wave.
constexpr int kSmallLaunchThreads = 64;
constexpr int64_t kFlatLargeItems = 6 * 256 * 1024;   // six generations of 256 CUs x 16 waves: 256 threads from here on
// The chunk walk: consecutive chunks per workgroup, so that all but the first inherit start row and verdict -- as many as
// leave some 1 500 workgroups to the launch (1 024 VGA pairs: 8 chunks 6.29, 4: 6.14, 1: 5.13 M pairs/s;
// 256 pairs: 3 chunks 4.84, 8: 4.38; profiles/r04_p8_chunks_per_workgroup.txt)
constexpr int64_t kWalkWorkgroups = 1536;
constexpr int kWalkMaxChunks = 8;

enum Lane8Kind : int32_t {
    LANE8_EXHAUSTIVE = 0,   // k_search_lane8, K3 follows
    LANE8_FUSED,            // k_flow_lane8_flat: finaliser workgroups behind the searching ones
    LANE8_CHUNK_WALK,       // k_search_lane8_pruned
};

// Why a launch cannot reduce inside itself: the FIRST condition that fails, in the order they are tested.
enum Lane8Votes : int32_t {
    VOTES_OK = 0,
    VOTES_PRUNED,        // the chunk walk has no such form
    VOTES_NO_MEMORY,     // the context has no vote memory
    VOTES_NO_FAULT,      // ... or no fault word
    VOTES_BINS,          // more than 62 bins per axis
    VOTES_STRIDE,        // a record does not hold the arrival word and both histograms
    VOTES_GRID,          // 64 blocks or fewer: a wave would cover more than two pairs
    VOTES_CAPACITY,      // more pairs in a launch slice than the context has records
};

struct Lane8FlatPlan {
    // ---- the whole call
    int32_t supported;       // lane8_plan_supported
    int32_t votes;           // Lane8Votes (of the call's arguments, whether or not the reduction was asked for)
    int32_t prune_large;     // enough 256-block chunks for ADAPTIVE to consider pruning (kPruneMinChunks)
    int64_t chunks_all;      // 256-block chunks of all pairs
    int64_t per;             // pairs per slice at the most
    int64_t slices;
    // ---- slice `slice`: its pairs and where its arrays begin, in elements of each array
    int64_t done, pairs;
    int64_t frame_off;       // prev, cur: bytes
    int64_t block_off;       // blocks (records), subdirs (bytes)
    int64_t pred_off;        // pred, the tail's pred, flows: records
    int64_t sums_off;        // sums: words
    int64_t items;
    int32_t kind;            // Lane8Kind
    int32_t threads;
    int64_t wgs;             // searching workgroups
    int64_t finalisers;      // fused: workgroups behind them, one wave per pair
    int64_t grid;            // workgroups launched
    int32_t last_live;       // lanes of the last searching workgroup (the walk: of its last chunk) that own an item
    int64_t chunks;          // the walk: 256-item chunks,
    int32_t spw;             //   consecutive chunks per workgroup,
    int32_t last_chunks;     //   chunks of the last workgroup
    uint32_t stride;         // the walk's report: one workgroup in `stride` writes a slot (the first slice reports)
    uint32_t expected;       //   slots written
};

// Pairs per slice: at most kMaxItems items, and pair indices are multiplied in 24 bits.
inline int64_t lane8_slice_pairs(int nb)
{
    int64_t per = kMaxItems / nb;
    if (per >= (1 << 24)) per = (1 << 24) - 1;
    return per;
}

inline int lane8_flat_threads(int64_t items)
{
    return items < kFlatLargeItems ? kSmallLaunchThreads : kThreads;   // fewer than six generations of 256 CUs x 16 waves
}

inline Lane8Votes lane8_votes_verdict(const SearchArgs &a, const VoteMem *votes, int64_t capacity_pairs)
{
    const int n = 2 * (2 * a.hist_range + 1) + 1;
    if (a.prune) return VOTES_PRUNED;
    if (!votes || !votes->base) return VOTES_NO_MEMORY;
    if (!votes->fault) return VOTES_NO_FAULT;
    if (n > 62) return VOTES_BINS;
    if (votes->stride < (uint32_t)(2 + 2 * n)) return VOTES_STRIDE;
    if (a.grid.blocks() <= 64) return VOTES_GRID;   // a wave covers at most two pairs
    const int64_t per = kMaxItems / a.grid.blocks();   // pairs per launch slice
    return (a.n_pairs < per ? a.n_pairs : per) <= capacity_pairs ? VOTES_OK : VOTES_CAPACITY;
}

// fused: the caller hands a tail and the vote memory (the reduction runs in the launch).  slice: which one to describe.
inline Lane8FlatPlan lane8_flat_plan(const SearchArgs &a, bool fused, const VoteMem *votes, int64_t capacity_pairs, int64_t slice = 0)
{
    Lane8FlatPlan p = {};
    const int nb = a.grid.blocks();
    p.supported = lane8_plan_supported(a) ? 1 : 0;
    p.votes = lane8_votes_verdict(a, votes, capacity_pairs);
    p.stride = 1;
    if (nb < 1 || a.n_pairs < 1) return p;
    p.chunks_all = (a.n_pairs * nb + kThreads - 1) / kThreads;
    p.prune_large = p.chunks_all >= kPruneMinChunks ? 1 : 0;
    p.per = lane8_slice_pairs(nb);
    p.slices = (a.n_pairs + p.per - 1) / p.per;
    if (slice < 0 || slice >= p.slices) return p;

    p.done = slice * p.per;
    p.pairs = a.n_pairs - p.done < p.per ? a.n_pairs - p.done : p.per;
    p.frame_off = p.done * a.pair_stride;
    p.block_off = p.done * nb;
    p.pred_off = p.done;
    p.sums_off = p.done * 4;
    p.items = p.pairs * nb;
    p.kind = fused ? LANE8_FUSED : (a.prune ? LANE8_CHUNK_WALK : LANE8_EXHAUSTIVE);
    if (p.kind == LANE8_CHUNK_WALK) {
        p.threads = kThreads;
        p.chunks = (p.items + kThreads - 1) / kThreads;
        p.spw = (int32_t)(p.chunks / kWalkWorkgroups < 1 ? 1 : (p.chunks / kWalkWorkgroups > kWalkMaxChunks ? kWalkMaxChunks : p.chunks / kWalkWorkgroups));
        p.wgs = (p.chunks + p.spw - 1) / p.spw;
        p.grid = p.wgs;
        p.last_chunks = (int32_t)(p.chunks - (p.wgs - 1) * p.spw);
        p.last_live = (int32_t)(p.items - (p.chunks - 1) * kThreads);
        if (slice == 0) {   // (launches of more than 2^31 items: the first slice reports)
            p.stride = (uint32_t)((p.wgs + kPruneSlots - 1) / kPruneSlots);
            p.expected = (uint32_t)((p.wgs + p.stride - 1) / p.stride);
        }
        return p;
    }
    p.threads = lane8_flat_threads(p.items);
    p.wgs = (p.items + p.threads - 1) / p.threads;
    p.last_live = (int32_t)(p.items - (p.wgs - 1) * p.threads);
    if (p.kind == LANE8_FUSED) p.finalisers = (p.pairs + p.threads / 64 - 1) / (p.threads / 64);   // one wave per pair
    p.grid = p.wgs + p.finalisers;
    return p;
}

}  // namespace aof
