// The search engine's side of the library: the block grid and the host's parameter logic, the argument structs its
// kernels take by value, and their launchers.  Not installed; the public surface is include/aof.h.
#pragma once

#include <cstddef>
#include <cstdint>

#include "aof.h"
#include "aof_fastdiv.hpp"
#include "aof_hd.hpp"

namespace aof {

struct Grid {
    int32_t x0, y0, step_x, step_y, nx, ny;
    AOF_HD int32_t blocks() const { return nx * ny; }
};

// Host-only parameter logic (aof_params.cpp).
int grid_for_level(const aof_params &p, int level, Grid *g);
int level_range(const aof_params &p, int level);  // histogram half-range R
int value_threshold_u16(const aof_params &p);     // SAD gate clamped to the u16 record
int reduce_chunks(int nblocks);                   // 0: one reduction workgroup per pair reads all records
size_t hist_bytes_per_pair(const aof_params &p, int level);  // vote-histogram scratch of one pair

// What turns a pair's vote histograms into its aof_flow (K3).
struct FlowTail {
    int32_t nblocks;
    int32_t range;             // R
    int32_t hist_filter;
    int32_t min_valid;
    aof_flow *flows;           // [n_pairs]
    const aof_flow *pred;      // copy pred_x/pred_y + PRED_VALID from here (level 0 of two), or nullptr
    int32_t emit_predictor;    // level 1: write the integer predictor into pred_x/pred_y
};

// The context's vote memory (zero at rest): one record per pair of the running launch -- word 0 the
// number of blocks that have arrived, then the two vote histograms (aof_reduce.hpp).
struct VoteMem {
    uint32_t *base;     // [pairs][stride] words
    uint32_t stride;    // words per pair, a multiple of 64 (256 bytes: pairs never share a line)
    uint32_t *fault;    // pinned host word of the context: a finaliser that gives up stores pair + 1 here
    uint32_t deadline_ticks;   // finaliser waves give up after this many ticks of the 100 MHz counter
};

// What the pruned lane8 search tells the host about itself (the ADAPTIVE mode of 8x8 contexts, choose_lane8 in aof_batch_plan.hpp):
// one workgroup in `stride` stores how many of its first wave's chunks left with "pruning pays" into a word of
// pinned host memory: tag (low 16 bits of launch_no) << 16 | paying << 8 | chunks.  Plain stores, nobody waits
// for them: the host reads whatever has arrived when it enqueues the next launch.  Speed only, never results.
constexpr int kPruneSlots = 256;
struct PruneReport {
    uint32_t *slots;      // pinned, kPruneSlots words; nullptr = no report
    uint32_t launch_no;
    uint32_t stride;      // (filled by the launcher)
    uint32_t expected;    // slots this launch writes (filled by the launcher)
};

// Everything one search launch needs; passed to the kernels by value.
struct SearchArgs {
    const uint8_t *prev;       // level frames of the older image, pair i at +i*stride
    const uint8_t *cur;        // level frames of the newer image
    int64_t pair_stride;       // bytes between consecutive pairs (both arrays)
    int32_t w, h;              // level frame size, row stride == w
    int32_t tile, search;      // B, S
    Grid grid;
    int32_t feature_threshold;
    int32_t value_threshold;   // clamped to <= 0xFFFF
    int32_t subpixel;
    aof_block *blocks;         // [n_pairs][grid.blocks()]
    uint8_t *subdirs;          // [n_pairs][grid.blocks()] or nullptr
    const aof_flow *pred;      // [n_pairs] level-1 results carrying the predictor, or nullptr
    const uint32_t *sums;      // [n_pairs][2][2] pixel sums, or nullptr when not equalising
    int32_t level;             // which sums column to use
    int64_t n_pairs;
    int32_t hist_range;        // R
    int32_t prune;             // 0 exhaustive, 1 exact partial-distortion elimination (lane8, tile16), 2 adaptive (tile16: per pair, by hints; lane8: the first chunk of a wave runs exhaustively and judges)
    uint32_t *hints;           // tile16, adaptive: [n_pairs] written by its probe kernel (1 = pruning pays), workspace
    FastDiv div_nb, div_nx;    // lane8: filled by its launchers (item -> pair, block -> row)
};

struct ReduceArgs {
    const aof_block *blocks;
    const uint8_t *subdirs;    // nullptr when half-pixel refinement is off
    int32_t value_threshold;
    FlowTail tail;
    int64_t n_pairs;
    const uint32_t *parts;     // per-chunk histograms of the first step of a two-step reduction (then blocks are not read)
    int32_t nstrips;           // chunks per pair
    uint32_t *chunk_parts;     // large grids: scratch for per-chunk histograms ([n_pairs][chunks][2][bins]), or nullptr
};

// The fused coarse kernel (k_coarse): K1 + level-1 search + level-1 reduction of one pair per
// workgroup, level-1 frames in LDS.
struct CoarseArgs {
    const uint8_t *prev, *cur; // level-0 frames
    int64_t pair_stride;
    int32_t w, h;              // level-0 frame size
    int32_t tile, search, subpixel;
    Grid grid;                 // level-1 block grid
    int32_t feature_threshold;
    int32_t value_threshold;   // clamped to <= 0xFFFF
    uint32_t *sums;            // [n_pairs][2][2] written here (no memset, no atomics), or nullptr
    aof_block *blocks;         // level-1 records [n_pairs][grid.blocks()]
    FlowTail tail;             // level-1 flows: the predictor
    int64_t n_pairs;
    FastDiv div_nb, div_nx, div_chunks;   // filled by the launcher
    int32_t first_generation;  // workgroups of the first generation = CUs of the device (set by the caller)
    int32_t stagger_groups, stagger_ticks;   // start-up stagger; stagger_groups == 0: the launcher chooses
    int32_t rows_per_sweep;    // launcher: level-1 rows one sweep of the workgroup's lanes covers
};

// The one-workgroup kernel for small pairs (k_flow_small): one or two levels of a pair whose frames
// fit LDS and whose grids have at most 256 blocks each.  Reads l0.prev / l0.cur only; l1.prev,
// l1.cur, the pred and sums pointers inside l0 / l1 are not used (level-1 frames, predictor and
// deltas stay on chip).
struct SmallArgs {
    SearchArgs l0, l1;         // l1 only for levels == 2
    FlowTail t0, t1;
    uint32_t *sums;            // [n_pairs][2][2] written here, or nullptr when not equalising
    int32_t levels;
};

struct PyramidArgs {
    const uint8_t *prev, *cur;
    int64_t pair_stride;
    int32_t w, h;
    uint8_t *l1_prev, *l1_cur; // [n_pairs][h/2][w/2] or nullptr (sums only)
    uint32_t *sums;            // [n_pairs][2][2] or nullptr (pyramid only)
    int64_t n_pairs;
    // A frame SEQUENCE (cur = prev + one frame, pair_stride = one frame): every frame is summed and filtered ONCE.
    // n_pairs then counts the FRAMES (pairs + 1), `prev` is the first frame, `cur` / `l1_cur` are not used,
    // l1_prev receives one level-1 frame per frame, and frame f's sums go to pair f (prev) and pair f - 1 (cur).
    int32_t sequence;
};

// Kernel launchers (one per .hip file).  All enqueue on `stream` and return the
// hipError_t of the launch as int (0 = ok).
int launch_pyramid(const PyramidArgs &a, void *stream);   // zeroes a.sums first
int launch_zero_words(uint32_t *words, int64_t count, void *stream);   // (a kernel: replays correctly from a hipGraph)
int launch_coarse_fused(const CoarseArgs &a, void *stream);
int launch_search_generic(const SearchArgs &a, void *stream);
// K2b: half-pixel refinement of records written by an integer search (tile 8 or 16; today no
// plan asks for it: every search kernel refines itself, k_refine.hip); fills a.subdirs.
int launch_refine(const SearchArgs &a, void *stream);
// Lane-per-block kernel straight from global memory for B=8, S=4 on ANY grid / width /
// predictor (sparse PX4Flow grid, rows that are no multiple of 16 bytes), half-pixel refinement
// included (lane8_plan_supported, aof_small_plan.hpp).
// tail + votes: the reduction runs inside the same launch (votes through agent-scope atomics into the
// context's vote memory, the last wave of a pair writes its flow record); no K3 follows (lane8_votes_verdict,
// aof_lane8_plan.hpp).
int launch_search_lane8(const SearchArgs &a, void *stream, const FlowTail *tail = nullptr,
                        const VoteMem *votes = nullptr, PruneReport *report = nullptr);
// The pruned kernels carry their hints from block to block of a wave and need a launch large enough for walks of three
// blocks before that pays: at least kPruneMinChunks (below) 256-block chunks (lane8_flat_plan, aof_lane8_plan.hpp).
// The pruned search on dense grids as a column walk (k_search_cols8.hip; lane8_cols_supported, aof_cols8_plan.hpp).  Same
// modes (a.prune 1 / 2), same report.  tail + votes: the reduction in the same launch (lane8_cols_votes_supported).
int launch_search_lane8_cols(const SearchArgs &a, void *stream, PruneReport *report = nullptr, const FlowTail *tail = nullptr,
                             const VoteMem *votes = nullptr);
// Smallest launch (in 256-block chunks) the ADAPTIVE mode lets prune.  Round 5 sweep, bench.py --pairs N as it chooses
// itself (two batches in flight, graph replay), pruned column walk against the exhaustive kernel with the reduction in
// its launch, us per step (profiles/r05_small_launch_prune_sweep.txt): 32 pairs 14.7 / 11.0, 64: 18.6 / 14.8,
// 96: 22.2 / 20.4, 128: 23.0-24.5 / 26.0, 192: 26.6 / 38.0, 256: 33.8 / 49.7 -- a walk of two blocks pays for its vote
// and its second round of row loads with too little; from three blocks on (112 VGA pairs) it wins.
constexpr int64_t kPruneMinChunks = 2048;
// Grids of 8..256 blocks: a workgroup owns whole pairs and also writes their flow records (no K3; lane8_group_plan,
// aof_small_plan.hpp).
int launch_flow_lane8(const SearchArgs &a, const FlowTail &tail, void *stream);
// LDS-tiled (block, dy)-per-lane kernel for B=16, S=8 on a dense grid (any predictor; tile16_plan, aof_tile16_plan.hpp).
// Test hook of the adaptive 16x16 search (aof_debug_tile16_verdicts): pair i gets v[i % count] instead of the probe's
// verdict; count 0 = the probe decides.  Only launches with prune == 2 read it.
constexpr int kMaxForcedVerdicts = 8;
struct Tile16Verdicts {
    uint8_t v[kMaxForcedVerdicts];
    int32_t count;
};
int launch_search_tile16(const SearchArgs &a, void *stream, const Tile16Verdicts &forced);
// Small pairs (frames fit LDS, grids <= 256 blocks), one or two levels, in one launch: one workgroup per pair
// (small_plan_make, aof_small_plan.hpp).
int launch_flow_small(const SmallArgs &a, void *stream);
// One pair, the record published in pinned host memory by ONE tagged 16-byte store (top byte of `count` =
// low byte of *tag, which the host wrote before the launch): the per-call path polls for it.
int launch_flow_small_tagged(const SmallArgs &a, aof_flow *host_record, const uint32_t *tag, void *stream);
// (the resident form of the same kernel: aof_resident.hpp)
int launch_reduce(const ReduceArgs &a, void *stream);
int launch_derotate(const aof_derotate_params &p, const aof_flow *flows, const aof_gyro *gyro,
                    int64_t n, float *out, void *stream);

}  // namespace aof
