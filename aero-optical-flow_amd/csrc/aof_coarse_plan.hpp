// The launch plans of the two coarse passes of a pair: k_coarse's sweep plan (k_coarse.hip launches it) and K1's strip
// plan (k_pyramid.hip).  Host only, no HIP: tests/native/host_selftest.cpp holds both to the model of
// tests/coarse_plan_ref.py.
#pragma once

#include <climits>
#include <cstddef>
#include <cstdint>

#include "aof_engine_args.hpp"
#include "aof_fastdiv.hpp"

namespace aof {

constexpr int kCoarseThreads = 512;
constexpr int kCoarseUnroll = 4;               // sweeps per batch; two batches = 16 loads of 16 B in flight per lane
constexpr int kCoarseMaxBins = 64;
constexpr int kCoarseScratch = 8;              // words behind the histograms: pixel sums, vote sums
constexpr size_t kCoarseLdsLimit = 160 * 1024;
constexpr int kCoarseStaggerGroups = 3;        // lab sweep (tools/coarse_lab.hip): 1: 0.215, 2: 0.206, 3: 0.203, 4: 0.212 ms
constexpr int64_t kCoarseStaggerBytesPerUs = 75000;   // start-up spacing of the groups: ~8 us at VGA

// Why k_coarse cannot serve a configuration: the FIRST condition that fails, in the order they are tested.
enum CoarseVerdict : int32_t {
    COARSE_OK = 0,
    COARSE_NO_TILE,        // tile != 8
    COARSE_NO_SEARCH,      // search != 4
    COARSE_NO_SUBPIXEL,    // half-pixel refinement asked for
    COARSE_NO_WIDTH,       // w % 16 (16-byte chunks; level-1 rows a multiple of 8 bytes)
    COARSE_NO_HEIGHT,      // h % 2
    COARSE_NO_STRIDE,      // pair_stride % 16
    COARSE_NO_CHUNKS,      // more 16-byte chunks per row than the workgroup has lanes
    COARSE_NO_PREV,        // prev off 16 bytes
    COARSE_NO_CUR,         // cur off 16 bytes
    COARSE_NO_GRID,        // not the dense level-1 grid at (4, 4), step 8
    COARSE_NO_BINS,        // more vote bins than the histograms hold
    COARSE_NO_PAIRS,       // pair count beyond 31 bits
    COARSE_NO_LDS,         // both level-1 frames, the keys and the histograms do not fit 160 KB
};

struct CoarsePlan {
    CoarseVerdict verdict;
    int32_t rows_per_sweep;        // level-1 rows one sweep of the workgroup's lanes covers
    int32_t nkf, nk, nk_pad;       // sweeps per frame, per pair, per pair in whole rounds of two batches
    FastDiv div_nb, div_nx, div_chunks;
    size_t lds;
    int32_t stagger_groups, stagger_ticks;
    int64_t wgs;
};

inline size_t coarse_plan_lds(int w, int h, const Grid &g)
{
    return (size_t)2 * (w / 2) * (h / 2) + (size_t)g.blocks() * 4 + 2 * (2 * kCoarseMaxBins + kCoarseScratch) * 4;
}

// One workgroup must hold both level-1 frames, and the windows must sit on 8-byte columns.
inline CoarseVerdict coarse_plan_verdict(int w, int h, int64_t pair_stride, uintptr_t prev, uintptr_t cur, const Grid &g, int range,
                                         int tile, int search, int subpixel, int64_t n_pairs)
{
    if (tile != 8) return COARSE_NO_TILE;
    if (search != 4) return COARSE_NO_SEARCH;
    if (subpixel) return COARSE_NO_SUBPIXEL;
    if (w < 16 || w % 16) return COARSE_NO_WIDTH;
    if (h < 2 || h % 2) return COARSE_NO_HEIGHT;
    if (pair_stride % 16) return COARSE_NO_STRIDE;
    if (w / 16 > kCoarseThreads) return COARSE_NO_CHUNKS;
    if (prev % 16) return COARSE_NO_PREV;
    if (cur % 16) return COARSE_NO_CUR;
    if (g.x0 != 4 || g.y0 != 4 || g.step_x != 8 || g.step_y != 8 || g.nx < 1 || g.ny < 1) return COARSE_NO_GRID;
    if ((w / 2) % 8) return COARSE_NO_WIDTH;   // level-1 rows a multiple of 8 bytes: aligned 8-byte LDS reads
    if (2 * (2 * range + 1) + 1 > kCoarseMaxBins) return COARSE_NO_BINS;
    if (n_pairs > 0x7FFFFFFF) return COARSE_NO_PAIRS;
    return coarse_plan_lds(w, h, g) <= kCoarseLdsLimit ? COARSE_OK : COARSE_NO_LDS;
}

// The launch of n_pairs pairs on a device of `cus` CUs.  Everything behind `verdict` is zero where it is not COARSE_OK.
inline CoarsePlan coarse_plan_make(int w, int h, int64_t pair_stride, uintptr_t prev, uintptr_t cur, const Grid &g, int range, int tile,
                                   int search, int subpixel, int64_t n_pairs, int cus)
{
    CoarsePlan p = {};
    p.verdict = coarse_plan_verdict(w, h, pair_stride, prev, cur, g, range, tile, search, subpixel, n_pairs);
    if (p.verdict != COARSE_OK) return p;
    p.div_nb = fastdiv_make((uint32_t)g.blocks());
    p.div_nx = fastdiv_make((uint32_t)g.nx);
    p.div_chunks = fastdiv_make((uint32_t)(w / 16));
    {   // Rows per sweep: as many as the workgroup has lanes for, but such that the two frames take a
        // whole number of rounds of two batches -- padding sweeps would be loaded for nothing
        // (VGA: 20 rows = 800 lanes, 24 sweeps, no padding; 25 rows would pad 20 sweeps to 24).
        const int chunks = w / 16, h1 = h / 2, rmax = kCoarseThreads / chunks;
        int best = rmax;
        int64_t best_rows = LLONG_MAX;
        for (int r = rmax; r >= 1 && r >= rmax / 2; r--) {
            const int nk = 2 * ((h1 + r - 1) / r);
            const int nk_pad = (nk + 2 * kCoarseUnroll - 1) / (2 * kCoarseUnroll) * (2 * kCoarseUnroll);
            const int64_t loaded = (int64_t)nk_pad * r;
            if (loaded < best_rows) { best_rows = loaded; best = r; }
        }
        p.rows_per_sweep = best;
        p.nkf = (h1 + best - 1) / best;
        p.nk = 2 * p.nkf;
        p.nk_pad = (p.nk + 2 * kCoarseUnroll - 1) / (2 * kCoarseUnroll) * (2 * kCoarseUnroll);
    }
    p.lds = coarse_plan_lds(w, h, g);
    p.stagger_groups = cus > 0 && n_pairs >= 2 * (int64_t)cus ? kCoarseStaggerGroups : 1;
    // one group's share of the stream phase: the pair's bytes at the rate a CU reaches when
    // only 1/groups of the chip streams
    p.stagger_ticks = (int32_t)((int64_t)2 * w * h * 100 / kCoarseStaggerBytesPerUs);
    // one workgroup per CU (LDS); each walks pairs blockIdx.x, blockIdx.x + gridDim.x, ...
    p.wgs = cus <= 0 ? 0 : n_pairs < cus ? n_pairs : cus;
    return p;
}

// The plan of a launch's arguments (first_generation: the CUs of the context's device).
inline CoarsePlan coarse_plan_of(const CoarseArgs &a)
{
    return coarse_plan_make(a.w, a.h, a.pair_stride, reinterpret_cast<uintptr_t>(a.prev), reinterpret_cast<uintptr_t>(a.cur), a.grid,
                            a.tail.range, a.tile, a.search, a.subpixel, a.n_pairs, a.first_generation);
}

constexpr int kPyramidThreads = 256;
constexpr int kPyramidItemsPerBlock = 1024;    // 16-px x 2-row items per workgroup

struct PyramidPlan {
    int32_t vec;                   // k_pyramid_vec (16-byte loads), else k_pyramid_scalar
    int32_t rows_per_strip;        // vec: level-1 rows of one workgroup (0 for the scalar kernel)
    int32_t nstrips;               // workgroups per unit
    int64_t units;                 // frames: two per pair, or the frames of a sequence
    int64_t total;                 // workgroups; more than 31 bits: the launch is refused
    int64_t zero_words;            // words of pixel sums to zero first
};

// n_pairs as PyramidArgs has it: the FRAMES of a sequence, else the pairs.
inline PyramidPlan pyramid_plan_make(int w, int h, int64_t pair_stride, uintptr_t prev, uintptr_t cur, int sequence, int64_t n_pairs,
                                     bool sums)
{
    PyramidPlan p = {};
    p.units = sequence ? n_pairs : n_pairs * 2;
    p.zero_words = sums ? (sequence ? n_pairs - 1 : n_pairs) * 4 : 0;
    if (p.zero_words < 0) p.zero_words = 0;
    p.vec = (w >= 16 && w % 16 == 0 && h % 2 == 0 && pair_stride % 16 == 0 && prev % 16 == 0 && (sequence || cur % 16 == 0)) ? 1 : 0;
    if (p.vec) {
        const int chunks = w / 16, h1 = h / 2;
        int rows = kPyramidItemsPerBlock / chunks;
        if (rows < 1) rows = 1;
        p.rows_per_strip = rows;
        p.nstrips = (h1 + rows - 1) / rows;
    } else {
        const int64_t cells = (int64_t)((w + 1) / 2) * ((h + 1) / 2);
        p.nstrips = (int)((cells + kPyramidItemsPerBlock - 1) / kPyramidItemsPerBlock);
        if (p.nstrips < 1) p.nstrips = 1;
    }
    p.total = p.units * p.nstrips;
    return p;
}

}  // namespace aof
