// The launch plan of the 16x16 search (DESIGN.md "Kernels": K2 tile16): which configurations k_search_tile16 serves, its
// dynamic LDS, the instantiation, the n_pairs * ny grid, and the kernel in front of an ADAPTIVE launch -- the probe with its
// sample strides, or the forced-verdict fill.  Host only, no HIP: tests/native/host_selftest.cpp holds tile16_plan to the
// model of tests/batch_plan_ref.py.  The kernels' own address arithmetic stays in the kernels (k_search_tile16.hip); what a
// workgroup stages, from which bytes into which, and its loops' trips are restated by tests/tile16_rows_ref.py, whose byte
// extents are held inside the frame arrays and inside tile16_lds() for every width, origin and predictor.
#pragma once

#include <cstddef>
#include <cstdint>

#include "aof_hd.hpp"
#include "aof_engine_args.hpp"

namespace aof {

constexpr int kTile16Threads = 512;
constexpr int kSide = 17;  // 2S+1
// ADAPTIVE mode (the default of 16x16 contexts): the probe kernel decides per pair.
constexpr int kProbeThreads = 1024;        // a pair's ~1 200 probe items in two rounds
constexpr int kProbeStride = 8;            // every eighth block in x and in y is probed (VGA-like grids: ~1.6 % of the blocks)
constexpr int kProbeMaxBlocks = 128;       // sample blocks per pair at the most (the strides grow beyond that)
constexpr int kFillThreads = 256;          // the forced-verdict fill: a lane per pair
constexpr size_t kTile16LdsLimit = 156 * 1024;    // one block row's tile, tables included
constexpr size_t kTile16AttrAbove = 64 * 1024;    // dynamic LDS beyond this needs the function attribute
// Blocks stride/2, stride/2 + stride, ... of an axis of n blocks.
AOF_HD_INLINE constexpr int probe_samples(int n, int stride) { return (n + stride - 1 - stride / 2) / stride; }

// Why k_search_tile16 cannot serve a search: the FIRST condition that fails, in the order they are tested.
enum Tile16Verdict : int32_t {
    TILE16_OK = 0,
    TILE16_NO_TILE,        // tile != 16 or search != 8
    TILE16_NO_GRID,        // not the dense grid at (8, 8) -- (9, 9) with half-pixel refinement --, step 16
    TILE16_NO_WIDTH,       // w % 16
    TILE16_NO_STRIDE,      // pair_stride % 16
    TILE16_NO_PREV,        // prev off 16 bytes
    TILE16_NO_CUR,         // cur off 16 bytes
    TILE16_NO_FRAME,       // a frame beyond 31 bits
    TILE16_NO_LDS,         // a block row's tile and tables do not fit kTile16LdsLimit
};

// The kernel in front of the search of an ADAPTIVE launch (a.prune == 2).
enum Tile16Front : int32_t {
    TILE16_FRONT_NONE = 0,
    TILE16_FRONT_PROBE,    // k_tile16_probe: one workgroup per pair judges it
    TILE16_FRONT_FILL,     // k_tile16_fill_verdicts: the test hook's verdicts in place of the probe's
};

struct Tile16Plan {
    int32_t verdict;       // Tile16Verdict
    int32_t refines;       // the launch also writes the half-pixel directions (no K2b behind it)
    size_t lds;            // dynamic LDS bytes of a workgroup
    int32_t attr;          // the launcher raises the instantiation's dynamic-LDS limit first
    int32_t prune, refine; // the instantiation k_search_tile16<prune, refine>
    int64_t total;         // workgroups: one per pair and block row
    int32_t overflow;      // more than 31 bits of them: the launch is refused
    int32_t front;         // Tile16Front
    int32_t refused;       // overflow, or a front kernel without its hints or with more verdicts than kMaxForcedVerdicts
    int64_t front_wgs;     // workgroups of the front kernel
    int32_t stx, sty;      // the probe: every stx-th block in x and sty-th in y,
    int32_t sx, sy;        //   samples per axis
};

// Half-pixel refinement runs inside the search launch (k_search_tile16<.., true>) whenever directions are wanted.
inline bool tile16_refines(const SearchArgs &a) { return a.subpixel && a.subdirs; }

inline size_t tile16_lds(const SearchArgs &a)
{
    size_t bytes = (size_t)48 * a.w + 4 * (size_t)a.grid.nx + 16;
    if (tile16_refines(a)) bytes += 2 * (size_t)a.w + 16 + 16;   // cur rows -1 and 32, the pad in front, dword reads past the last ring
    if (a.prune) bytes += 4 * (size_t)kSide * a.grid.nx + 16;   // lower bounds + item list + counter
    return bytes;
}

inline Tile16Verdict tile16_verdict(const SearchArgs &a)
{
    if (a.tile != 16 || a.search != 8) return TILE16_NO_TILE;
    const int org = a.subpixel ? 1 : 0;  // origin S+1: K2b follows
    if (a.grid.x0 != 8 + org || a.grid.y0 != 8 + org || a.grid.step_x != 16 || a.grid.step_y != 16) return TILE16_NO_GRID;
    if (a.w % 16) return TILE16_NO_WIDTH;
    if (a.pair_stride % 16) return TILE16_NO_STRIDE;
    if (reinterpret_cast<uintptr_t>(a.prev) % 16) return TILE16_NO_PREV;
    if (reinterpret_cast<uintptr_t>(a.cur) % 16) return TILE16_NO_CUR;
    if ((int64_t)a.w * a.h > 0x7FFFFFFF) return TILE16_NO_FRAME;
    return tile16_lds(a) <= kTile16LdsLimit ? TILE16_OK : TILE16_NO_LDS;
}

// LDS-tiled (block, dy)-per-lane kernel for B=16, S=8 on a dense grid (any predictor).
inline bool tile16_supported(const SearchArgs &a) { return tile16_verdict(a) == TILE16_OK; }

// forced_count: the verdicts of the test hook (Tile16Verdicts.count; 0 = the probe decides).
inline Tile16Plan tile16_plan(const SearchArgs &a, int forced_count)
{
    Tile16Plan p = {};
    p.verdict = tile16_verdict(a);
    p.refines = tile16_refines(a) ? 1 : 0;
    p.lds = tile16_lds(a);
    p.attr = p.lds > kTile16AttrAbove ? 1 : 0;
    p.prune = a.prune ? 1 : 0;
    p.refine = p.refines;
    p.total = a.n_pairs * a.grid.ny;
    p.overflow = p.total > 0x7FFFFFFF ? 1 : 0;
    p.refused = p.overflow;
    if (a.prune != 2 || p.overflow) return p;
    if (forced_count > 0) {   // (test hook: the verdicts are set, no probe runs)
        p.front = TILE16_FRONT_FILL;
        p.refused = !a.hints || forced_count > kMaxForcedVerdicts ? 1 : 0;
        p.front_wgs = (a.n_pairs + kFillThreads - 1) / kFillThreads;
        return p;
    }
    // ADAPTIVE: judge every pair first (hints in the workspace), then the search decides per pair
    p.front = TILE16_FRONT_PROBE;
    p.refused = a.hints ? 0 : 1;
    p.front_wgs = a.n_pairs;
    // every kProbeStride-th block per axis; an axis with fewer blocks than that is sampled more densely (at least one
    // block), and the strides grow -- the longer axis first -- until the sample fits the kernel's table
    int stx = kProbeStride, sty = kProbeStride;
    while (stx > 1 && probe_samples(a.grid.nx, stx) == 0) stx /= 2;
    while (sty > 1 && probe_samples(a.grid.ny, sty) == 0) sty /= 2;
    while (probe_samples(a.grid.nx, stx) * probe_samples(a.grid.ny, sty) > kProbeMaxBlocks) {
        if (probe_samples(a.grid.nx, stx) >= probe_samples(a.grid.ny, sty)) stx *= 2; else sty *= 2;
    }
    p.stx = stx; p.sty = sty;
    p.sx = probe_samples(a.grid.nx, stx); p.sy = probe_samples(a.grid.ny, sty);
    return p;
}

}  // namespace aof
