// The plan of a batch: which kernels, with which arguments, serve one aof_flow_batch_device call (BatchPlan: every kernel
// choice, made once before the first launch; the sequences per configuration are in DESIGN.md "Kernels"), and the one
// decision a flat 8x8 launch makes per launch (choose_lane8).  Host only, no HIP: tests/native/host_selftest.cpp holds
// plan_batch and choose_lane8 to the model of tests/batch_plan_ref.py.  aof_batch.cpp is the executor.
#pragma once

#include <cstdint>

#include "aof_coarse_plan.hpp"
#include "aof_cols8_plan.hpp"
#include "aof_engine_args.hpp"
#include "aof_lane8_plan.hpp"
#include "aof_small_plan.hpp"
#include "aof_tile16_plan.hpp"

namespace aof {

// What the plan reads of a context (aof_ctx holds one: aof_ctx.hpp).
struct BatchConfig {
    aof_params params;
    Grid g0, g1;
    int cus;                    // compute units of the context's device
    int search_mode;
    bool force_generic;
    bool split_coarse;          // run K1 / level-1 search / level-1 reduce as separate kernels
};

// ADAPTIVE search of 8x8 contexts (choose_lane8): what the pruned kernel's last reporting launch said, in pinned host
// words behind the fault word (same allocation), and what the context does with it.
struct AdaptiveSearch {
    uint32_t *slots;            // kPruneSlots words
    uint32_t launch_no;         // number of the last reporting launch (its low 16 bits tag the words)
    uint32_t expected;          // words that launch writes, 0 = none yet
    int belief;                 // -1 nothing known yet, 0 pruning does not pay on this context's images, 1 it does
    int since_probe;            // exhaustive launches since the last look
    aof_search_stats stats;
};

// Device views of one batch: frames, outputs and the workspace regions (all [n_pairs]-major).
struct BatchView {
    const uint8_t *prev, *cur;
    int64_t stride;
    uint32_t *sums;
    uint8_t *l1_prev, *l1_cur;
    aof_block *blocks1; uint8_t *subdirs1; aof_flow *flows1; uint8_t *hist1;
    aof_block *blocks0; uint8_t *subdirs0; aof_flow *flows; uint8_t *hist0;
    uint32_t *hints;   // 16x16 adaptive search: per-pair verdicts (both levels use it, one after the other)
};

enum SearchKind { SK_TILE16, SK_LANE8_GROUP, SK_LANE8, SK_GENERIC };
enum CoarseKind { COARSE_NONE, COARSE_FUSED, COARSE_K1 };

// One level's search as planned: the kernel and the arguments it was chosen on.
struct LevelPlan {
    SearchKind kind;
    bool refine;       // tile16 without half-pixel directions out of its tile: K2b follows
    SearchArgs a;      // tile16: a.prune resolved; flat lane8: the context's mode, which choose_lane8 resolves per launch
    FlowTail tail;
};

// Every kernel choice of one aof_flow_batch_device call, made before the first launch.
struct BatchPlan {
    bool small;        // k_flow_small does the whole batch in one launch, from `sm`; nothing below applies
    bool small_class;  // ... could, were the batch not larger than kSmallMaxPairs (the stream bank's tick kernel asks)
    SmallArgs sm;
    CoarseKind coarse; // pixel sums / pyramid / level-1 search: none, fused into k_coarse, or K1 + level[1]
    bool k1_pass;      // COARSE_K1 and its outputs are not in the workspace yet: K1 runs
    bool sequence;     // the frames are a sequence view (d_cur = d_prev + one frame = pair_stride)
    CoarseArgs fused;  // COARSE_FUSED
    PyramidArgs k1;    // COARSE_K1
    LevelPlan level[2];   // [1]: COARSE_K1 with two levels, a level-1 search before level 0
};

inline BatchView batch_view(const BatchConfig &cfg, const aof_ws_layout &L, const uint8_t *d_prev, const uint8_t *d_cur,
                            int64_t pair_stride, aof_block *d_blocks, uint8_t *d_subdirs, aof_flow *d_flows, void *d_workspace)
{
    const aof_params &p = cfg.params;
    BatchView v;
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    const bool two = p.pyramid_levels == 2, eq = p.mean_subtract != 0;
    v.prev = d_prev; v.cur = d_cur; v.stride = pair_stride;
    v.sums = eq ? reinterpret_cast<uint32_t *>(ws + L.sums) : nullptr;
    v.l1_prev = two ? ws + L.l1_prev : nullptr;
    v.l1_cur = two ? ws + L.l1_cur : nullptr;
    v.blocks1 = reinterpret_cast<aof_block *>(ws + L.l1_blocks);
    v.subdirs1 = p.subpixel ? ws + L.l1_subdirs : nullptr;
    v.flows1 = reinterpret_cast<aof_flow *>(ws + L.l1_flows);
    v.hist1 = ws + L.l1_hist;
    v.blocks0 = d_blocks ? d_blocks : reinterpret_cast<aof_block *>(ws + L.l0_blocks);
    v.subdirs0 = nullptr;
    if (p.subpixel) v.subdirs0 = d_subdirs ? d_subdirs : ws + L.l0_subdirs;
    v.flows = d_flows;
    v.hist0 = ws + L.l0_hist;
    v.hints = p.tile == 16 ? reinterpret_cast<uint32_t *>(ws + L.hints) : nullptr;
    return v;
}

inline SearchArgs search_args(const BatchConfig &cfg, int level, const uint8_t *prev, const uint8_t *cur, int64_t stride,
                              aof_block *blocks, uint8_t *subdirs, const aof_flow *pred, const uint32_t *sums, int64_t n)
{
    const aof_params &p = cfg.params;
    SearchArgs a;
    a.prev = prev; a.cur = cur; a.pair_stride = stride;
    a.w = p.width >> level; a.h = p.height >> level;
    a.tile = p.tile; a.search = p.search;
    a.grid = level ? cfg.g1 : cfg.g0;
    a.feature_threshold = p.feature_threshold;
    a.value_threshold = value_threshold_u16(p);
    a.subpixel = p.subpixel;
    a.blocks = blocks; a.subdirs = p.subpixel ? subdirs : nullptr;
    a.pred = pred; a.sums = sums; a.level = level; a.n_pairs = n;
    a.hist_range = level_range(p, level);
    // 0 exhaustive, 1 pruned, 2 adaptive (16x16: a probe kernel judges every pair first; flat 8x8 launches:
    // choose_lane8 decides per launch from what the context's previous launches reported)
    a.prune = cfg.search_mode;
    a.hints = nullptr;   // (16x16 searches: set from the workspace by plan_batch)
    return a;
}

// Which search kernel serves `a`; the 16x16 tile's prune flag is resolved in *a.
inline SearchKind search_kind(const BatchConfig &cfg, SearchArgs *a)
{
    if (cfg.force_generic) return SK_GENERIC;
    // 8x8 tiles run lane-per-block straight from L2 (measured faster than LDS-staged strips on every
    // dense configuration: full lane use, no staging phases, no barriers)
    if (tile16_supported(*a)) return SK_TILE16;
    SearchArgs x = *a;   // the pruned steps' tables (68 B per block column) may not fit LDS where the exhaustive tile does: widths of ~3 000 px
    x.prune = 0;
    if (a->prune && tile16_supported(x)) {
        a->prune = 0;
        return SK_TILE16;
    }
    if (lane8_plan_supported(*a)) return lane8_group_plan(*a).ppw > 0 ? SK_LANE8_GROUP : SK_LANE8;
    return SK_GENERIC;
}

constexpr int64_t kSmallMaxPairs = 128;   // one-launch path for small pairs: measured faster than the separate kernels up to here

inline FlowTail flow_tail(const BatchConfig &cfg, int level, aof_flow *flows, const aof_flow *pred)
{
    const aof_params &p = cfg.params;
    FlowTail t;
    t.nblocks = (level ? cfg.g1 : cfg.g0).blocks(); t.range = level_range(p, level);
    t.hist_filter = p.hist_filter; t.min_valid = p.min_valid;
    t.flows = flows; t.pred = pred; t.emit_predictor = level ? 1 : 0;
    return t;
}

inline LevelPlan plan_level(const BatchConfig &cfg, SearchArgs a, const FlowTail &tail)
{
    const SearchKind kind = search_kind(cfg, &a);
    return {kind, kind == SK_TILE16 && a.subpixel && !tile16_refines(a), a, tail};
}

// k1_ready: the sequence pipeline's ingest has left K1's outputs already.
inline BatchPlan plan_batch(const BatchConfig &cfg, const BatchView &v, int64_t n, bool k1_ready)
{
    const aof_params &p = cfg.params;
    const bool two = p.pyramid_levels == 2, eq = p.mean_subtract != 0;
    const int64_t frame = (int64_t)p.width * p.height, l1_frame = (int64_t)(p.width / 2) * (p.height / 2);
    BatchPlan P = {};
    const SmallArgs &sm = P.sm = {search_args(cfg, 0, v.prev, v.cur, v.stride, v.blocks0, v.subdirs0, nullptr, v.sums, n),
                                  search_args(cfg, 1, v.l1_prev, v.l1_cur, l1_frame, v.blocks1, v.subdirs1, nullptr, v.sums, n),
                                  flow_tail(cfg, 0, v.flows, two ? v.flows1 : nullptr), flow_tail(cfg, 1, v.flows1, nullptr),
                                  v.sums, two ? 2 : 1};
    // level 0, under the level-1 predictor when there is one
    SearchArgs a0 = sm.l0;
    a0.pred = sm.t0.pred;
    a0.hints = v.hints;
    P.level[0] = plan_level(cfg, a0, sm.t0);

    // Small pairs (sparse grids, frames that fit LDS -- the reference's call shape): sums, pyramid, searches and
    // reductions of a pair in one launch, one workgroup per pair.  Large batches of such pairs keep the separate
    // kernels, whose grouped searches pack several pairs into a workgroup.
    P.small_class = !cfg.force_generic && !cfg.split_coarse && P.level[0].kind == SK_LANE8_GROUP &&
                    (!two || plan_level(cfg, sm.l1, sm.t1).kind == SK_LANE8_GROUP) && small_plan_make(sm).verdict == SMALL_OK;
    P.small = P.small_class && n <= kSmallMaxPairs;
    if (P.small || (!two && !eq)) return P;   // (one level without equalisation: no coarse pass)

    // K1C: sums, pyramid, level-1 search and predictor of a pair in one workgroup, the level-1 frames never
    // leave LDS (workspace regions l1_prev / l1_cur stay untouched)
    CoarseArgs &c = P.fused;
    c.prev = v.prev; c.cur = v.cur; c.pair_stride = v.stride;
    c.w = p.width; c.h = p.height; c.tile = p.tile; c.search = p.search; c.subpixel = p.subpixel;
    c.grid = cfg.g1;
    c.feature_threshold = p.feature_threshold;
    c.value_threshold = value_threshold_u16(p);
    c.sums = v.sums; c.blocks = v.blocks1; c.tail = sm.t1; c.n_pairs = n;
    c.first_generation = cfg.cus; c.stagger_groups = 0; c.stagger_ticks = 0;   // stagger chosen by the launcher
    if (two && !cfg.force_generic && !cfg.split_coarse && coarse_plan_of(P.fused).verdict == COARSE_OK) {
        P.coarse = COARSE_FUSED;
        return P;
    }
    P.coarse = COARSE_K1;
    // A frame sequence (aof.h: d_cur = d_prev + one frame, pair_stride = one frame): frame k is cur of pair k-1
    // and prev of pair k -- K1 sums and filters every frame once instead of twice.  The level-1 frames then
    // form a sequence of their own (n + 1 frames from the start of the workspace's two level-1 regions, which
    // are adjacent: 2 n frames of room), which the level-1 search views twice the same way.
    const bool seq = P.sequence = v.cur - v.prev == frame && v.stride == frame && v.l1_cur >= v.l1_prev;
    P.k1 = {v.prev, seq ? nullptr : v.cur, v.stride, p.width, p.height, v.l1_prev, seq ? nullptr : v.l1_cur, v.sums,
            seq ? n + 1 : n, seq ? 1 : 0};
    P.k1_pass = !(P.sequence && k1_ready);   // (the sequence pipeline's ingest has left sums and level-1 frames already)
    if (two) {
        SearchArgs a1 = sm.l1;
        if (P.sequence) a1.cur = v.l1_prev + l1_frame;
        a1.hints = v.hints;
        P.level[1] = plan_level(cfg, a1, sm.t1);
    }
    return P;
}

// ---- flat 8x8 launches: the one decision made per launch, by the executor ----

// ADAPTIVE search of the flat 8x8 kernel: does THIS launch run the pruned kernel?  The context goes by what its
// PREVIOUS launches reported (PruneReport; DESIGN.md, "per launch, on the host"): the pruned kernel while at least
// kPayingPct of their chunks pruned, else the exhaustive one with one pruned launch in kProbeEvery to look again.
// Speed only: every kernel writes the same records.
constexpr uint32_t kPayingPct = 40;
constexpr int kProbeEvery = 16;

inline bool adaptive_lane8_prunes(AdaptiveSearch &st, const SearchArgs &a)
{
    // level-1 searches and small launches: too few blocks per wave to carry a hint along
    if (a.level != 0 || !st.slots || !lane8_flat_plan(a, false, nullptr, 0).prune_large) return false;
    if (st.expected) {
        const uint32_t tag = st.launch_no & 0xFFFFu;
        uint32_t arrived = 0, paying = 0, seen = 0;
        for (uint32_t i = 0; i < st.expected && i < (uint32_t)kPruneSlots; i++) {
            const uint32_t w = __atomic_load_n(st.slots + i, __ATOMIC_RELAXED);
            if ((w >> 16) != tag) continue;
            arrived++;
            paying += (w >> 8) & 0xFFu;
            seen += w & 0xFFu;
        }
        if (arrived * 4 >= st.expected && seen) {   // (a launch still running has told enough after a quarter)
            st.stats.paying_pct = (int32_t)(paying * 100u / seen);
            st.belief = paying * 100u >= seen * kPayingPct ? 1 : 0;
            st.stats.belief = st.belief;
            st.stats.reports_read++;
        }
    }
    if (st.belief != 0) return true;
    if (++st.since_probe >= kProbeEvery) {
        st.since_probe = 0;
        return true;
    }
    return false;
}

// Capture state of the launch's stream: none, capturing, or the query itself failed.
enum Capture { CAPTURE_NONE, CAPTURE_ACTIVE, CAPTURE_UNKNOWN };

struct Lane8Launch {
    int prune;          // 0 the exhaustive kernel, 1 pruned, 2 pruned with the first chunk of every wave judging
    bool cols;          // the column walk (dense grids); otherwise the chunk walk or the exhaustive kernel
    bool fused;         // the reduction runs in the launch: no K3
    PruneReport rep;    // where the pruned kernel reports (slots == nullptr: nowhere)
};

// vm, vote_pairs, separate, captured: the context's vote memory and what InLaunchReduce (aof_ctx.hpp) says of it.
inline Lane8Launch choose_lane8(const BatchConfig &cfg, AdaptiveSearch &st, const SearchArgs &a, Capture cap, const VoteMem &vm,
                                int64_t vote_pairs, bool separate, bool captured)
{
    Lane8Launch l = {a.prune, false, false, {nullptr, 0, 1, 0}};
    if (l.prune && cfg.search_mode == AOF_SEARCH_ADAPTIVE) {
        // (where the caller switched the in-launch reduction on, launches that do not prune -- too small, or
        //  images on which it does not pay -- still get it: that kernel is the exhaustive one.  256 VGA pairs,
        //  two batches in flight: pruned + K3 40.9 us, exhaustive with the reduction in the launch 49.9 us)
        if (!adaptive_lane8_prunes(st, a)) {
            l.prune = 0;
            st.stats.exhaustive_launches++;
        } else {
            // a context that knows pruning pays starts every wave in the pruned code (optimistic, like
            // PRUNED); one that does not lets the first block (chunk) of every wave run exhaustively and judge
            l.prune = st.belief == 1 ? 1 : 2;
            if (++st.launch_no % 0x10000u == 0) st.launch_no++;   // (tag 0 = never written)
            l.rep.slots = st.slots;
            l.rep.launch_no = st.launch_no & 0xFFFFu;
            st.stats.pruned_launches++;
        }
    }
    SearchArgs x = a;
    x.prune = l.prune;
    // (dense grids prune as a column walk, whose lanes keep half of their window for the block below)
    l.cols = l.prune && lane8_cols_supported(x);
    // search + reduction in one launch where the vote memory can serve it (the chunk walk has no such form).  A captured
    // graph holding one replays whenever its owner likes, without a `done` event: eager launches keep to K3 from then
    // on.  A stream whose capture state cannot be queried takes K3 and leaves that state alone.
    const bool fits = l.cols ? lane8_cols_votes_supported(x, vm, vote_pairs)
                             : (!l.prune && lane8_votes_verdict(x, &vm, vote_pairs) == VOTES_OK);
    l.fused = fits && !separate && (cap == CAPTURE_ACTIVE || (cap == CAPTURE_NONE && !captured));
    return l;
}

}  // namespace aof
