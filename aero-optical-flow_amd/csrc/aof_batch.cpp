// aof_flow_batch_device (include/aof.h): the plan of a batch (BatchPlan: every kernel choice, made once before the first
// launch; the sequences per configuration are in DESIGN.md "Kernels") and the executor that enqueues it on the caller's
// stream.  Nothing here allocates or synchronises, so the sequence can be captured into a hipGraph.
#include <cerrno>

#include "aof_ctx.hpp"

using namespace aof;

namespace {

// Event timing of one kernel id around the launches in its scope (aof_set_profiling).
struct Timed {
    aof_ctx *ctx; int id; hipStream_t s; bool on; int slot;
    Timed(aof_ctx *c, int k, hipStream_t st)
        : ctx(c), id(k), s(st), on(c->prof.on && !c->capturing && ((c->prof.mask >> k) & 1u)),
          slot((int)(c->prof.count[k] % AOF_PROFILE_RING))
    {
        if (on) (void)hipEventRecord(ctx->prof.ev[id][slot][0], s);
    }
    ~Timed() { if (on) { (void)hipEventRecord(ctx->prof.ev[id][slot][1], s); ctx->prof.count[id]++; } }
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

BatchView batch_view(const aof_ctx *ctx, const aof_ws_layout &L, const uint8_t *d_prev, const uint8_t *d_cur,
                     int64_t pair_stride, aof_block *d_blocks, uint8_t *d_subdirs, aof_flow *d_flows, void *d_workspace)
{
    const aof_params &p = ctx->params;
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

SearchArgs search_args(const aof_ctx *ctx, int level, const uint8_t *prev, const uint8_t *cur, int64_t stride,
                       aof_block *blocks, uint8_t *subdirs, const aof_flow *pred, const uint32_t *sums, int64_t n)
{
    const aof_params &p = ctx->params;
    SearchArgs a;
    a.prev = prev; a.cur = cur; a.pair_stride = stride;
    a.w = p.width >> level; a.h = p.height >> level;
    a.tile = p.tile; a.search = p.search;
    a.grid = level ? ctx->g1 : ctx->g0;
    a.feature_threshold = p.feature_threshold;
    a.value_threshold = value_threshold_u16(p);
    a.subpixel = p.subpixel;
    a.blocks = blocks; a.subdirs = p.subpixel ? subdirs : nullptr;
    a.pred = pred; a.sums = sums; a.level = level; a.n_pairs = n;
    a.hist_range = level_range(p, level);
    // 0 exhaustive, 1 pruned, 2 adaptive (16x16: a probe kernel judges every pair first; flat 8x8 launches:
    // choose_lane8 decides per launch from what the context's previous launches reported)
    a.prune = ctx->search_mode;
    a.hints = nullptr;   // (16x16 searches: set from the workspace by plan_batch)
    return a;
}

// Which search kernel serves `a`; the 16x16 tile's prune flag is resolved in *a.
SearchKind search_kind(const aof_ctx *ctx, SearchArgs *a)
{
    if (ctx->force_generic) return SK_GENERIC;
    // 8x8 tiles run lane-per-block straight from L2 (measured faster than LDS-staged strips on every
    // dense configuration: full lane use, no staging phases, no barriers)
    if (tile16_supported(*a)) return SK_TILE16;
    SearchArgs x = *a;   // the pruned steps' tables (68 B per block column) may not fit LDS where the exhaustive tile does: widths of ~3 000 px
    x.prune = 0;
    if (a->prune && tile16_supported(x)) {
        a->prune = 0;
        return SK_TILE16;
    }
    if (lane8_supported(*a)) return lane8_group(*a) > 0 ? SK_LANE8_GROUP : SK_LANE8;
    return SK_GENERIC;
}

constexpr int64_t kSmallMaxPairs = 128;   // one-launch path for small pairs: measured faster than the separate kernels up to here

FlowTail flow_tail(const aof_ctx *ctx, int level, aof_flow *flows, const aof_flow *pred)
{
    const aof_params &p = ctx->params;
    FlowTail t;
    t.nblocks = (level ? ctx->g1 : ctx->g0).blocks(); t.range = level_range(p, level);
    t.hist_filter = p.hist_filter; t.min_valid = p.min_valid;
    t.flows = flows; t.pred = pred; t.emit_predictor = level ? 1 : 0;
    return t;
}

LevelPlan plan_level(const aof_ctx *ctx, SearchArgs a, const FlowTail &tail)
{
    const SearchKind kind = search_kind(ctx, &a);
    return {kind, kind == SK_TILE16 && a.subpixel && !tile16_refines(a), a, tail};
}

// const on the context, no HIP calls.  k1_ready: the sequence pipeline's ingest has left K1's outputs already.
BatchPlan plan_batch(const aof_ctx *ctx, const BatchView &v, int64_t n, bool k1_ready)
{
    const aof_params &p = ctx->params;
    const bool two = p.pyramid_levels == 2, eq = p.mean_subtract != 0;
    const int64_t frame = (int64_t)p.width * p.height, l1_frame = (int64_t)(p.width / 2) * (p.height / 2);
    BatchPlan P = {};
    const SmallArgs &sm = P.sm = {search_args(ctx, 0, v.prev, v.cur, v.stride, v.blocks0, v.subdirs0, nullptr, v.sums, n),
                                  search_args(ctx, 1, v.l1_prev, v.l1_cur, l1_frame, v.blocks1, v.subdirs1, nullptr, v.sums, n),
                                  flow_tail(ctx, 0, v.flows, two ? v.flows1 : nullptr), flow_tail(ctx, 1, v.flows1, nullptr),
                                  v.sums, two ? 2 : 1};
    // level 0, under the level-1 predictor when there is one
    SearchArgs a0 = sm.l0;
    a0.pred = sm.t0.pred;
    a0.hints = v.hints;
    P.level[0] = plan_level(ctx, a0, sm.t0);

    // Small pairs (sparse grids, frames that fit LDS -- the reference's call shape): sums, pyramid, searches and
    // reductions of a pair in one launch, one workgroup per pair.  Large batches of such pairs keep the separate
    // kernels, whose grouped searches pack several pairs into a workgroup.
    P.small_class = !ctx->force_generic && !ctx->split_coarse && P.level[0].kind == SK_LANE8_GROUP &&
                    (!two || plan_level(ctx, sm.l1, sm.t1).kind == SK_LANE8_GROUP) && flow_small_supported(sm);
    P.small = P.small_class && n <= kSmallMaxPairs;
    if (P.small || (!two && !eq)) return P;   // (one level without equalisation: no coarse pass)

    // K1C: sums, pyramid, level-1 search and predictor of a pair in one workgroup, the level-1 frames never
    // leave LDS (workspace regions l1_prev / l1_cur stay untouched)
    CoarseArgs &c = P.fused;
    c.prev = v.prev; c.cur = v.cur; c.pair_stride = v.stride;
    c.w = p.width; c.h = p.height; c.tile = p.tile; c.search = p.search; c.subpixel = p.subpixel;
    c.grid = ctx->g1;
    c.feature_threshold = p.feature_threshold;
    c.value_threshold = value_threshold_u16(p);
    c.sums = v.sums; c.blocks = v.blocks1; c.tail = sm.t1; c.n_pairs = n;
    c.first_generation = ctx->cus; c.stagger_groups = 0; c.stagger_ticks = 0;   // stagger chosen by the launcher
    if (two && !ctx->force_generic && !ctx->split_coarse && coarse_fused_supported(P.fused)) {
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
        P.level[1] = plan_level(ctx, a1, sm.t1);
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

bool adaptive_lane8_prunes(AdaptiveSearch &st, const SearchArgs &a)
{
    // level-1 searches and small launches: too few blocks per wave to carry a hint along
    if (a.level != 0 || !st.slots || !lane8_prune_large(a)) return false;
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

VoteMem vote_mem(const aof_ctx *ctx) { return {ctx->votes.mem, kVoteStride, ctx->h_fault, ctx->votes.deadline_ticks}; }

Lane8Launch choose_lane8(aof_ctx *ctx, const SearchArgs &a, Capture cap)
{
    Lane8Launch l = {a.prune, false, false, {nullptr, 0, 1, 0}};
    if (l.prune && ctx->search_mode == AOF_SEARCH_ADAPTIVE) {
        // (where the caller switched the in-launch reduction on, launches that do not prune -- too small, or
        //  images on which it does not pay -- still get it: that kernel is the exhaustive one.  256 VGA pairs,
        //  two batches in flight: pruned + K3 40.9 us, exhaustive with the reduction in the launch 49.9 us)
        AdaptiveSearch &st = ctx->adapt;
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
    const VoteMem vm = vote_mem(ctx);
    const bool fits = l.cols ? lane8_cols_votes_supported(x, vm, ctx->votes.pairs)
                             : (!l.prune && lane8_votes_supported(x, vm, ctx->votes.pairs));
    l.fused = fits && !ctx->votes.separate && (cap == CAPTURE_ACTIVE || (cap == CAPTURE_NONE && !ctx->votes.captured));
    return l;
}

// A flat 8x8 launch as choose_lane8 decides it.  *reduced: the reduction ran in the launch.  Returns a HIP error,
// or a negative code already reported.
int launch_lane8(aof_ctx *ctx, SearchArgs a, const FlowTail &tail, hipStream_t s, bool *reduced)
{
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    const Capture cap = hipStreamIsCapturing(s, &status) != hipSuccess ? CAPTURE_UNKNOWN
                        : status == hipStreamCaptureStatusNone         ? CAPTURE_NONE
                                                                       : CAPTURE_ACTIVE;
    Lane8Launch l = choose_lane8(ctx, a, cap);
    a.prune = l.prune;
    // launches on another stream than the last one wait for that one first (the records are shared)
    const bool eager = cap == CAPTURE_NONE;
    if (l.fused && eager && ctx->votes.used && ctx->votes.stream != s && hipStreamWaitEvent(s, ctx->votes.done, 0) != hipSuccess)
        return fail(ctx, -EIO, "cannot order the launch behind the context's previous one");
    const VoteMem vm = vote_mem(ctx);
    const FlowTail *t = l.fused ? &tail : nullptr;
    const VoteMem *m = l.fused ? &vm : nullptr;
    PruneReport *rep = l.prune ? &l.rep : nullptr;
    int rc = l.cols ? launch_search_lane8_cols(a, s, rep, t, m) : launch_search_lane8(a, s, t, m, rep);
    if (!rc && l.fused && eager) {
        rc = (int)hipEventRecord(ctx->votes.done, s);
        ctx->votes.stream = s;
        ctx->votes.used = true;
    } else if (!rc && l.fused) {
        ctx->votes.captured = true;   // (replays are the owner's to order: include/aof.h)
    }
    *reduced = l.fused;
    if (rep && l.rep.slots) ctx->adapt.expected = l.rep.expected;
    return rc;
}

// ---- the executor ----

// One level: its search, then K3 unless the search kernel reduced itself.
int enqueue_level(aof_ctx *ctx, const LevelPlan &l, uint8_t *hist, int kid_search, int kid_reduce, hipStream_t s)
{
    bool reduced = l.kind == SK_LANE8_GROUP;   // (refines in the same lane and finalises the flow records)
    {
        Timed t(ctx, kid_search, s);
        int rc;
        switch (l.kind) {
        case SK_TILE16:   // (refines out of its LDS tile when directions are wanted)
            rc = launch_search_tile16(l.a, s, ctx->tile16_verdicts);
            if (!rc && l.refine) rc = launch_refine(l.a, s);
            break;
        case SK_LANE8_GROUP:
            rc = launch_flow_lane8(l.a, l.tail, s);
            break;
        case SK_LANE8:
            rc = launch_lane8(ctx, l.a, l.tail, s, &reduced);
            if (rc < 0) return rc;
            break;
        default:
            rc = launch_search_generic(l.a, s);
        }
        if (rc) return fail(ctx, -EIO, "search launch: %s", hipGetErrorString((hipError_t)rc));
    }
    if (reduced) return 0;
    const ReduceArgs r = {l.a.blocks, l.a.subdirs, value_threshold_u16(ctx->params), l.tail, l.a.n_pairs, nullptr, 0,
                          reinterpret_cast<uint32_t *>(hist)};
    Timed t(ctx, kid_reduce, s);
    const int rc = launch_reduce(r, s);
    if (rc) return fail(ctx, -EIO, "reduce launch: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}

// aof_flow_batch_device: checks, plan, launches.  k1_ready: the sequence pipeline's ingest has left K1's outputs in the
// workspace.
int flow_batch(aof_ctx *ctx, const uint8_t *d_prev, const uint8_t *d_cur, int64_t pair_stride, int64_t n_pairs,
               aof_block *d_blocks, uint8_t *d_subdirs, aof_flow *d_flows, void *d_workspace, size_t workspace_bytes,
               void *stream, bool k1_ready)
{
    if (!ctx) return -EINVAL;
    if (n_pairs < 0 || (n_pairs > 0 && (!d_prev || !d_cur || !d_flows)))
        return fail(ctx, -EINVAL, "null frame or flow pointer");
    if (int sticky = sticky_error(ctx)) return sticky;
    if (n_pairs == 0) return 0;
    const aof_params &p = ctx->params;
    if (pair_stride < (int64_t)p.width * p.height && n_pairs > 1)
        return fail(ctx, -EINVAL, "pair_stride smaller than a frame");
    aof_ws_layout L;
    int rc = aof_workspace_layout(&p, n_pairs, &L);
    if (rc) return fail(ctx, rc, "bad workspace layout");
    if (!d_workspace || workspace_bytes < L.total_bytes)
        return fail(ctx, -ENOSPC, "workspace %zu B < required %zu B", workspace_bytes, L.total_bytes);
    if (!aligned(d_workspace, 256))
        return fail(ctx, -EINVAL, "workspace must be 256-byte aligned");
    if (!aligned(d_blocks, 4) || !aligned(d_flows, 4))
        return fail(ctx, -EINVAL, "block and flow records must be 4-byte aligned");
    if ((rc = device_check(ctx))) return rc;
    const BatchView v = batch_view(ctx, L, d_prev, d_cur, pair_stride, d_blocks, d_subdirs, d_flows, d_workspace);
    const BatchPlan P = plan_batch(ctx, v, n_pairs, k1_ready);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (P.small) {
        Timed t(ctx, AOF_K_SEARCH, s);
        if ((rc = launch_flow_small(P.sm, s))) return fail(ctx, -EIO, "small-pair launch: %s", hipGetErrorString((hipError_t)rc));
        return 0;
    }
    if (P.coarse == COARSE_FUSED) {
        Timed t(ctx, AOF_K_PYRAMID, s);
        if ((rc = launch_coarse_fused(P.fused, s))) return fail(ctx, -EIO, "coarse launch: %s", hipGetErrorString((hipError_t)rc));
    }
    if (P.k1_pass) {
        Timed t(ctx, AOF_K_PYRAMID, s);
        if ((rc = launch_pyramid(P.k1, s))) return fail(ctx, -EIO, "pyramid launch: %s", hipGetErrorString((hipError_t)rc));
    }
    if (P.coarse == COARSE_K1 && p.pyramid_levels == 2 && (rc = enqueue_level(ctx, P.level[1], v.hist1, AOF_K_SEARCH_L1, AOF_K_REDUCE_L1, s))) return rc;
    return enqueue_level(ctx, P.level[0], v.hist0, AOF_K_SEARCH, AOF_K_REDUCE, s);
}

}  // namespace

namespace aof {

bool plan_small_pair(const aof_ctx *ctx, const uint8_t *prev, const uint8_t *cur, aof_flow *flow, SmallArgs *sm)
{
    const aof_params &p = ctx->params;
    aof_ws_layout L;
    aof_workspace_layout(&p, 1, &L);
    const BatchView v = batch_view(ctx, L, prev, cur, (int64_t)p.width * p.height, ctx->host.d_blocks, ctx->host.d_subdirs,
                                   flow, ctx->host.d_ws);
    const BatchPlan P = plan_batch(ctx, v, 1, false);
    *sm = P.sm;
    return P.small;
}

bool plan_small_batch(const aof_ctx *ctx, const uint8_t *prev, const uint8_t *cur, int64_t stride, int64_t n, aof_flow *flows,
                      void *d_workspace, SmallArgs *sm)
{
    aof_ws_layout L;
    if (n < 1 || aof_workspace_layout(&ctx->params, n, &L)) return false;
    const BatchView v = batch_view(ctx, L, prev, cur, stride, nullptr, nullptr, flows, d_workspace);
    const BatchPlan P = plan_batch(ctx, v, n, false);
    *sm = P.sm;
    return P.small_class;
}

int bank_path(const aof_ctx *ctx) { return ctx->bank_path; }
void set_bank_path(aof_ctx *ctx, int path) { ctx->bank_path = path; }
BankTables &bank_tables(aof_ctx *ctx) { return ctx->bank; }

// Would a sequence-view call (frames viewed twice, n_pairs = frames - 1) run K1 as a pass of its own?  The sequence
// pipeline asks, because its ingest kernel can leave K1's outputs (pixel sums at ws + L.sums, one level-1 frame per
// FRAME from ws + L.l1_prev on) itself.
bool sequence_runs_k1(aof_ctx *ctx, const uint8_t *d_frames, int64_t n_pairs, void *d_workspace)
{
    const aof_params &p = ctx->params;
    aof_ws_layout L;
    if (n_pairs < 1 || aof_workspace_layout(&p, n_pairs, &L)) return false;
    const int64_t frame = (int64_t)p.width * p.height;
    const BatchView v = batch_view(ctx, L, d_frames, d_frames + frame, frame, nullptr, nullptr, nullptr, d_workspace);
    return plan_batch(ctx, v, n_pairs, false).k1_pass;
}

// aof_flow_batch_device on the sequence view of `d_frames`; k1_ready: K1's outputs are in the workspace already.
int flow_sequence(aof_ctx *ctx, const uint8_t *d_frames, int64_t n_pairs, aof_flow *d_flows, void *d_workspace,
                  size_t workspace_bytes, void *stream, bool k1_ready)
{
    const int64_t frame = (int64_t)ctx->params.width * ctx->params.height;
    return flow_batch(ctx, d_frames, d_frames + frame, frame, n_pairs, nullptr, nullptr, d_flows, d_workspace,
                      workspace_bytes, stream, k1_ready);
}

}  // namespace aof

extern "C" {

int aof_flow_batch_device(aof_ctx *ctx, const uint8_t *d_prev, const uint8_t *d_cur, int64_t pair_stride, int64_t n_pairs,
                          aof_block *d_blocks, uint8_t *d_subdirs, aof_flow *d_flows, void *d_workspace,
                          size_t workspace_bytes, void *stream)
{
    return flow_batch(ctx, d_prev, d_cur, pair_stride, n_pairs, d_blocks, d_subdirs, d_flows, d_workspace,
                      workspace_bytes, stream, false);
}

const char *aof_search_variant(const aof_ctx *ctx)
{
    if (!ctx) return "";
    // which search kernel will level 0 use? (the plan of one pair at null, i.e. aligned, addresses)
    BatchView v = {};
    v.stride = (int64_t)ctx->params.width * ctx->params.height;
    switch (plan_batch(ctx, v, 1, false).level[0].kind) {
    case SK_TILE16: return "tile16_lds";
    case SK_GENERIC: return "generic";
    default: return "lane8";
    }
}

}  // extern "C"
