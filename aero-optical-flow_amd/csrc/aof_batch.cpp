// aof_flow_batch_device (include/aof.h): the executor that enqueues the plan of a batch (plan_batch and choose_lane8,
// aof_batch_plan.hpp) on the caller's stream.  Nothing here allocates or synchronises, so the sequence can be captured
// into a hipGraph.
#include <cerrno>

#include "aof_batch_plan.hpp"
#include "aof_ctx.hpp"
#include "aof_engine_args.hpp"
#include "aof_host.hpp"

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

VoteMem vote_mem(const aof_ctx *ctx) { return {ctx->votes.mem, kVoteStride, ctx->h_fault, ctx->votes.deadline_ticks}; }

// A flat 8x8 launch as choose_lane8 decides it.  *reduced: the reduction ran in the launch.  Returns a HIP error,
// or a negative code already reported.
int launch_lane8(aof_ctx *ctx, SearchArgs a, const FlowTail &tail, hipStream_t s, bool *reduced)
{
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    const Capture cap = hipStreamIsCapturing(s, &status) != hipSuccess ? CAPTURE_UNKNOWN
                        : status == hipStreamCaptureStatusNone         ? CAPTURE_NONE
                                                                       : CAPTURE_ACTIVE;
    const VoteMem vm = vote_mem(ctx);
    Lane8Launch l = choose_lane8(ctx->cfg, ctx->adapt, a, cap, vm, ctx->votes.pairs, ctx->votes.separate, ctx->votes.captured);
    a.prune = l.prune;
    // launches on another stream than the last one wait for that one first (the records are shared)
    const bool eager = cap == CAPTURE_NONE;
    if (l.fused && eager && ctx->votes.used && ctx->votes.stream != s && hipStreamWaitEvent(s, ctx->votes.done, 0) != hipSuccess)
        return fail(ctx, -EIO, "cannot order the launch behind the context's previous one");
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
    const ReduceArgs r = {l.a.blocks, l.a.subdirs, value_threshold_u16(ctx->cfg.params), l.tail, l.a.n_pairs, nullptr, 0,
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
    const aof_params &p = ctx->cfg.params;
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
    const BatchView v = batch_view(ctx->cfg, L, d_prev, d_cur, pair_stride, d_blocks, d_subdirs, d_flows, d_workspace);
    const BatchPlan P = plan_batch(ctx->cfg, v, n_pairs, k1_ready);
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
    const aof_params &p = ctx->cfg.params;
    aof_ws_layout L;
    aof_workspace_layout(&p, 1, &L);
    const BatchView v = batch_view(ctx->cfg, L, prev, cur, (int64_t)p.width * p.height, ctx->host.d_blocks, ctx->host.d_subdirs,
                                   flow, ctx->host.d_ws);
    const BatchPlan P = plan_batch(ctx->cfg, v, 1, false);
    *sm = P.sm;
    return P.small;
}

bool plan_small_batch(const aof_ctx *ctx, const uint8_t *prev, const uint8_t *cur, int64_t stride, int64_t n, aof_flow *flows,
                      void *d_workspace, SmallArgs *sm)
{
    aof_ws_layout L;
    if (n < 1 || aof_workspace_layout(&ctx->cfg.params, n, &L)) return false;
    const BatchView v = batch_view(ctx->cfg, L, prev, cur, stride, nullptr, nullptr, flows, d_workspace);
    const BatchPlan P = plan_batch(ctx->cfg, v, n, false);
    *sm = P.sm;
    return P.small_class;
}

bool plan_small_params(const aof_params *p, SmallArgs *sm)
{
    aof_ws_layout L;
    *sm = SmallArgs{};
    if (aof_params_check(p) || aof_workspace_layout(p, 1, &L)) return false;
    BatchConfig cfg = {};
    cfg.params = *p;
    cfg.cus = 256;
    cfg.search_mode = AOF_SEARCH_ADAPTIVE;
    grid_for_level(*p, 0, &cfg.g0);
    if (p->pyramid_levels == 2) grid_for_level(*p, 1, &cfg.g1);
    // (never dereferenced: the plan looks at alignments and at which outputs exist)
    uint8_t *at = reinterpret_cast<uint8_t *>(uintptr_t(256));
    const BatchView v = batch_view(cfg, L, at, at, (int64_t)p->width * p->height, nullptr, nullptr, reinterpret_cast<aof_flow *>(at), at);
    const BatchPlan P = plan_batch(cfg, v, 1, false);
    *sm = P.sm;
    return P.small_class;
}

// Would a sequence-view call (frames viewed twice, n_pairs = frames - 1) run K1 as a pass of its own?  The sequence
// pipeline asks, because its ingest kernel can leave K1's outputs (pixel sums at ws + L.sums, one level-1 frame per
// FRAME from ws + L.l1_prev on) itself.
bool sequence_runs_k1(aof_ctx *ctx, const uint8_t *d_frames, int64_t n_pairs, void *d_workspace)
{
    const aof_params &p = ctx->cfg.params;
    aof_ws_layout L;
    if (n_pairs < 1 || aof_workspace_layout(&p, n_pairs, &L)) return false;
    const int64_t frame = (int64_t)p.width * p.height;
    const BatchView v = batch_view(ctx->cfg, L, d_frames, d_frames + frame, frame, nullptr, nullptr, nullptr, d_workspace);
    return plan_batch(ctx->cfg, v, n_pairs, false).k1_pass;
}

// aof_flow_batch_device on the sequence view of `d_frames`; k1_ready: K1's outputs are in the workspace already.
int flow_sequence(aof_ctx *ctx, const uint8_t *d_frames, int64_t n_pairs, aof_flow *d_flows, void *d_workspace,
                  size_t workspace_bytes, void *stream, bool k1_ready)
{
    const int64_t frame = (int64_t)ctx->cfg.params.width * ctx->cfg.params.height;
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
    v.stride = (int64_t)ctx->cfg.params.width * ctx->cfg.params.height;
    switch (plan_batch(ctx->cfg, v, 1, false).level[0].kind) {
    case SK_TILE16: return "tile16_lds";
    case SK_GENERIC: return "generic";
    default: return "lane8";
    }
}

}  // extern "C"
