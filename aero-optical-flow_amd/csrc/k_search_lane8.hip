// K2 (lane8), host side: which of the lane-per-block kernels serves a launch.  The launch geometry of the flat kernels is
// lane8_flat_plan's (aof_lane8_plan.hpp), that of the grouped kernel lane8_group_plan's (aof_small_plan.hpp).  The kernels
// themselves are templates in aof_lane8_kernels.hpp, each shipped instantiation compiled in its own translation unit
// (k_lane8_*.hip) together with the launch function declared below.
#include <hip/hip_runtime.h>

#include "aof_engine_args.hpp"
#include "aof_fastdiv.hpp"
#include "aof_lane8_launch.hpp"
#include "aof_lane8_plan.hpp"    // the plan of the flat launches, the slices of every launch here
#include "aof_small_plan.hpp"    // the grouped plan

namespace aof {

namespace {

// The arguments of slice p (lane8_flat_plan: at most kMaxItems (pair, block) items each).
SearchArgs slice_args(const SearchArgs &a, const Lane8FlatPlan &p)
{
    SearchArgs s = a;
    s.n_pairs = p.pairs;
    s.prev += p.frame_off;
    s.cur += p.frame_off;
    s.blocks += p.block_off;
    if (s.subdirs) s.subdirs += p.block_off;
    if (s.pred) s.pred += p.pred_off;
    if (s.sums) s.sums += p.sums_off;
    s.div_nb = fastdiv_make((uint32_t)a.grid.blocks());
    s.div_nx = fastdiv_make((uint32_t)a.grid.nx);
    return s;
}

FlowTail slice_tail(const FlowTail &tail, const Lane8FlatPlan &p)
{
    FlowTail t = tail;
    t.flows += p.pred_off;
    if (t.pred) t.pred += p.pred_off;
    return t;
}

}  // namespace

// The launcher only launches: every number below is lane8_flat_plan's.
int launch_search_lane8(const SearchArgs &a, void *stream, const FlowTail *tail, const VoteMem *votes, PruneReport *report)
{
    if (report) report->expected = 0;
    if (a.n_pairs == 0) return 0;
    if (a.subpixel && !a.subdirs) return (int)hipErrorInvalidValue;
    const bool fused = tail && votes;   // search + reduction in one launch
    const int64_t slices = lane8_flat_plan(a, fused, votes, 0).slices;
    for (int64_t k = 0; k < slices; k++) {
        const Lane8FlatPlan p = lane8_flat_plan(a, fused, votes, 0, k);
        const SearchArgs s = slice_args(a, p);
        int rc;
        if (p.kind == LANE8_FUSED) {
            auto fn = s.sums ? (s.subpixel ? launch_k_flow_lane8_flat_tt : launch_k_flow_lane8_flat_ft)
                             : (s.subpixel ? launch_k_flow_lane8_flat_tf : launch_k_flow_lane8_flat_ff);
            rc = fn(s, (uint32_t)p.items, (uint32_t)p.wgs, (uint32_t)p.grid, p.threads, slice_tail(*tail, p), *votes, stream);
        } else if (p.kind == LANE8_CHUNK_WALK) {
            PruneReport rep = {nullptr, 0, 1, 0};
            if (report && report->slots && k == 0) {   // (launches of more than 2^31 items: the first slice reports)
                rep = *report;
                rep.stride = p.stride;
                report->stride = p.stride;
                report->expected = p.expected;
            }
            rc = (s.subpixel ? launch_k_search_lane8_pruned_t : launch_k_search_lane8_pruned_f)(s, (uint32_t)p.items, (uint32_t)p.wgs, p.spw, rep,
                                                                                                static_cast<hipStream_t>(stream));
        } else {
            // (EQ = false: a launch without pixel sums runs a kernel without any equalisation code)
            auto fn = s.sums ? (s.subpixel ? launch_k_search_lane8_tt : launch_k_search_lane8_ft)
                             : (s.subpixel ? launch_k_search_lane8_tf : launch_k_search_lane8_ff);
            rc = fn(s, (uint32_t)p.items, (uint32_t)p.wgs, p.threads, static_cast<hipStream_t>(stream));
        }
        if (rc) return rc;
    }
    return 0;
}

int launch_flow_lane8(const SearchArgs &a, const FlowTail &tail, void *stream)
{
    if (a.n_pairs == 0) return 0;
    if (lane8_group_plan(a).ppw == 0) return (int)hipErrorInvalidValue;
    if (a.subpixel && !a.subdirs) return (int)hipErrorInvalidValue;
    const int64_t slices = lane8_flat_plan(a, false, nullptr, 0).slices;   // (the slices are the flat launches')
    for (int64_t k = 0; k < slices; k++) {
        const Lane8FlatPlan p = lane8_flat_plan(a, false, nullptr, 0, k);
        const SearchArgs s = slice_args(a, p);
        const Lane8GroupPlan g = lane8_group_plan(s);   // (of the slice: its pairs)
        const int rc = (s.subpixel ? launch_k_flow_lane8_t : launch_k_flow_lane8_f)(s, slice_tail(tail, p), g.ppw, (uint32_t)g.wgs, g.lds, stream);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace aof
