// K2, pruned 8x8 search on DENSE grids, column walk: host side (segments, launch geometry).  The kernels are templates in
// aof_cols8_kernels.hpp, each shipped instantiation compiled in its own translation unit (k_cols8_*.hip).
#include <hip/hip_runtime.h>

#include "aof_cols8_plan.hpp"
#include "aof_engine_args.hpp"
#include "aof_lane8_launch.hpp"

namespace aof {

int launch_search_lane8_cols(const SearchArgs &a, void *stream, PruneReport *report, const FlowTail *tail, const VoteMem *votes)
{
    if (report) report->expected = 0;
    if (a.n_pairs == 0) return 0;
    if (!lane8_cols_supported(a) || (a.subpixel && !a.subdirs)) return (int)hipErrorInvalidValue;
    const int64_t per = cols_plan_make(a.grid, a.w, a.h, a.pair_stride, reinterpret_cast<uintptr_t>(a.cur), a.n_pairs).per;
    for (int64_t done = 0; done < a.n_pairs; done += per) {
        // (segments, short segments for the pairs behind the last full generation of waves, alignment: aof_cols8_plan.hpp)
        const ColsLaunch l = cols_plan_make(a.grid, a.w, a.h, a.pair_stride, reinterpret_cast<uintptr_t>(a.cur), a.n_pairs, done);
        const ColsPlan &plan = l.plan;
        SearchArgs s = a;
        s.n_pairs = l.pairs;
        s.prev += done * a.pair_stride;
        s.cur += done * a.pair_stride;
        s.blocks += done * a.grid.blocks();
        if (s.subdirs) s.subdirs += done * a.grid.blocks();
        if (s.pred) s.pred += done;
        if (s.sums) s.sums += done * 4;
        // a launch of one or two generations of waves ends sooner with one-wave workgroups, whose slots free up wave by
        // wave for the other batch in flight (as lane8_flat_threads does for the exhaustive kernel, aof_lane8_plan.hpp)
        // (one-wave workgroups for launches of one or two generations of waves, as the exhaustive kernel has them, measure
        //  the same within the spread of 200-step runs: profiles/r05_small_launch_shape.txt)
        const int threads = kColsThreads;
        const int64_t wgs = l.wgs;
        PruneReport rep = {nullptr, 0, 1, 0};
        if (report && report->slots && done == 0) {
            rep = *report;
            rep.stride = (uint32_t)((wgs + kPruneSlots - 1) / kPruneSlots);
            report->stride = rep.stride;
            report->expected = (uint32_t)((wgs + rep.stride - 1) / rep.stride);
        }
        int rc;
        if (tail && votes) {
            if (done != 0 || s.n_pairs != a.n_pairs) return (int)hipErrorInvalidValue;   // (lane8_cols_votes_supported)
            ColsVotes cv;
            cv.search_wgs = (uint32_t)wgs;
            cv.tail = *tail;
            cv.votes = *votes;
            const int64_t finalisers = (s.n_pairs + (threads >> 6) - 1) / (threads >> 6);   // one wave per pair
            rc = (s.subpixel ? launch_k_flow_lane8_cols_t : launch_k_flow_lane8_cols_f)(s, plan, rep, cv, (uint32_t)(wgs + finalisers), threads, stream);
        } else {
            rc = (s.subpixel ? launch_k_search_lane8_cols_t : launch_k_search_lane8_cols_f)(s, plan, rep, (uint32_t)wgs, threads, stream);
        }
        if (rc) return rc;
    }
    return 0;
}

}  // namespace aof
