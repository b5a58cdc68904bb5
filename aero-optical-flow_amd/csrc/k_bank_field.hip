// The stream bank's motion field (aof_bank_field_device; include/aof.h "the stream bank's motion field"): behind a tick,
// per stream, the fit of the pair the tick ran -- over the level-0 block records the tick left in the bank's scratch
// region -- and the step that integrates it over the rate limiter's window.  A translation unit of its own: nothing
// another kernel file compiles to moves.  The fit is field_fit (aof_field_fit.hpp, the text k_field.hip compiles), the step
// is aof_bank_field_step.hpp, which aof_bank_field_host runs; this file is the two forms of them over a bank, shaped like
// k_field's:
//   * k_bank_field<64, 1>: a wave per stream, four streams per workgroup, for grids of at most 256 blocks -- every
//     configuration the one-launch tick takes; k_bank_field<256, 5>: a workgroup per stream above that.
//   * the group reads its tick record FIRST, from an address that is uniform in the group (the stream's number goes
//     through readfirstlane): quality and frame decide, uniformly, whether the stream ran a pair.  A stream without one --
//     idle, refused by its sensor record, or on its first frame -- loads no block: what lies in its part of the scratch
//     region is stale on the one-launch path and computed for nobody on the composed path.
//   * lane 0 of the group runs the step and is the only lane that stores: the pair's fit (if the caller wants it), the
//     tick's output record and the stream's state -- 64, 48 and 64 bytes.  A stream without a frame stores no state.
// The bank and the tick records are only read.  The launch ends with a system-scope release behind its stores: records
// kept in pinned host memory are there for a host that sees the tag of a collect call enqueued behind this launch.
#include "aof_device.hpp"   // (the HIP runtime first: the rule headers' qualifiers are its)
#include "aof_bank_field_step.hpp"
#include "aof_fastdiv.hpp"
#include "aof_field_fit.hpp"

namespace aof {

namespace {

constexpr int kThreads = kFieldThreads;
constexpr int kTickWords = sizeof(aof_tick_record) / 4;

template <int GROUP, int KEEP>
__global__ __launch_bounds__(kThreads) void k_bank_field(BankFieldArgs a)
{
    constexpr int kGroups = kThreads / GROUP;
    const int grp = (int)threadIdx.x / GROUP, tid = (int)threadIdx.x % GROUP;
    const int s = __builtin_amdgcn_readfirstlane((int)blockIdx.x * kGroups + grp);   // (whole waves share a stream)
    if (GROUP < kThreads && s >= a.n_streams) return;   // whole waves only: no barrier is skipped

    // the stream's tick record, the same words for every lane of the group
    const uint32_t *rw = a.records + (size_t)s * kTickWords;
    const uint32_t fw = rw[kTickWords - 1];   // pixel: quality | flags << 8 | pred_x << 16 | pred_y << 24
    BankFieldTick r;
    r.quality = (int32_t)rw[0]; r.dt_us = (int32_t)rw[1]; r.frame = rw[7];
    r.pred_x = (int8_t)(fw >> 16); r.pred_y = (int8_t)(fw >> 24);
    const bool pair = bank_field_pair(r);   // (uniform in the group)

    aof_field f = field_publish(0u, 0u, 0u, nullptr, 0u, false);   // all zero: the fit of a stream without a pair
    if (pair) {
        const int nb = a.g.nb;
        f = field_fit<GROUP, KEEP>(a.g, FastDiv{a.div_nx_mul, a.div_nx_shift}, a.blocks + (size_t)s * nb,
                                   a.subdirs ? a.subdirs + (size_t)s * nb : nullptr, r.pred_x, r.pred_y);
    }
    if (tid == 0) {
        if (a.fields) a.fields[s] = f;
        if (bank_field_no_frame(r.quality)) {
            a.out[s] = bank_field_record_zero(r.quality);
        } else {
            float focal_x = a.focal_x, focal_y = a.focal_y;
            if (a.streams) { focal_x = a.streams[s].focal_x; focal_y = a.streams[s].focal_y; }
            aof_bank_field_state st = a.state[s];
            a.out[s] = bank_field_step(r, pair, f, focal_x, focal_y, st);
            a.state[s] = st;
        }
    }
    // the records out to where a host reads them, before the launch counts as done
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
}

}  // namespace

int launch_bank_field(const BankFieldArgs &args, void *stream)
{
    if (args.n_streams < 1 || !args.blocks || !args.records || !args.state || !args.out || args.g.nb < 1 || args.g.nx < 1)
        return (int)hipErrorInvalidValue;   // one workgroup (or wave) per stream
    BankFieldArgs a = args;
    const FastDiv d = fastdiv_make((uint32_t)a.g.nx);
    a.div_nx_mul = d.mul;
    a.div_nx_shift = d.shift;
    if (a.g.nb <= 256)   // sparse grids: one wave per stream
        hipLaunchKernelGGL((k_bank_field<64, 1>), dim3(((uint32_t)a.n_streams + 3u) / 4u), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    else
        hipLaunchKernelGGL((k_bank_field<kThreads, 5>), dim3((uint32_t)a.n_streams), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

}  // namespace aof
