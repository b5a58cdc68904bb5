// The motion-field fit of a batch (aof_field_batch_device; include/aof.h "the motion FIELD of a batch"): per pair, the
// least-squares similarity over the block records K2 wrote -- zoom, rotation and the flow at the frame centre.  A
// translation unit of its own: nothing another kernel file compiles to moves.  The rule is aof_field_step.hpp, the text
// aof_field_host runs; the data movement around it -- the record loads with their peeled head and tail, the sweeps, the
// solve and the gated second pass -- is field_fit (aof_field_fit.hpp), which the stream bank's kernel (k_bank_field.hip)
// compiles too.  This file is the two forms of it over a batch, shaped like k_reduce's:
//   * k_field<64, 1>: a wave per pair, four pairs per workgroup, for grids of at most 256 blocks (one quad of records per
//     lane); k_field<256, 5>: a workgroup per pair above that, looping over the pair's quads, whatever their number.
// Inputs are only read; a pair's 64-byte record, stored by lane 0 of its group, is the only store.
#include "aof_fastdiv.hpp"
#include "aof_field_fit.hpp"

namespace aof {

namespace {

constexpr int kThreads = kFieldThreads;

template <int GROUP, int KEEP>
__global__ __launch_bounds__(kThreads) void k_field(FieldArgs a)
{
    constexpr int kGroups = kThreads / GROUP;
    const int grp = (int)threadIdx.x / GROUP, tid = (int)threadIdx.x % GROUP;
    const int64_t pair = (int64_t)blockIdx.x * kGroups + grp;
    if (GROUP < kThreads && pair >= a.n_pairs) return;   // whole waves only: no barrier is skipped
    const int nb = a.g.nb;
    const uint32_t fw = a.flows[4 * pair + 3];
    const aof_field f = field_fit<GROUP, KEEP>(a.g, FastDiv{a.div_nx_mul, a.div_nx_shift}, a.blocks + pair * nb,
                                               a.subdirs ? a.subdirs + pair * nb : nullptr, (int8_t)(fw >> 16), (int8_t)(fw >> 24));
    if (tid == 0) a.fields[pair] = f;
}

}  // namespace

int launch_field(const FieldArgs &args, void *stream)
{
    if (args.n_pairs == 0) return 0;
    if (args.n_pairs < 0 || args.n_pairs > 0x7FFFFFFF || !args.blocks || !args.flows || !args.fields || args.g.nb < 1 || args.g.nx < 1)
        return (int)hipErrorInvalidValue;   // one workgroup (or wave) per pair
    FieldArgs a = args;
    const FastDiv d = fastdiv_make((uint32_t)a.g.nx);
    a.div_nx_mul = d.mul;
    a.div_nx_shift = d.shift;
    if (a.g.nb <= 256)   // sparse grids: one wave per pair
        hipLaunchKernelGGL((k_field<64, 1>), dim3((uint32_t)((a.n_pairs + 3) / 4)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    else
        hipLaunchKernelGGL((k_field<kThreads, 5>), dim3((uint32_t)a.n_pairs), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

}  // namespace aof
