// KS -- a whole small pair, one or two levels, in ONE workgroup, ONE launch and out of LDS
// (DESIGN.md "Kernels": KS).
//
// The call shape of the reference -- one small frame per calcFlow(), mainloop.cpp:322 -- is bound by
// launches and memory round trips, not by arithmetic.  As separate kernels two levels are a memset,
// K1, the level-1 search and the level-0 search (four graph nodes, 45 us per call), and each search
// is a few dozen lanes walking all 81 candidates of their block alone, every row from memory.  Here
// one workgroup does the lot for a pair whose frames fit LDS and whose grids have at most 256 blocks
// (the published sparse grid: 25):
//   A  both level-0 frames: global (or pinned host) memory -> LDS, every load issued before the
//      first use -- one round trip --, pixel sums on the way;
//   B  two levels: 2x2 box pyramid LDS -> LDS, level-1 sums;
//   C  per level: one lane per (block, dy) -- nine lanes share a block, 25 blocks fill the workgroup --
//      reads tile and window rows from LDS at any byte offset (aligned dwords + v_alignbyte), sums its
//      nine dx candidates with v_qsad_pk_u16_u8 / v_sad_hi_u8 and joins its block through one LDS
//      atomicMin on the packed key (sad << 16 | idx): first minimum in scan order;
//   D  one lane per block: record, half-pixel refinement from LDS, votes; wave 0 finalises the
//      level's flow record; the level-1 predictor reaches level 0 through LDS.
// Nothing but the block records, the flow records and the sums leaves the chip (the level-1 frames of
// the workspace stay untouched, as under the fused coarse kernel).  Results are those of the separate
// kernels bit for bit.
// Every kernel of this class -- the three forms here, the stream bank's tick and burst -- goes out through the one
// launcher launch_small_class (aof_flow_small.hpp): the support check, the dynamic-LDS attribute, the launch.
#include "aof_engine_args.hpp"
#include "aof_flow_small.hpp"
#include "aof_resident.hpp"

namespace aof {

namespace {

template <bool SUBPIXEL>
__global__ __launch_bounds__(kThreads) void k_flow_small(SmallArgs a)   // (latency path: occupancy does not matter)
{
    const uint32_t pair = blockIdx.x;
    flow_small_pair<SUBPIXEL>(a, pair, a.l0.prev + (int64_t)pair * a.l0.pair_stride, a.l0.cur + (int64_t)pair * a.l0.pair_stride,
                              1, 3u);
}

// The per-call path (one pair per launch, record in pinned host memory): the record leaves with ONE 16-byte
// store whose `count` carries the low byte of *tag in its top byte (block counts stay below 2^24) -- the
// host, which wrote the tag before the launch, polls the record for it instead of waiting for the stream
// to drain (the runtime's completion path costs more than the kernel).
template <bool SUBPIXEL>
__global__ __launch_bounds__(kThreads) void k_flow_small_tagged(SmallArgs a, aof_flow *host_record, const uint32_t *tag)
{
    __shared__ aof_flow s_record;
    uint32_t t = 0;
    if (threadIdx.x == 0) t = __hip_atomic_load(tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // (in flight beside the frames)
    flow_small_pair<SUBPIXEL>(a, 0, a.l0.prev, a.l0.cur, 1, 3u, &s_record);
    __syncthreads();
    if (threadIdx.x == 0) {
        aof_flow r = s_record;
        r.count = (r.count & 0x00FFFFFFu) | (t << 24);
        *reinterpret_cast<uint4 *>(host_record) = __builtin_bit_cast(uint4, r);
    }
}

// ---- the resident form of the per-call path (aof_set_stream_resident) --------------------------------
// calcFlow() hands over ONE small frame per call (mainloop.cpp:322), and 20 of the 25 us such a call takes
// through a replayed hipGraph are the runtime's launch and completion, not the 4 us kernel.  Here ONE
// workgroup stays on the device between calls: the host writes the frame into its pinned ping-pong slot and
// bumps a request word in pinned memory; lane 0 polls that word, the workgroup computes the pair exactly
// as k_flow_small does (same function) and publishes the 16-byte record in pinned memory with ONE store,
// the request's low byte riding in the top byte of `count`, which the host polls for.  The kernel ALWAYS ends by itself: after `idle_ticks` of the 100 MHz
// real-time counter without a request, after `life_ticks` in total (so that nothing that waits for the
// device to drain -- a hipFree anywhere in the process -- waits longer than that), or when the host sets
// the stop word; the next call starts it again.
template <bool SUBPIXEL>
__global__ __launch_bounds__(kThreads) void k_flow_resident(SmallArgs a, ResidentBox *box, aof_flow *host_record,
                                                            const uint8_t *frame_a, const uint8_t *frame_b, uint32_t served,
                                                            uint32_t launch_no, uint64_t idle_ticks, uint64_t life_ticks, int deaf)
{
    __shared__ uint32_t s_req[3];   // request number (0 = leave), slot of the newest frame, buffers to fetch
    __shared__ aof_flow s_record;   // the call's flow record (the kernel's own copy goes to device memory)
    const uint64_t born = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) __hip_atomic_store(&box->started, launch_no, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    uint64_t idle_since = born;
    uint32_t held[2] = {0u, 0u};    // (thread 0) tag of the request at which LDS buffer b received pinned frame b, 0 = never
    for (;;) {
        if (threadIdx.x == 0) {
            uint32_t req = 0, slot = 0, load = 3u;
            unsigned long long word = 0;
            for (;;) {
                word = __hip_atomic_load(&box->word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // one PCIe read
                // (deaf: fault injection of the tests -- the stop bit is ignored, the kernel neither serves nor leaves
                //  when asked and goes on its idle / lifetime deadline only: aof_debug_resident_fault)
                const bool stop = (word & kResidentStopBit) != 0;
                if (!stop && (uint32_t)word != served) { req = (uint32_t)word; break; }
                const uint64_t now = __builtin_amdgcn_s_memrealtime();
                if ((stop && !deaf) || now - idle_since > idle_ticks || now - born > life_ticks) break;
                __builtin_amdgcn_s_sleep(8);
            }
            if (req) {
                slot = (uint32_t)(word >> 32) & 1u;
                // the older frame of this pair sits in pinned frame 1 - slot; the host says at which request
                // it was posted (0: not through a request) -- if that is when this workgroup fetched its
                // LDS buffer 1 - slot, the copy is still good and only the new frame crosses PCIe
                const uint32_t prev_tag = (uint32_t)(word >> 33) & 0x7FFFFFFFu;   // (low 30 bits of the request) + 1
                load = (prev_tag != 0u && held[1u - slot] == prev_tag) ? (1u << slot) : 3u;
                held[slot] = (req & 0x3FFFFFFFu) + 1u;
                if (load == 3u) held[1u - slot] = prev_tag;
            }
            s_req[0] = req;
            s_req[1] = slot;
            s_req[2] = load;
        }
        __syncthreads();
        const uint32_t req = s_req[0], slot = s_req[1], load = s_req[2];
        if (req == 0) break;   // (uniform)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");   // the host's frame bytes: nothing stale out of L1 / L2
        flow_small_pair<SUBPIXEL>(a, 0, frame_a, frame_b, (int)slot, load, &s_record);
        __syncthreads();
        if (threadIdx.x == 0) {
            // ONE 16-byte store publishes the record: the low byte of the request number rides in the top
            // byte of `count` (block counts stay below 2^24), the host polls for it and masks it out -- the host
            // does not wait for a second PCIe write behind a fence.  `done` follows for the next kernel instance
            // (read only after this one has left).
            aof_flow r = s_record;
            r.count = (r.count & 0x00FFFFFFu) | (req << 24);
            *reinterpret_cast<uint4 *>(host_record) = __builtin_bit_cast(uint4, r);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // pushes the record out (the host is polling for it already)
            __hip_atomic_store(&box->done, req, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        served = req;
        idle_since = __builtin_amdgcn_s_memrealtime();
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(&box->exited, served, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&box->running, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace

int launch_flow_resident(const SmallArgs &a, ResidentBox *box, aof_flow *host_record, const uint8_t *frame_a,
                         const uint8_t *frame_b, uint32_t served, uint32_t launch_no, uint64_t idle_ticks,
                         uint64_t life_ticks, bool deaf, void *stream)
{
    if (a.l0.n_pairs != 1) return (int)hipErrorInvalidValue;
    return launch_small_class(a.l0.subpixel ? k_flow_resident<true> : k_flow_resident<false>, 1, a, stream, a, box, host_record,
                              frame_a, frame_b, served, launch_no, idle_ticks, life_ticks, deaf ? 1 : 0);
}

int launch_flow_small_tagged(const SmallArgs &a, aof_flow *host_record, const uint32_t *tag, void *stream)
{
    if (a.l0.n_pairs != 1 || !host_record || !tag) return (int)hipErrorInvalidValue;
    return launch_small_class(a.l0.subpixel ? k_flow_small_tagged<true> : k_flow_small_tagged<false>, 1, a, stream, a, host_record, tag);
}

int launch_flow_small(const SmallArgs &a, void *stream)
{
    if (a.l0.n_pairs == 0) return 0;
    return launch_small_class(a.l0.subpixel ? k_flow_small<true> : k_flow_small<false>, (uint32_t)a.l0.n_pairs, a, stream, a);
}

}  // namespace aof
