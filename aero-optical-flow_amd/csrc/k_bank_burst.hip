// The stream bank's burst on the device (aof_bank_push_burst_device / aof_bank_push_camera_burst_device,
// include/aof.h): K frame rounds per stream from ONE launch, byte for byte what K ticks of k_bank_tick leave.
//   k_bank_burst   one workgroup per stream walks the stream's rounds in order.  The state record is read once, lives
//                  in LDS across the rounds (in registers it would be live through every search: 16 VGPRs of every
//                  lane) and is stored once; the stored frame is read once (pass A of the first
//                  pair, and only if the stream has one); round k's frame goes into the LDS buffer that does not hold
//                  round k - 1's (flow_small_pair's cur_buf / load), so the older frame's bytes, level-1 image and
//                  pixel sums are never made twice; the slot is written once, behind the last round, out of LDS.
//                  (K + 2) W H bytes per stream instead of the 3 K W H of K ticks.  A first frame inside the burst is
//                  fetched into LDS buffer 0 like any other frame (flow_small_pair's fetch-only form) and round 1
//                  pairs with it there.  A stream without a frame writes its K idle records and leaves before any
//                  frame load.
// Every record comes from bank_tail_step, every idle record from bank_idle, the gate, the histogram and the MSV from
// aof_bank_stream.hpp: the functions k_bank_tick runs.
#include "aof_bank_args.hpp"
#include "aof_bank_stream.hpp"
#include "aof_engine_args.hpp"

namespace aof {

namespace {

// (four waves per SIMD: the loop over the rounds costs registers the tick does not need, and 1 024 streams are four
// workgroups per compute unit -- one VGPR over 128 would leave the fourth one waiting for a whole burst)
// Sen: nothing, or one BankSensors (aof_set_bank_sensors; the camera form only): the body of k_bank_burst and of
// k_bank_burst_sensors below.
template <bool SUBPIXEL, bool CAMERA, typename... Sen>
__device__ __forceinline__ void bank_burst_rounds(SmallArgs sm, BankArgs a, BankBurst b, Sen... sen)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_mem[];
    __shared__ aof_flow s_record;
    __shared__ uint8_t s_payload[kMavlinkPayloadBytes];
    __shared__ uint32_t s_hist[AOF_EXPOSURE_BINS];
    __shared__ BankState s_state;    // the stream's state record, on chip across the rounds; only the tail lane touches it
    __shared__ uint32_t s_gate;      // bit 0: the stream has no stored frame (round 0 only), bit 1: the round's frame is due
    const int tid = threadIdx.x;
    const uint32_t s = blockIdx.x;   // (the launcher: one workgroup per stream)
    const size_t S = (size_t)a.n_streams;
    const int K = b.n_rounds;        // (the launcher: 1..AOF_BANK_BURST_MAX)
    int n = K;                       // the stream has frames in rounds 0..n-1 (uniform)
    if (b.count) n = min((int)b.count[s], K);
    if constexpr (sizeof...(Sen) > 0) {
        // a round's frame lies round_stride bytes behind the previous one's, so the rounds whose record forbids the read
        // are the stream's last ones -- they get AOF_TICK_BAD_SENSOR and are otherwise idle rounds
        const int given = n;
        n = 0;
        while (n < given && bank_source<true>(a, s, (uint64_t)n * (uint64_t)b.round_stride, sen...).ok) n++;
        if (tid < K - n) bank_idle<true>(a, (size_t)(n + tid) * S + s, n + tid < given ? AOF_TICK_BAD_SENSOR : AOF_TICK_IDLE);
    } else {
        if (tid < K - n) bank_idle<CAMERA>(a, (size_t)(n + tid) * S + s);
    }
    if (n == 0) return;

    if (tid == 0) {
        const BankState st = a.state[s];
        s_state = st;
        s_gate = (st.has_prev == 0 ? 1u : 0u) | (CAMERA && exposure_due(a, st, a.time_us[s]) ? 2u : 0u);
    }
    __syncthreads();                 // (neither the state nor, behind pass A of the first pair, the slot is read again)
    uint32_t gate = s_gate;
    uint8_t *slot = a.bank_frames + (int64_t)s * a.frame_stride;
    const BankSource from = bank_source<CAMERA>(a, s, 0, sen...);
    const uint8_t *base = from.src;
    uint8_t *const f0[2] = {s_mem, s_mem + a.frame_bytes + kPad};   // flow_small_pair's layout: frame, kPad bytes, frame
    constexpr uint32_t kWindow = CAMERA ? 1u : 0u;
    int newest = -1;                 // the LDS buffer that holds the newest frame; -1: none yet, the slot does
    for (int k = 0; k < n; k++) {
        const size_t o = (size_t)k * S + s;
        if (k > 0) {
            // behind the tail lane's reads of the previous round's flow record and histogram, in front of this round's
            // writes to them; the lane's own state says whether this round's frame is due
            if constexpr (CAMERA) {
                if (tid == 0) s_gate = exposure_due(a, s_state, a.time_us[o]) ? 2u : 0u;
            }
            __syncthreads();
            if constexpr (CAMERA) gate = s_gate;
        }
        // the round's copy of the plan, opaque to the compiler: what a lane derives from the frame's and the grid's
        // geometry is the same in every round, and hoisted out of this loop it stays live through all of it
        SmallArgs r = sm;
        asm volatile("" : "+s"(r.l0.w), "+s"(r.l0.grid.nx), "+s"(r.l1.w), "+s"(r.l1.grid.nx));
        // a stream's first frame (round 0 only) is fetched like any other -- level-1 image and sums included -- into
        // buffer 0, and no pair is searched; the first pair of a stream with a stored frame fetches both buffers
        const bool first = (gate & 1u) != 0;
        const int cur = newest < 0 ? (first ? 0 : 1) : 1 - newest;
        const uint32_t load = first ? 1u : newest < 0 ? 3u : 1u << cur;
        const uint8_t *src = base + (int64_t)k * b.round_stride;
        flow_small_pair<SUBPIXEL, CAMERA, (sizeof...(Sen) > 0)>(r, s, cur ? slot : src, cur ? src : slot, cur, load, &s_record, from.crop,
                                          kWindow << cur, !first);
        // (run_level's last barrier is behind every read of the frames; s_hist is nobody else's)
        if constexpr (CAMERA) {
            if (gate & 2u) bank_histogram(a.cam, f0[cur], s_hist);
        }
        __syncthreads();
        if (tid == 0) {
            BankState st = s_state;
            bank_tail_step<CAMERA>(a, o, s, st, first ? aof_flow{} : s_record, first, s_payload, s_hist);
            s_state = st;
        }
        newest = cur;
        gate &= ~1u;
    }
    if (tid == 0) a.state[s] = s_state;
    store_slot(a, slot, f0[newest]);
}

template <bool SUBPIXEL, bool CAMERA>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4))) void k_bank_burst(SmallArgs sm, BankArgs a, BankBurst b)
{
    bank_burst_rounds<SUBPIXEL, CAMERA>(sm, a, b);
}

// The camera burst with a sensor array bound: the same rounds, every round's source from the stream's record.  A kernel
// of its own name and argument list: with nothing bound the four instantiations above are launched as they always were.
template <bool SUBPIXEL>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4))) void k_bank_burst_sensors(SmallArgs sm, BankArgs a, BankBurst b,
                                                                                                       BankSensors sen)
{
    bank_burst_rounds<SUBPIXEL, true>(sm, a, b, sen);
}

}  // namespace

int launch_bank_burst(const SmallArgs &sm, const BankArgs &a, const BankBurst &b, void *stream, const BankSensors &sen)
{
    if (!bank_plan_fits(sm, a)) return (int)hipErrorInvalidValue;
    if (b.n_rounds < 1 || b.n_rounds > AOF_BANK_BURST_MAX) return (int)hipErrorInvalidValue;
    const bool camera = a.cam.camera != nullptr;
    if (sen.recs) {
        if (!camera) return (int)hipErrorInvalidValue;
        return launch_small_class(sm.l0.subpixel ? k_bank_burst_sensors<true> : k_bank_burst_sensors<false>, (uint32_t)a.n_streams, sm,
                                  stream, sm, a, b, sen);
    }
    return launch_small_class(camera ? (sm.l0.subpixel ? k_bank_burst<true, true> : k_bank_burst<false, true>)
                                     : (sm.l0.subpixel ? k_bank_burst<true, false> : k_bank_burst<false, false>),
                              (uint32_t)a.n_streams, sm, stream, sm, a, b);
}

}  // namespace aof
