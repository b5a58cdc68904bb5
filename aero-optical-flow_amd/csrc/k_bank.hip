// The stream bank on the device (aof_bank_push_device / aof_bank_reset_device, include/aof.h): S independent live
// streams, each with the state one facade object keeps on the host, served per tick.
//   k_bank_tick    one workgroup per stream, ONE launch per tick: the stored frame and the new frame go to LDS with
//                  all loads in flight, the pair runs through flow_small_pair -- the function k_flow_small runs, so the
//                  pixel record cannot differ --, one lane runs the stream's tail (rate limiter, angles, gyro sums,
//                  OPTICAL_FLOW_RAD frame) and the workgroup stores the new frame over the old one out of LDS.  The
//                  slot is read in pass A only, which ends in a barrier; the write-back comes behind the whole pair.
//                  A stream's first frame and idle streams branch out workgroup-uniformly before any frame load.
//   k_bank_commit  the composed path's second launch, behind aof_flow_batch_device's plan on (bank frames, tick
//                  frames): the same tail per stream and the copy of the active streams' frames into the bank.
//   k_bank_reset   masked streams back to "no previous frame".
// CAMERA forms (aof_bank_push_camera_device): the tick kernel fetches the new frame as the centre crop of the stream's
// sensor frame (flow_small_pair's pitched source: 3 W H bytes per stream and tick instead of the 5 W H of an ingest
// launch in front of the plain tick); on a tick that passes the stream's exposure gate the workgroup builds the masked
// 10-bin histogram from the new frame's LDS copy; the tail lane moves the gate, writes the exposure record (the MSV in
// aof_exposure_msv's float operations and order) and the de-rotated pair (derotate_flow, the function k_derotate
// runs).  The commit kernel does the same from the staging region's frames and raw histograms (k_ingest).
// With a sensor array bound (aof_set_bank_sensors) the launchers pick the instantiations that take a BankSensors argument:
// the crop's place, pitch and origin are then the stream's own (bank_source), and a stream whose record forbids the read
// leaves like an idle one, with quality AOF_TICK_BAD_SENSOR.  With nothing bound the kernels without it are launched.
// What a stream does with a frame (tail, gate, histogram, copies) is aof_bank_stream.hpp, shared with k_bank_burst.hip,
// as is the launchers' check of the plan against the bank (bank_plan_fits); the tick goes out through the one launcher
// of the one-workgroup class (launch_small_class, aof_flow_small.hpp).  On the host all four push forms are one path
// (bank_push, aof_bank.cpp).
#include "aof_bank_args.hpp"
#include "aof_bank_stream.hpp"
#include "aof_engine_args.hpp"

namespace aof {

namespace {

// Sen: nothing, or one BankSensors (aof_set_bank_sensors; camera forms only).  With nothing bound the launched kernel
// is the instantiation without the argument: no record, no branch on one, the arguments of a build that never had them.
template <bool SUBPIXEL, bool CAMERA, typename... Sen>
__global__ __launch_bounds__(kThreads) void k_bank_tick(SmallArgs sm, BankArgs a, Sen... sen)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_mem[];
    __shared__ aof_flow s_record;
    __shared__ uint8_t s_payload[kMavlinkPayloadBytes];
    constexpr bool kSensors = sizeof...(Sen) > 0;
    const uint32_t s = blockIdx.x;   // (the launcher: one workgroup per stream)
    if (a.active && a.active[s] == 0) {   // (uniform)
        if (threadIdx.x == 0) bank_idle<CAMERA>(a, s);
        return;
    }
    const BankSource from = bank_source<CAMERA>(a, s, 0, sen...);   // (uniform: with a sensor array bound, the stream's record)
    const uint8_t *src = from.src;
    uint8_t *slot = a.bank_frames + (int64_t)s * a.frame_stride;
    if constexpr (CAMERA) {
        __shared__ uint32_t s_hist[AOF_EXPOSURE_BINS];
        uint8_t *lds_new = s_mem + a.frame_bytes + kPad;
        const uint32_t gate = bank_gate(a, s, from.ok);   // (uniform)
        if constexpr (kSensors) {
            if (gate & kGateBadSensor) {         // as early as the idle exit, and like it in front of any frame load
                if (threadIdx.x == 0) bank_idle<true>(a, s, AOF_TICK_BAD_SENSOR);
                return;
            }
        }
        if (gate & kGateFirst) {
            crop_first_frame(a.cam, src, from.crop, lds_new, slot);
            if (gate & kGateDue) bank_histogram(a.cam, lds_new, s_hist);
            if (threadIdx.x == 0) bank_tail<true>(a, s, aof_flow{}, true, s_payload, s_hist);
            return;
        }
        flow_small_pair<SUBPIXEL, true, kSensors>(sm, s, slot, src, 1, 3u, &s_record, from.crop);
        // (run_level's last barrier is behind every read of the frames; s_hist is nobody else's)
        if (gate & kGateDue) bank_histogram(a.cam, lds_new, s_hist);
        __syncthreads();
        if (threadIdx.x == 0) bank_tail<true>(a, s, s_record, false, s_payload, s_hist);
    } else {
        if (bank_first(a, s)) {               // (uniform)
            copy_frame(slot, src, a.frame_bytes);
            if (threadIdx.x == 0) bank_tail<false>(a, s, aof_flow{}, true, s_payload);
            return;
        }
        flow_small_pair<SUBPIXEL>(sm, s, slot, src, 1, 3u, &s_record);
        __syncthreads();
        if (threadIdx.x == 0) bank_tail<false>(a, s, s_record, false, s_payload);
    }
    // the new frame sits in LDS buffer 1 (flow_small_pair's layout: frame, kPad bytes, frame)
    store_slot(a, slot, s_mem + a.frame_bytes + kPad);
}

// count (a burst's composed path, round `round` of it; a's per-round pointers are the round's): the stream is active
// iff round < count[s]; NULL: a.active decides, as in a tick.  Sen: as in k_bank_tick.
template <bool CAMERA, typename... Sen>
__global__ __launch_bounds__(kThreads) void k_bank_commit(BankArgs a, const uint8_t *count, int32_t round, Sen... sen)
{
    __shared__ uint8_t s_payload[kMavlinkPayloadBytes];
    const uint32_t s = blockIdx.x;
    if (count ? round >= (int32_t)count[s] : (a.active && a.active[s] == 0)) {   // (uniform)
        if (threadIdx.x == 0) bank_idle<CAMERA>(a, s);
        return;
    }
    const bool first = bank_first(a, s);
    if constexpr (sizeof...(Sen) > 0) {
        // the round's sensor record, judged by the function the ingest kernel judged it with: a stream whose frame was
        // not cropped gets its record and nothing else (no tail, no copy of whatever the staging region holds)
        if (!bank_source<true>(a, s, 0, sen...).ok) {       // (uniform)
            if (threadIdx.x == 0) bank_idle<true>(a, s, AOF_TICK_BAD_SENSOR);
            return;
        }
    }
    if (threadIdx.x == 0)
        bank_tail<CAMERA>(a, s, a.flows[s], first, s_payload, CAMERA ? a.cam.hist + (size_t)s * AOF_EXPOSURE_BINS : nullptr);
    copy_frame(a.bank_frames + (int64_t)s * a.frame_stride, a.frames + (int64_t)s * a.frame_stride, a.frame_bytes);
}

__global__ __launch_bounds__(kThreads) void k_bank_reset(BankState *state, const uint8_t *mask, int32_t n)
{
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= n || (mask && mask[s] == 0)) return;
    state[s] = BankState{};
}

}  // namespace

int launch_bank_tick(const SmallArgs &sm, const BankArgs &a, void *stream, const BankSensors &sen)
{
    if (!bank_plan_fits(sm, a)) return (int)hipErrorInvalidValue;
    const bool camera = a.cam.camera != nullptr;
    if (sen.recs) {   // (the instantiations with the argument)
        if (!camera) return (int)hipErrorInvalidValue;
        return launch_small_class(sm.l0.subpixel ? k_bank_tick<true, true, BankSensors> : k_bank_tick<false, true, BankSensors>,
                                  (uint32_t)a.n_streams, sm, stream, sm, a, sen);
    }
    return launch_small_class(camera ? (sm.l0.subpixel ? k_bank_tick<true, true> : k_bank_tick<false, true>)
                                     : (sm.l0.subpixel ? k_bank_tick<true, false> : k_bank_tick<false, false>),
                              (uint32_t)a.n_streams, sm, stream, sm, a);
}

int launch_bank_commit(const BankArgs &a, void *stream, const uint8_t *count, int32_t round, const BankSensors &sen)
{
    if (a.n_streams < 1) return (int)hipErrorInvalidValue;
    const dim3 grid((uint32_t)a.n_streams), block(kThreads);
    if (sen.recs) {
        if (!a.cam.camera) return (int)hipErrorInvalidValue;
        hipLaunchKernelGGL((k_bank_commit<true, BankSensors>), grid, block, 0, static_cast<hipStream_t>(stream), a, count, round, sen);
        return (int)hipGetLastError();
    }
    void (*fn)(BankArgs, const uint8_t *, int32_t) = a.cam.camera ? k_bank_commit<true> : k_bank_commit<false>;
    hipLaunchKernelGGL(fn, grid, block, 0, static_cast<hipStream_t>(stream), a, count, round);
    return (int)hipGetLastError();
}

int launch_bank_reset(BankState *state, const uint8_t *mask, int32_t n_streams, void *stream)
{
    if (n_streams < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bank_reset, dim3((uint32_t)((n_streams + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), state, mask, n_streams);
    return (int)hipGetLastError();
}

}  // namespace aof
