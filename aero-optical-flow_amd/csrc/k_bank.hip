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
// The tail is the facade's limitRate() / integrate() (facade/src/optical_flow.cpp) and mainloop.cpp:322-373 on ONE
// stream's state: every float operation is the host's, in the host's order.
#include "aof_flow_small.hpp"
#include "aof_mavlink.hpp"
#include "aof_math.h"

namespace aof {

namespace {

__device__ __forceinline__ void bank_idle(const BankArgs &a, uint32_t s)
{
    aof_tick_record rec = {};
    rec.quality = AOF_TICK_IDLE;
    a.records[s] = rec;
    if (a.mavlink_len) a.mavlink_len[s] = 0;
}

// One lane: stream s has been given a frame; `f` is the pixel record of (stored frame, new frame), `first` says
// that there was no stored frame.  payload: kMavlinkPayloadBytes of LDS for the packer.
__device__ __forceinline__ void bank_tail(const BankArgs &a, uint32_t s, aof_flow f, bool first, uint8_t *payload)
{
    BankState st = a.state[s];
    const uint64_t t64 = a.time_us[s];
    const uint32_t t = (uint32_t)t64;   // calcFlow sees 32 bits (mainloop.cpp:305-315)
    st.frames++;
    if (a.gyro) {                       // integrated since the last message (mainloop.cpp:383-405)
        const aof_gyro g = a.gyro[s];
        st.gyro_x += g.integ_x; st.gyro_y += g.integ_y; st.gyro_z += g.integ_z;
    }
    int quality = 0, dt_us = 0;
    float px = 0.0f, py = 0.0f;
    if (first) {
        // calcFlow returns 0 with its outputs untouched (integrate(): nothing to compare the frame with), and the
        // caller sends what its zero-initialised locals hold (mainloop.cpp:280-281,322-373)
        st.has_prev = 1;
        f = aof_flow{};
    } else {
        quality = f.quality; px = f.flow_x; py = f.flow_y;
        if (a.output_rate <= 0) {       // limitRate: no limit, the frame's own flow and quality
            dt_us = (int)(t - st.time_last_pub);
            st.time_last_pub = t;
        } else {
            if (quality > 0) {
                st.sum_flow_x += px;
                st.sum_flow_y += py;
                st.sum_flow_quality += quality;
                st.valid_frame_count++;
            }
            if ((float)(t - st.time_last_pub) > a.period_us) {
                quality = 0;
                if (st.valid_frame_count > 0) quality = (int)floorf((float)st.sum_flow_quality / (float)st.valid_frame_count);
                px = st.sum_flow_x; py = st.sum_flow_y;
                st.sum_flow_x = 0.0f; st.sum_flow_y = 0.0f; st.sum_flow_quality = 0; st.valid_frame_count = 0;
                dt_us = (int)(t - st.time_last_pub);
                st.time_last_pub = t;
            } else {
                quality = AOF_TICK_HELD;   // still integrating: the caller skips this frame (mainloop.cpp:327-331)
            }
        }
    }
    aof_tick_record rec = {};
    rec.quality = quality;
    rec.frame = st.frames;
    rec.pixel = f;
    uint8_t len = 0;
    if (quality >= 0) {
        float ang_x = 0.0f, ang_y = 0.0f;
        if (!first) { ang_x = aof_atan2f(px, a.focal_x); ang_y = aof_atan2f(py, a.focal_y); }
        rec.dt_us = dt_us;
        rec.flow_x = ang_x; rec.flow_y = ang_y;
        rec.gyro_x = (float)st.gyro_x; rec.gyro_y = (float)st.gyro_y; rec.gyro_z = (float)st.gyro_z;
        if (a.mavlink && a.offset_timestamp_usec != 0)   // (0: vehicle time not known, nothing is sent; mainloop.cpp:353-357)
            len = (uint8_t)pack_optical_flow_rad(a.mavlink + (size_t)s * AOF_SEQ_FRAME_BYTES, payload, a.offset_timestamp_usec + t64, dt_us,
                                                 ang_x, ang_y, st.gyro_x, st.gyro_y, st.gyro_z, quality,
                                                 (uint8_t)(a.first_seq + st.messages), a.system_id, a.component_id);
        st.messages++;
        st.gyro_x = 0.0; st.gyro_y = 0.0; st.gyro_z = 0.0;   // taken with the message (mainloop.cpp:333-334)
    }
    a.records[s] = rec;
    if (a.mavlink_len) a.mavlink_len[s] = len;
    a.state[s] = st;
}

// `bytes` from src to dst by the whole workgroup: 16 bytes per lane where both are aligned (dst, a bank slot, always is).
__device__ __forceinline__ void copy_frame(uint8_t *dst, const uint8_t *src, int64_t bytes)
{
    const int tid = threadIdx.x;
    int64_t done = 0;
    if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        const int64_t chunks = bytes / 16;
        for (int64_t c = tid; c < chunks; c += kThreads)
            reinterpret_cast<uint4 *>(dst)[c] = reinterpret_cast<const uint4 *>(src)[c];
        done = chunks * 16;
    }
    for (int64_t b = done + tid; b < bytes; b += kThreads) dst[b] = src[b];
}

// Is stream s's frame its first?  Asked through LDS: lane 0 rewrites the state record later, and the waves of a
// workgroup do not run in step.
__device__ __forceinline__ bool bank_first(const BankArgs &a, uint32_t s)
{
    __shared__ uint32_t s_first;
    if (threadIdx.x == 0) s_first = a.state[s].has_prev == 0 ? 1u : 0u;
    __syncthreads();
    return s_first != 0;
}

template <bool SUBPIXEL>
__global__ __launch_bounds__(kThreads) void k_bank_tick(SmallArgs sm, BankArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_mem[];
    __shared__ aof_flow s_record;
    __shared__ uint8_t s_payload[kMavlinkPayloadBytes];
    const uint32_t s = blockIdx.x;   // (the launcher: one workgroup per stream)
    if (a.active && a.active[s] == 0) {   // (uniform)
        if (threadIdx.x == 0) bank_idle(a, s);
        return;
    }
    const uint8_t *src = a.frames + (int64_t)s * a.frame_stride;
    uint8_t *slot = a.bank_frames + (int64_t)s * a.frame_stride;
    if (bank_first(a, s)) {               // (uniform)
        copy_frame(slot, src, a.frame_bytes);
        if (threadIdx.x == 0) bank_tail(a, s, aof_flow{}, true, s_payload);
        return;
    }
    flow_small_pair<SUBPIXEL>(sm, s, slot, src, 1, 3u, &s_record);
    __syncthreads();
    if (threadIdx.x == 0) bank_tail(a, s, s_record, false, s_payload);
    // the new frame sits in LDS buffer 1 (flow_small_pair's layout: frame, kPad bytes, frame)
    const uint8_t *lds_new = s_mem + a.frame_bytes + kPad;
    for (int c = threadIdx.x; c < (int)(a.frame_bytes / 16); c += kThreads)
        reinterpret_cast<uint4 *>(slot)[c] = reinterpret_cast<const uint4 *>(lds_new)[c];
}

__global__ __launch_bounds__(kThreads) void k_bank_commit(BankArgs a)
{
    __shared__ uint8_t s_payload[kMavlinkPayloadBytes];
    const uint32_t s = blockIdx.x;
    if (a.active && a.active[s] == 0) {   // (uniform)
        if (threadIdx.x == 0) bank_idle(a, s);
        return;
    }
    const bool first = bank_first(a, s);
    if (threadIdx.x == 0) bank_tail(a, s, a.flows[s], first, s_payload);
    copy_frame(a.bank_frames + (int64_t)s * a.frame_stride, a.frames + (int64_t)s * a.frame_stride, a.frame_bytes);
}

__global__ __launch_bounds__(kThreads) void k_bank_reset(BankState *state, const uint8_t *mask, int32_t n)
{
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= n || (mask && mask[s] == 0)) return;
    state[s] = BankState{};
}

}  // namespace

int launch_bank_tick(const SmallArgs &sm, const BankArgs &a, void *stream)
{
    if (a.n_streams < 1 || sm.l0.n_pairs != a.n_streams || !flow_small_supported(sm)) return (int)hipErrorInvalidValue;
    if (a.frame_bytes != (int64_t)sm.l0.w * sm.l0.h || a.frame_bytes % 16) return (int)hipErrorInvalidValue;
    void (*fn)(SmallArgs, BankArgs) = sm.l0.subpixel ? k_bank_tick<true> : k_bank_tick<false>;
    const size_t lds = small_lds_bytes(sm);
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fn),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(fn, dim3((uint32_t)a.n_streams), dim3(kThreads), lds, static_cast<hipStream_t>(stream), sm, a);
    return (int)hipGetLastError();
}

int launch_bank_commit(const BankArgs &a, void *stream)
{
    if (a.n_streams < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bank_commit, dim3((uint32_t)a.n_streams), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
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
