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
// The tail is the facade's limitRate() / integrate() (facade/src/optical_flow.cpp) and mainloop.cpp:322-373 on ONE
// stream's state: every float operation is the host's, in the host's order.
#include "aof_derotate.hpp"
#include "aof_flow_small.hpp"
#include "aof_mavlink.hpp"
#include "aof_math.h"

namespace aof {

namespace {

template <bool CAMERA>
__device__ __forceinline__ void bank_idle(const BankArgs &a, uint32_t s)
{
    aof_tick_record rec = {};
    rec.quality = AOF_TICK_IDLE;
    a.records[s] = rec;
    if (a.mavlink_len) a.mavlink_len[s] = 0;
    if constexpr (CAMERA) {
        if (a.cam.exposure) a.cam.exposure[s] = aof_exposure_record{};
        if (a.cam.derotated) { a.cam.derotated[2 * s] = 0.0f; a.cam.derotated[2 * s + 1] = 0.0f; }
    }
}

// Is a frame of 64-bit time t due for exposure statistics (mainloop.cpp:199-201: the untruncated time)?
__device__ __forceinline__ bool exposure_due(const BankArgs &a, const BankState &st, uint64_t t)
{
    return a.cam.exposure != nullptr && t >= st.next_exposure_us;
}

// mainloop.cpp:216-220 as aof_exposure_msv computes it: the same float operations in the same order, none fused.
__device__ __forceinline__ float exposure_msv(const uint32_t *hist)
{
#pragma clang fp contract(off)
    float msv = 0.0f;
    for (int i = 0; i < AOF_EXPOSURE_BINS; i++) msv += (i + 1) * (float)hist[i] / 16384.0f;
    return msv;
}

// One lane: stream s has been given a frame; `f` is the pixel record of (stored frame, new frame), `first` says
// that there was no stored frame.  payload: kMavlinkPayloadBytes of LDS for the packer.  CAMERA: `hist` holds the
// frame's ten raw bin totals if the frame is due (exposure_due; LDS or global memory).
template <bool CAMERA>
__device__ __forceinline__ void bank_tail(const BankArgs &a, uint32_t s, aof_flow f, bool first, uint8_t *payload,
                                          const uint32_t *hist = nullptr)
{
    BankState st = a.state[s];
    const uint64_t t64 = a.time_us[s];
    if constexpr (CAMERA) {
        if (a.cam.exposure) {
            aof_exposure_record e = {};
            if (exposure_due(a, st, t64)) {
                for (int i = 0; i < AOF_EXPOSURE_BINS; i++) e.hist[i] = hist[i];
                e.msv = exposure_msv(e.hist);
                e.due = 1;
                st.next_exposure_us = t64 + a.cam.interval_us;
            }
            a.cam.exposure[s] = e;
        }
        if (a.cam.derotated) {   // of the pair's own pixel record, whatever the limiter does with it
            float x = 0.0f, y = 0.0f;
            if (!first) derotate_flow(a.cam.derotate, f, a.gyro ? a.gyro[s] : aof_gyro{}, &x, &y);
            a.cam.derotated[2 * s] = x;
            a.cam.derotated[2 * s + 1] = y;
        }
    }
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

// CAMERA: is stream s's frame its first (bit 0), and is it due for exposure statistics (bit 1)?  One lane reads the
// state and the time, like bank_first.
__device__ __forceinline__ uint32_t bank_gate(const BankArgs &a, uint32_t s)
{
    __shared__ uint32_t s_gate;
    if (threadIdx.x == 0) {
        const BankState st = a.state[s];
        s_gate = (st.has_prev == 0 ? 1u : 0u) | (exposure_due(a, st, a.time_us[s]) ? 2u : 0u);
    }
    __syncthreads();
    return s_gate;
}

// The masked 10-bin histogram (k_ingest's, mainloop.cpp:203-214) of a cropped frame in LDS, by the whole workgroup:
// the mask has at most 128 x 128 pixels, 16 dwords per lane, so a lane's ten counters fit 12-bit fields of two
// 64-bit registers (no table, no scratch); ten wave sums, and one lane per wave adds each to `hist`.  Needs a crop
// width and mask origin on a dword (the one-workgroup class: widths are multiples of 16).  Ends in a barrier.
__device__ __forceinline__ void bank_histogram(const BankCamera &c, const uint8_t *frame, uint32_t *hist)
{
    const int tid = threadIdx.x;
    if (tid < AOF_EXPOSURE_BINS) hist[tid] = 0;
    __syncthreads();
    const int row_dwords = (c.mx1 - c.mx0) / 4, dwords = row_dwords * (c.my1 - c.my0);
    unsigned long long lo = 0, hi = 0;   // bins 0..4, bins 5..9
    for (int i = tid; i < dwords; i += kThreads) {
        const int y = i / row_dwords, x = i - y * row_dwords;
        const uint32_t v = *reinterpret_cast<const uint32_t *>(frame + (c.my0 + y) * c.crop_w + c.mx0 + 4 * x);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t b = (((v >> (8 * k)) & 0xFFu) * 10u) / 255u;   // 10 for v = 255: outside cv::calcHist's range
            if (b < 5) lo += 1ull << (12 * b);
            else if (b < 10) hi += 1ull << (12 * (b - 5));
        }
    }
#pragma unroll
    for (int b = 0; b < AOF_EXPOSURE_BINS; b++) {
        const uint32_t n = wave_sum_u32((uint32_t)((b < 5 ? lo >> (12 * b) : hi >> (12 * (b - 5))) & 0xFFFu));
        if ((tid & 63) == 0 && n) atomicAdd(&hist[b], n);
    }
    __syncthreads();
}

// CAMERA: the crop of a stream's first frame, sensor rows -> LDS -> slot (a first frame is always due: its histogram
// comes from the LDS copy).  Ends in a barrier.
__device__ __forceinline__ void crop_first_frame(const BankCamera &c, const uint8_t *src, uint8_t *lds, uint8_t *slot)
{
    const int row_chunks = c.crop_w / 16, chunks = row_chunks * c.crop_h;
    for (int i = threadIdx.x; i < chunks; i += kThreads) {
        const int y = i / row_chunks, x = i - y * row_chunks;
        uint4 v;
        __builtin_memcpy(&v, src + (int64_t)y * c.pitch + x * 16, 16);
        reinterpret_cast<uint4 *>(lds)[i] = v;
        reinterpret_cast<uint4 *>(slot)[i] = v;
    }
    __syncthreads();
}

template <bool SUBPIXEL, bool CAMERA>
__global__ __launch_bounds__(kThreads) void k_bank_tick(SmallArgs sm, BankArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_mem[];
    __shared__ aof_flow s_record;
    __shared__ uint8_t s_payload[kMavlinkPayloadBytes];
    const uint32_t s = blockIdx.x;   // (the launcher: one workgroup per stream)
    if (a.active && a.active[s] == 0) {   // (uniform)
        if (threadIdx.x == 0) bank_idle<CAMERA>(a, s);
        return;
    }
    const uint8_t *src = CAMERA ? a.cam.camera + (int64_t)s * a.cam.camera_stride + a.cam.origin : a.frames + (int64_t)s * a.frame_stride;
    uint8_t *slot = a.bank_frames + (int64_t)s * a.frame_stride;
    if constexpr (CAMERA) {
        __shared__ uint32_t s_hist[AOF_EXPOSURE_BINS];
        uint8_t *lds_new = s_mem + a.frame_bytes + kPad;
        const uint32_t gate = bank_gate(a, s);   // (uniform)
        if (gate & 1u) {
            crop_first_frame(a.cam, src, lds_new, slot);
            if (gate & 2u) bank_histogram(a.cam, lds_new, s_hist);
            if (threadIdx.x == 0) bank_tail<true>(a, s, aof_flow{}, true, s_payload, s_hist);
            return;
        }
        flow_small_pair<SUBPIXEL, true>(sm, s, slot, src, 1, 3u, &s_record, a.cam.pitch);
        // (run_level's last barrier is behind every read of the frames; s_hist is nobody else's)
        if (gate & 2u) bank_histogram(a.cam, lds_new, s_hist);
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
    const uint8_t *lds_new = s_mem + a.frame_bytes + kPad;
    for (int c = threadIdx.x; c < (int)(a.frame_bytes / 16); c += kThreads)
        reinterpret_cast<uint4 *>(slot)[c] = reinterpret_cast<const uint4 *>(lds_new)[c];
}

template <bool CAMERA>
__global__ __launch_bounds__(kThreads) void k_bank_commit(BankArgs a)
{
    __shared__ uint8_t s_payload[kMavlinkPayloadBytes];
    const uint32_t s = blockIdx.x;
    if (a.active && a.active[s] == 0) {   // (uniform)
        if (threadIdx.x == 0) bank_idle<CAMERA>(a, s);
        return;
    }
    const bool first = bank_first(a, s);
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

int launch_bank_tick(const SmallArgs &sm, const BankArgs &a, void *stream)
{
    if (a.n_streams < 1 || sm.l0.n_pairs != a.n_streams || !flow_small_supported(sm)) return (int)hipErrorInvalidValue;
    if (a.frame_bytes != (int64_t)sm.l0.w * sm.l0.h || a.frame_bytes % 16) return (int)hipErrorInvalidValue;
    const bool camera = a.cam.camera != nullptr;
    if (camera && (a.cam.crop_w != sm.l0.w || a.cam.crop_h != sm.l0.h)) return (int)hipErrorInvalidValue;
    void (*fn)(SmallArgs, BankArgs) = camera ? (sm.l0.subpixel ? k_bank_tick<true, true> : k_bank_tick<false, true>)
                                             : (sm.l0.subpixel ? k_bank_tick<true, false> : k_bank_tick<false, false>);
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
    void (*fn)(BankArgs) = a.cam.camera ? k_bank_commit<true> : k_bank_commit<false>;
    hipLaunchKernelGGL(fn, dim3((uint32_t)a.n_streams), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
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
