// What one stream of the bank does with one frame, shared by the tick kernels (k_bank.hip) and the burst kernel
// (k_bank_burst.hip): the idle record, the exposure gate and the MSV, the tail (rate limiter, angles, gyro sums,
// OPTICAL_FLOW_RAD frame), the masked histogram and the frame copies.  One function each, as aof_flow_small.hpp has one
// function for the pair: a record cannot depend on the entry point that produced it.
// The tail is the facade's limitRate() / integrate() (facade/src/optical_flow.cpp) and mainloop.cpp:322-373 on ONE
// stream's state: every float operation is the host's, in the host's order.
#pragma once

#include "aof_bank_args.hpp"
#include "aof_derotate.hpp"
#include "aof_engine_args.hpp"
#include "aof_exposure_step.hpp"
#include "aof_flow_small.hpp"
#include "aof_bank_sensor_rule.hpp"   // (behind the HIP runtime's qualifiers)
#include "aof_mavlink.hpp"
#include "aof_math.h"

namespace aof {

namespace {

// The record of a stream without a frame in round o: idle, or (quality AOF_TICK_BAD_SENSOR) given one its sensor record
// does not let the kernels read.  Nothing else differs.
template <bool CAMERA>
__device__ __forceinline__ void bank_idle(const BankArgs &a, size_t o, int32_t quality = AOF_TICK_IDLE)
{
    aof_tick_record rec = {};
    rec.quality = quality;
    a.records[o] = rec;
    if (a.mavlink_len) a.mavlink_len[o] = 0;
    if constexpr (CAMERA) {
        if (a.cam.exposure) a.cam.exposure[o] = aof_exposure_record{};
        if (a.cam.derotated) { a.cam.derotated[2 * o] = 0.0f; a.cam.derotated[2 * o + 1] = 0.0f; }
    }
}

// Is a frame of 64-bit time t due for exposure statistics (mainloop.cpp:199-201: the untruncated time)?
__device__ __forceinline__ bool exposure_due(const BankArgs &a, const BankState &st, uint64_t t)
{
    return a.cam.exposure != nullptr && t >= st.next_exposure_us;
}

// What belongs to ONE camera and its vehicle: the limiter's rate and period, the focal lengths, the vehicle-time offset and
// the MAVLink identity.  The one place they are resolved: from the call's scalars (aof_bank_params), or, with an array
// bound (aof_set_bank_streams), from stream s's record -- two 16-byte loads by the lane that runs the tail, made inside
// the tail so that nothing of the record is live across a pair.  The branch is uniform, and without an array the values
// are the kernel arguments themselves.  The period is limiter_period_us's float: one correctly rounded division.
struct BankStream {
    int32_t output_rate;
    float period_us, focal_x, focal_y;
    uint64_t offset_timestamp_usec;
    uint8_t system_id, component_id, first_seq;
};
static_assert(sizeof(aof_bank_stream) == 32 && offsetof(aof_bank_stream, output_rate) == 8 && offsetof(aof_bank_stream, system_id) == 12 &&
              offsetof(aof_bank_stream, offset_timestamp_usec) == 16, "a stream record is two 16-byte words");

__device__ __forceinline__ BankStream bank_stream(const BankArgs &a, uint32_t s)
{
    BankStream v;
    if (a.streams) {
        const uint4 *rec = reinterpret_cast<const uint4 *>(a.streams + s);
        const uint4 lo = rec[0], hi = rec[1];
        v.focal_x = __uint_as_float(lo.x); v.focal_y = __uint_as_float(lo.y);
        v.output_rate = (int32_t)lo.z;
        v.period_us = v.output_rate > 0 ? 1.0e6f / (float)v.output_rate : 0.0f;
        v.system_id = (uint8_t)lo.w; v.component_id = (uint8_t)(lo.w >> 8); v.first_seq = (uint8_t)(lo.w >> 16);
        v.offset_timestamp_usec = (uint64_t)hi.x | (uint64_t)hi.y << 32;
    } else {
        v.output_rate = a.output_rate; v.period_us = a.period_us;
        v.focal_x = a.focal_x; v.focal_y = a.focal_y;
        v.offset_timestamp_usec = a.offset_timestamp_usec;
        v.system_id = a.system_id; v.component_id = a.component_id; v.first_seq = a.first_seq;
    }
    return v;
}

// What stream s's sensor record (aof_set_bank_sensors) means for a crop of w x h in the round whose frames start `base`
// bytes into the camera buffer: where the crop starts behind the round's first byte, how far apart its rows lie, and
// whether one byte of it may be read.  The ONE place that is decided: tick, burst, commit and ingest cannot disagree
// (the rule itself: aof_bank_sensor_rule.hpp, which the host compiles too).  The record is the same for every lane of a
// workgroup (a workgroup serves one stream, or one strip of one frame): its 32 bytes are read through the scalar path
// (the constant address space, from an address made of kernel arguments and blockIdx), so the values arrive in scalar
// registers and the arithmetic below costs no lane anything.  Records rewritten between launches are seen -- the scalar
// cache does not outlive a launch --, which tests/test_gpu_bank_sensors.py holds with offsets rewritten before every
// tick, eagerly and through a replayed graph (test_offsets_rewritten_every_tick_eager_and_through_a_replayed_graph).
// With a format array bound as well (aof_set_bank_pixel_formats) stream s's format byte decides the row's layout
// (bank_pixel_layout: group bytes and shift); it is read by the lanes (one byte, no alignment, nothing outside
// formats[0..S)) and made uniform, so every branch on it is a scalar one.  A value that is no format makes the record
// invalid (a layout of no groups).
// With a binning array bound (aof_set_bank_binning) stream s's byte is read the same way and decides `bin`: the crop's
// footprint is bin * w x bin * h sensor pixels at (x0, y0); a value that is none of 1, 2, 4 makes the record invalid.
struct BankSensor {
    int64_t origin;    // offset + y0 * pitch + x0 / G * gb: the first byte of the crop's first group (0 for an invalid record)
    CropSource crop;   // the record's pitch, its format's group bytes and shift, its bin (aof_crop.hpp)
    bool ok;
};
static_assert(sizeof(aof_bank_sensor) == 32 && offsetof(aof_bank_sensor, pitch) == 8 && offsetof(aof_bank_sensor, width) == 12 &&
              offsetof(aof_bank_sensor, height) == 16 && offsetof(aof_bank_sensor, x0) == 20 && offsetof(aof_bank_sensor, y0) == 24,
              "a sensor record is two 16-byte words");

__device__ __forceinline__ BankSensor bank_sensor(const aof_bank_sensor *sensors, size_t s, int32_t w, int32_t h, uint64_t base,
                                                  uint64_t camera_bytes, const uint8_t *formats = nullptr, const uint8_t *bins = nullptr)
{
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef const u32x4 __attribute__((address_space(4))) *const_words;
    const const_words rec = reinterpret_cast<const_words>(reinterpret_cast<uintptr_t>(sensors + s));
    const u32x4 lo = rec[0], hi = rec[1];
    const uint64_t offset = (uint64_t)lo.x | (uint64_t)lo.y << 32;
    const int32_t pitch = (int32_t)lo.z, width = (int32_t)lo.w, height = (int32_t)hi.x, x0 = (int32_t)hi.y, y0 = (int32_t)hi.z;
    BankSensor v;
    BankPixelLayout l = {1, 1, 0};
    if (formats) l = bank_pixel_layout((uint32_t)__builtin_amdgcn_readfirstlane((int)formats[s]));
    v.crop.gb = l.group_bytes; v.crop.shift = l.shift;
    v.crop.bin = 1;
    if (bins) v.crop.bin = __builtin_amdgcn_readfirstlane((int)bins[s]);
    v.ok = bank_sensor_valid_groups(offset, pitch, width, height, x0, y0, w, h, base, camera_bytes, l.group_px, l.group_bytes, v.crop.bin);
    v.crop.pitch = pitch;
    v.origin = v.ok ? (int64_t)offset + (int64_t)y0 * pitch + (int64_t)(x0 >> (l.group_px >> 1)) * l.group_bytes : 0;   // (x0 is whole groups of 1, 2 or 4)
    return v;
}

// One lane: a stream has been given a frame; `st` is the stream's state record, `f` the pixel record of (older frame,
// new frame), `first` says that there was no older frame.  `o` indexes the frame's time, gyro sample and every output:
// the stream's number in a tick, round * S + stream in a burst.  payload: kMavlinkPayloadBytes of LDS for the packer.
// CAMERA: `hist` holds the frame's ten raw bin totals if the frame is due (exposure_due; LDS or global memory).
// The ONE place a record is made: a tick's (bank_tail below) and a burst round's cannot differ.
template <bool CAMERA>
__device__ __forceinline__ void bank_tail_step(const BankArgs &a, size_t o, uint32_t s, BankState &st, aof_flow f, bool first,
                                               uint8_t *payload, const uint32_t *hist = nullptr)
{
    const uint64_t t64 = a.time_us[o];
    const BankStream c = bank_stream(a, s);   // (behind the time's load: the record's loads are in flight with it, one wait for both)
    if constexpr (CAMERA) {
        if (a.cam.exposure) {
            aof_exposure_record e = {};
            if (exposure_due(a, st, t64)) {
                for (int i = 0; i < AOF_EXPOSURE_BINS; i++) e.hist[i] = hist[i];
                e.msv = exposure_msv(e.hist);
                e.due = 1;
                st.next_exposure_us = t64 + a.cam.interval_us;
            }
            a.cam.exposure[o] = e;
        }
        if (a.cam.derotated) {   // of the pair's own pixel record, whatever the limiter does with it
            float x = 0.0f, y = 0.0f;
            if (!first) derotate_flow(a.cam.derotate, f, a.gyro ? a.gyro[o] : aof_gyro{}, &x, &y);
            a.cam.derotated[2 * o] = x;
            a.cam.derotated[2 * o + 1] = y;
        }
    }
    const uint32_t t = (uint32_t)t64;   // calcFlow sees 32 bits (mainloop.cpp:305-315)
    st.frames++;
    if (a.gyro) {                       // integrated since the last message (mainloop.cpp:383-405)
        const aof_gyro g = a.gyro[o];
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
        if (c.output_rate <= 0) {       // limitRate: no limit, the frame's own flow and quality
            dt_us = (int)(t - st.time_last_pub);
            st.time_last_pub = t;
        } else {
            if (quality > 0) {
                st.sum_flow_x += px;
                st.sum_flow_y += py;
                st.sum_flow_quality += quality;
                st.valid_frame_count++;
            }
            if ((float)(t - st.time_last_pub) > c.period_us) {
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
        if (!first) { ang_x = aof_atan2f(px, c.focal_x); ang_y = aof_atan2f(py, c.focal_y); }
        rec.dt_us = dt_us;
        rec.flow_x = ang_x; rec.flow_y = ang_y;
        rec.gyro_x = (float)st.gyro_x; rec.gyro_y = (float)st.gyro_y; rec.gyro_z = (float)st.gyro_z;
        if (a.mavlink && c.offset_timestamp_usec != 0)   // (0: vehicle time not known, nothing is sent; mainloop.cpp:353-357)
            len = (uint8_t)pack_optical_flow_rad(a.mavlink + o * AOF_SEQ_FRAME_BYTES, payload, c.offset_timestamp_usec + t64, dt_us,
                                                 ang_x, ang_y, st.gyro_x, st.gyro_y, st.gyro_z, quality,
                                                 (uint8_t)(c.first_seq + st.messages), c.system_id, c.component_id);
        st.messages++;
        st.gyro_x = 0.0; st.gyro_y = 0.0; st.gyro_z = 0.0;   // taken with the message (mainloop.cpp:333-334)
    }
    a.records[o] = rec;
    if (a.mavlink_len) a.mavlink_len[o] = len;
}

// The tail of a tick: the state record comes from the bank and goes back to it.
template <bool CAMERA>
__device__ __forceinline__ void bank_tail(const BankArgs &a, uint32_t s, aof_flow f, bool first, uint8_t *payload,
                                          const uint32_t *hist = nullptr)
{
    BankState st = a.state[s];
    bank_tail_step<CAMERA>(a, s, s, st, f, first, payload, hist);
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

// CAMERA: is stream s's frame its first (bit 0), is it due for exposure statistics (bit 1), and does the stream's
// sensor record keep the kernels from reading it (bit 2: sensor_ok false)?  One lane reads the state and the time, like
// bank_first.
constexpr uint32_t kGateFirst = 1u, kGateDue = 2u, kGateBadSensor = 4u;
__device__ __forceinline__ uint32_t bank_gate(const BankArgs &a, uint32_t s, bool sensor_ok = true)
{
    __shared__ uint32_t s_gate;
    if (threadIdx.x == 0) {
        const BankState st = a.state[s];
        s_gate = (st.has_prev == 0 ? kGateFirst : 0u) | (exposure_due(a, st, a.time_us[s]) ? kGateDue : 0u) |
                 (sensor_ok ? 0u : kGateBadSensor);
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
__device__ __forceinline__ void crop_first_frame(const BankCamera &c, const uint8_t *src, const CropSource &from, uint8_t *lds, uint8_t *slot)
{
    const int row_chunks = c.crop_w / 16, chunks = row_chunks * c.crop_h;
    for (int i = threadIdx.x; i < chunks; i += kThreads) {
        const int y = i / row_chunks, x = i - y * row_chunks;
        uint4 v;
        crop_piece(v, src, y, x, from);
        reinterpret_cast<uint4 *>(lds)[i] = v;
        reinterpret_cast<uint4 *>(slot)[i] = v;
    }
    __syncthreads();
}

// Where stream s's new frames start and how far apart their rows lie: the crop rectangle inside its sensor frame, or
// its frame in the tick buffer.  With a BankSensors argument (the instantiations for a bound array): by the stream's
// record, for the round whose frames start `base` bytes into the camera buffer (a.cam.camera is round 0's first byte);
// ok false: the record forbids the read (src is then the buffer's first byte and must not be used).  Without one:
// by the call's scalars, and ok is the constant true -- everything that asks for it folds away.
struct BankSource {
    const uint8_t *src;
    CropSource crop;   // grey, unbinned -- constants -- without a sensor argument
    bool ok;
};
template <bool CAMERA>
__device__ __forceinline__ BankSource bank_source(const BankArgs &a, uint32_t s, uint64_t base = 0)
{
    if constexpr (CAMERA) return BankSource{a.cam.camera + (int64_t)s * a.cam.camera_stride + a.cam.origin, crop_grey(a.cam.pitch), true};
    else return BankSource{a.frames + (int64_t)s * a.frame_stride, crop_grey(0), true};
}
template <bool CAMERA>
__device__ __forceinline__ BankSource bank_source(const BankArgs &a, uint32_t s, uint64_t base, const BankSensors &sen)
{
    static_assert(CAMERA, "sensor records belong to the camera forms");
    const BankSensor r = bank_sensor(sen.recs, s, a.cam.crop_w, a.cam.crop_h, sen.camera_base + base, sen.camera_bytes, sen.formats,
                                     sen.bins);
    return BankSource{a.cam.camera + r.origin, r.crop, r.ok};
}

// The stream's newest frame out of LDS into its slot, by the whole workgroup.
__device__ __forceinline__ void store_slot(const BankArgs &a, uint8_t *slot, const uint8_t *lds_new)
{
    for (int c = threadIdx.x; c < (int)(a.frame_bytes / 16); c += kThreads)
        reinterpret_cast<uint4 *>(slot)[c] = reinterpret_cast<const uint4 *>(lds_new)[c];
}

// Host: does the small-pair plan `sm` belong to the bank `a`?  What launch_bank_tick and launch_bank_burst check before
// they hand both to a kernel: a workgroup per stream, the plan's frame the bank's (in 16-byte chunks), and the camera
// crop the plan's frame.
inline bool bank_plan_fits(const SmallArgs &sm, const BankArgs &a)
{
    if (a.n_streams < 1 || sm.l0.n_pairs != a.n_streams) return false;
    if (a.frame_bytes != (int64_t)sm.l0.w * sm.l0.h || a.frame_bytes % 16) return false;
    return a.cam.camera == nullptr || (a.cam.crop_w == sm.l0.w && a.cam.crop_h == sm.l0.h);
}

}  // namespace

}  // namespace aof
