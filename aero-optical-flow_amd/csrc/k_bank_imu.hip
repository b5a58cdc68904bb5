// The IMU call of a stream bank (aof_bank_imu_device / aof_bank_imu_reset_device, include/aof.h "the stream bank's
// IMU"): the gyro integrator of mainloop.cpp:383-405 and the two send gates of mainloop.cpp:333-357 for S streams behind
// a push, ONE launch, a lane per stream:
//   * a lane loads its K sample counts and its 64-byte state once, all of these loads in flight together; the counts
//     are then clamped to M and packed into two 64-bit words;
//   * it walks the rounds in order.  A round's record and time are loaded first, then its samples in groups of kGroup:
//     none of these loads depends on the state, so every load of a group is in flight before the group's first step.
//     What a lane waits for is its own serial chain of double operations (a division, three multiplies and three adds
//     per sample, each behind the one before through `prev` and the sums), not memory: lanes with fewer samples idle
//     while the wave's longest chain runs, and 256 streams per workgroup keep four waves per group to hide it;
//   * imu_sample / imu_take (aof_imu_step.hpp: the arithmetic and the gates the host function runs) decide; a sent
//     record's frame is packed by pack_optical_flow_rad into the lane's own 44-byte slice of static LDS (aof_mavlink.hpp:
//     a private array would become scratch memory);
//   * records, lengths and frames are stored per round, lane-consecutive within a round; the state is stored once, and
//     the kernel ends with a system-scope release behind its stores: outputs kept in pinned host memory are there for a
//     host that sees the tag of a collect call enqueued behind this launch.
// In place (records_out == records_in) a lane reads a record before it writes it, and no lane touches another's.
// No cross-lane traffic, no waiting.  Samples, times and states are read in 8-byte words, records in 4-byte words (the
// entry point's alignment rules); gfx950 takes wider accesses at those addresses, so the compiler may join them.
#include <hip/hip_runtime.h>

#include "aof_bank_calls.hpp"
#include "aof_device.hpp"
#include "aof_imu_step.hpp"
#include "aof_mavlink.hpp"

namespace aof {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kGroup = 4;       // samples whose loads are in flight together: 24 VGPRs
constexpr uint32_t kSampleBytes = sizeof(aof_imu_sample), kRecordBytes = sizeof(aof_tick_record), kRecordWords = kRecordBytes / 4;
static_assert(kSampleBytes == 24 && offsetof(aof_imu_sample, xgyro) == 8 && offsetof(aof_imu_sample, zgyro) == 16,
              "a sample is three 8-byte words: time, (x, y), (z, reserved)");
static_assert(sizeof(aof_imu_state) == 64 && kRecordBytes == 48, "the state is 64 bytes, a record twelve words");
static_assert(AOF_BANK_BURST_MAX == 16 && AOF_IMU_SLOTS_MAX <= 255, "K counts of a byte each fill two 64-bit words");

__global__ __launch_bounds__(kThreads) void k_bank_imu(ImuArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_payload[kThreads * kMavlinkPayloadBytes];
    const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
    if (s < a.n_streams) {
        const size_t S = a.n_streams;
        const uint32_t M = a.max_samples, last = a.n_rounds - 1u;
        // the K counts of this stream and its state: every load issued before the first wait.  The count loads carry no
        // branch (the NULL case stands apart, in front): a round behind the last one reads the last one's count again
        // and is never walked.  They are clamped and packed only once all of them are there.
        uint64_t counts[2];
        aof_imu_state st = a.state[s];
        if (a.sample_count) {
            uint32_t c[AOF_BANK_BURST_MAX];
#pragma unroll
            for (uint32_t k = 0; k < AOF_BANK_BURST_MAX; k++) c[k] = a.sample_count[(size_t)min(k, last) * S + s];
            counts[0] = counts[1] = 0u;
#pragma unroll
            for (uint32_t k = 0; k < AOF_BANK_BURST_MAX; k++) counts[k >> 3] |= (uint64_t)min(c[k], M) << (8u * (k & 7u));
        } else {
            counts[0] = counts[1] = (uint64_t)M * 0x0101010101010101ull;
        }
        // the stream's MAVLink identity: the call's, or with an array bound (aof_set_bank_streams) the fourth word of the
        // stream's own record (system_id, component_id, first_seq, reserved); the branch is uniform
        uint32_t id = (uint32_t)a.system_id | (uint32_t)a.component_id << 8 | (uint32_t)a.first_seq << 16;
        if (a.streams) id = reinterpret_cast<const uint32_t *>(a.streams + s)[3];
        const uint8_t system_id = (uint8_t)id, component_id = (uint8_t)(id >> 8), first_seq = (uint8_t)(id >> 16);
        uint8_t *payload = s_payload + threadIdx.x * kMavlinkPayloadBytes;
        for (uint32_t k = 0; k <= last; k++) {
            const size_t o = (size_t)k * S + s;
            uint32_t rw[kRecordWords];
            const uint32_t *rin = reinterpret_cast<const uint32_t *>(a.records_in + o * kRecordBytes);
#pragma unroll
            for (uint32_t i = 0; i < kRecordWords; i++) rw[i] = rin[i];
            const uint64_t t = a.time_us[o];
            const uint32_t n = (uint32_t)((k < 8u ? counts[0] : counts[1]) >> (8u * (k & 7u))) & 0xFFu;
            const uint8_t *round = a.samples + ((size_t)k * M * S + s) * kSampleBytes;
            for (uint32_t j0 = 0; j0 < n; j0 += kGroup) {
                // (a slot behind the round's last sample reads the last one again -- the same cache line -- and is not stepped)
                uint64_t w[kGroup][3];
#pragma unroll
                for (uint32_t g = 0; g < kGroup; g++) {
                    const uint64_t *p = reinterpret_cast<const uint64_t *>(round + (size_t)min(j0 + g, n - 1u) * S * kSampleBytes);
                    w[g][0] = p[0]; w[g][1] = p[1]; w[g][2] = p[2];
                }
#pragma unroll
                for (uint32_t g = 0; g < kGroup; g++) {
                    if (j0 + g < n)
                        imu_sample(st, w[g][0], __uint_as_float((uint32_t)w[g][1]), __uint_as_float((uint32_t)(w[g][1] >> 32)),
                                   __uint_as_float((uint32_t)w[g][2]));
                }
            }
            aof_tick_record rec;
            __builtin_memcpy(&rec, rw, sizeof(rec));
            ImuFrame f;
            uint8_t len = 0;
            if (imu_take(st, rec, t, first_seq, f) && a.mavlink)
                len = (uint8_t)pack_optical_flow_rad(a.mavlink + o * AOF_SEQ_FRAME_BYTES, payload, f.time_usec, rec.dt_us, rec.flow_x,
                                                     rec.flow_y, f.gx, f.gy, f.gz, rec.quality, f.seq, system_id, component_id);
            __builtin_memcpy(rw, &rec, sizeof(rec));
            uint32_t *rout = reinterpret_cast<uint32_t *>(a.records_out + o * kRecordBytes);
#pragma unroll
            for (uint32_t i = 0; i < kRecordWords; i++) rout[i] = rw[i];
            if (a.mavlink_len) a.mavlink_len[o] = len;
        }
        a.state[s] = st;
    }
    // the outputs out to where a host reads them, before the launch counts as done
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

__global__ __launch_bounds__(kThreads) void k_bank_imu_reset(aof_imu_state *state, const uint8_t *mask, uint32_t n, uint64_t offset0)
{
    const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
    if (s >= n || (mask && !mask[s])) return;
    aof_imu_state z = {};
    z.offset_timestamp_usec = offset0;   // 0: the stream's first sample sets it
    state[s] = z;
}

}  // namespace

int launch_bank_imu(const ImuArgs &a, void *stream)
{
    if (a.n_streams < 1 || a.n_rounds < 1 || a.n_rounds > AOF_BANK_BURST_MAX || a.max_samples < 1 || a.max_samples > AOF_IMU_SLOTS_MAX ||
        !a.samples || !a.time_us || !a.records_in || !a.records_out || !a.state || !a.mavlink != !a.mavlink_len)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bank_imu, dim3((a.n_streams + kThreads - 1) / kThreads), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

int launch_bank_imu_reset(aof_imu_state *state, const uint8_t *mask, uint32_t n_streams, uint64_t offset0, void *stream)
{
    if (n_streams < 1 || !state) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bank_imu_reset, dim3((n_streams + kThreads - 1) / kThreads), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), state, mask, n_streams, offset0);
    return (int)hipGetLastError();
}

}  // namespace aof
