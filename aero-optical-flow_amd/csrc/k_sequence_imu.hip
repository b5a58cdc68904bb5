// The sequence pipeline's IMU (aof_sequence_imu_device, include/aof_sequence_imu.h): the gyro integrator of
// mainloop.cpp:383-405 and the two send gates of mainloop.cpp:333-357 for ONE recorded stream of n frames and T samples,
// behind a records-only aof_sequence_device call.  The stream bank walks a stream serially, a lane per stream; a recording
// is one stream, so the serial run is restated in parallel ("Sequence IMU"; exact, not approximate).
// With E(m) = min(T, sample_end[frame of record m]), E(-1) = 0, and p_m = the time of sample E(m) - 1 (0 for E(m) = 0):
//   * whether sample i is accepted depends on it and on the time of sample i - 1 alone (0 for i = 0);
//   * the sums of record m are the accepted samples of [E(m-1), E(m)), added in order from 0.0: one lane walks one window;
//   * record m is stale iff p_m == p_(m-1): last_taken_time_usec is p_(m-1) behind record m - 1 whichever way it went;
//   * the vehicle time is offset0, or the time of the first sample with a non-zero time once it lies in front of E(m);
//   * a sent record's sequence number is first_seq + the number of sent records in front of it.
// So a lane seeds a local aof_imu_state with what the serial run would hold at the start of its window and runs the steps
// of aof_imu_step.hpp on it: the arithmetic and the gates are that file's, nothing of them is written here.
//   k_seq_imu_init     zeroes the three words;
//   k_seq_imu_samples  a lane per sample: index of the first non-zero time (wave minimum, one atomic per wave), accepted
//                      and rejected samples of [0, E_last) (ballots, one atomic per wave and counter);
//   k_seq_imu_records  a lane per record, and one for the tail window [E(M-1), E_last) whose sums the final state keeps:
//                      the window walk, the gates, quality and gyro floats stored; the workgroup leaves its count of sent
//                      records;
//   k_seq_imu_scan     exclusive scan of up to 256 counts per workgroup in place, its total to the next level; launched
//                      once per level, the top level by one workgroup, which also finishes count[1] and the state;
//   k_seq_imu_pack     a lane per record: scanned offsets of its workgroup + its rank inside the workgroup = the sequence
//                      number; packs the frame (aof_mavlink.hpp) through the lane's own 44 bytes of LDS.
// No workgroup waits for another inside a launch: the order is the stream's.  Every index read from device memory is clamped:
// a frame index into [0, n), a sample count to T, count[0] to n; a window with E(m) < E(m-1) is empty.  A window walk ends
// after at most T samples.
#include <hip/hip_runtime.h>

#include "aof_device.hpp"
#include "aof_imu_step.hpp"
#include "aof_mavlink.hpp"
#include "aof_sequence_imu_args.hpp"

namespace aof {

namespace {

constexpr int kThreads = (int)kSeqImuThreads, kWaves = kThreads / 64;
constexpr uint32_t kSampleBytes = sizeof(aof_imu_sample);
constexpr uint32_t kGroup = 4;   // samples whose loads are in flight together
static_assert(kSampleBytes == 24 && offsetof(aof_imu_sample, xgyro) == 8 && offsetof(aof_imu_sample, zgyro) == 16,
              "a sample is three 8-byte words: time, (x, y), (z, reserved)");
static_assert(sizeof(aof_seq_record) == 32, "a record is eight words");

__device__ __forceinline__ const uint64_t *sample_words(const uint8_t *samples, uint32_t i)
{
    return reinterpret_cast<const uint64_t *>(samples + (size_t)i * kSampleBytes);
}

// p of a sample count e <= T: the time of sample e - 1, 0 in front of the first
__device__ __forceinline__ uint64_t time_before(const SeqImuArgs &a, uint32_t e) { return e > 0 ? sample_words(a.samples, e - 1u)[0] : 0u; }

// E of frame f (clamped into the recording)
__device__ __forceinline__ uint32_t samples_before_frame(const SeqImuArgs &a, uint32_t f)
{
    const uint32_t last = (uint32_t)(a.n_frames - 1);
    return min(a.sample_end[min(f, last)], a.n_samples);
}

// index of the first sample with a non-zero time, T where there is none
__device__ __forceinline__ uint32_t first_timed_sample(const SeqImuArgs &a)
{
    const uint32_t w = a.words[kSeqImuFirst];
    return w ? ~w : a.n_samples;
}

// this lane's rank among the lanes of its workgroup with `flag` set, and (total) their number; every lane calls it
__device__ __forceinline__ uint32_t workgroup_rank(bool flag, uint32_t *s_wave, uint32_t &total)
{
    const unsigned long long mask = __ballot(flag);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)kWaves; w++) {
        const uint32_t c = s_wave[w];
        rank += w < wave ? c : 0u;
        total += c;
    }
    return rank;
}

__global__ __launch_bounds__(64) void k_seq_imu_init(SeqImuArgs a)
{
    if (threadIdx.x < (uint32_t)kSeqImuWords) a.words[threadIdx.x] = 0u;
}

__global__ __launch_bounds__(kThreads) void k_seq_imu_samples(SeqImuArgs a)
{
    const uint32_t T = a.n_samples;   // >= 1: the launcher skips the pass for T == 0
    const uint64_t gi = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool in = gi < T;
    const uint32_t i = in ? (uint32_t)gi : T - 1u;   // (lanes behind the last sample read it again and count nothing)
    const uint32_t e_last = samples_before_frame(a, (uint32_t)(a.n_frames - 1));
    const uint64_t *w = sample_words(a.samples, i);
    const uint64_t t = w[0], xy = w[1], z = w[2];
    aof_imu_state st = {};
    st.prev_time_usec = time_before(a, i);
    imu_sample(st, t, __uint_as_float((uint32_t)xy), __uint_as_float((uint32_t)(xy >> 32)), __uint_as_float((uint32_t)z));
    const bool counted = in && i < e_last;
    const uint32_t accepted = (uint32_t)__popcll(__ballot(counted && st.samples_integrated != 0u));
    const uint32_t rejected = (uint32_t)__popcll(__ballot(counted && st.samples_integrated == 0u));
    const uint32_t first = wave_min_u32(in && t != 0u ? i : 0xFFFFFFFFu);
    if ((threadIdx.x & 63u) == 0u) {
        if (accepted) atomicAdd(&a.words[kSeqImuAccepted], accepted);
        if (rejected) atomicAdd(&a.words[kSeqImuRejected], rejected);
        if (first != 0xFFFFFFFFu) atomicMax(&a.words[kSeqImuFirst], ~first);   // (i <= 2^32 - 2: ~i is never 0)
    }
}

// The samples of [lo, hi) through imu_sample, in order.
__device__ __forceinline__ void walk_window(const SeqImuArgs &a, aof_imu_state &st, uint32_t lo, uint32_t hi)
{
#pragma clang fp contract(off)
    for (uint32_t j0 = lo; j0 < hi; j0 += min(kGroup, hi - j0)) {
        // (a slot behind the window's last sample reads the last one again and is not stepped)
        uint64_t w[kGroup][3];
#pragma unroll
        for (uint32_t g = 0; g < kGroup; g++) {
            const uint64_t *p = sample_words(a.samples, j0 + min(g, hi - 1u - j0));
            w[g][0] = p[0]; w[g][1] = p[1]; w[g][2] = p[2];
        }
#pragma unroll
        for (uint32_t g = 0; g < kGroup; g++) {
            if (g < hi - j0)
                imu_sample(st, w[g][0], __uint_as_float((uint32_t)w[g][1]), __uint_as_float((uint32_t)(w[g][1] >> 32)),
                           __uint_as_float((uint32_t)w[g][2]));
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_seq_imu_records(SeqImuArgs a)
{
    __shared__ uint32_t s_wave[kWaves];
    const uint64_t n = (uint64_t)a.n_frames;
    const uint64_t m = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t M = min((uint64_t)a.count[0], n);
    bool sent = false;
    if (m <= M) {   // (m == M: the tail window, which no record takes)
        aof_seq_record rec = {};
        if (m < M) rec = a.records[m];
        const uint32_t hi = samples_before_frame(a, m < M ? rec.frame : (uint32_t)(n - 1));
        const uint32_t lo = m > 0 ? samples_before_frame(a, a.records[m - 1].frame) : 0u;
        const uint32_t first = first_timed_sample(a);
        // the state the serial run holds where this window begins
        aof_imu_state st = {};
        st.prev_time_usec = st.last_taken_time_usec = time_before(a, lo);
        st.offset_timestamp_usec = a.offset0 ? a.offset0 : first < hi ? sample_words(a.samples, first)[0] : 0u;
        walk_window(a, st, lo, hi);
        if (m < M) {
            ImuFrame f;
            sent = imu_take(st, rec, 0u, a.first_seq, f);   // (the frame is packed behind the scan: k_seq_imu_pack)
            aof_seq_record *out = a.records + m;
            out->quality = rec.quality;
            out->gyro_x = rec.gyro_x; out->gyro_y = rec.gyro_y; out->gyro_z = rec.gyro_z;
        } else if (a.state) {   // (messages and the three counters: the top level of the scan)
            a.state->gyro_x = st.gyro_x; a.state->gyro_y = st.gyro_y; a.state->gyro_z = st.gyro_z;
            a.state->prev_time_usec = st.prev_time_usec;
            a.state->last_taken_time_usec = st.last_taken_time_usec;
            a.state->offset_timestamp_usec = st.offset_timestamp_usec;
        }
    }
    uint32_t total;
    workgroup_rank(sent, s_wave, total);
    if (threadIdx.x == 0) a.sums[0][blockIdx.x] = total;
}

// level[i] becomes the sum of the entries in front of it inside its group of kThreads; the group's total goes to the next
// level, or (top) to count[1] and the state.
__global__ __launch_bounds__(kThreads) void k_seq_imu_scan(SeqImuArgs a, int level, uint32_t entries, int top)
{
    __shared__ uint32_t s_wave[kWaves];
    uint32_t *v = a.sums[level];
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t mine = i < entries ? v[i] : 0u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, o, 64);
        incl += lane >= (uint32_t)o ? up : 0u;
    }
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)kWaves; w++) {
        const uint32_t c = s_wave[w];
        before += w < wave ? c : 0u;
        total += c;
    }
    if (i < entries) v[i] = before + incl - mine;
    if (threadIdx.x != 0) return;
    if (!top) {
        a.sums[level + 1][blockIdx.x] = total;
        return;
    }
    a.count[1] = total;
    if (a.state) {
        const uint32_t M = (uint32_t)min((uint64_t)a.count[0], (uint64_t)a.n_frames);
        a.state->messages = total;
        a.state->samples_integrated = a.words[kSeqImuAccepted];
        a.state->samples_rejected = a.words[kSeqImuRejected];
        a.state->dropped = M - total;
    }
}

__global__ __launch_bounds__(kThreads) void k_seq_imu_pack(SeqImuArgs a, int levels)
{
    __shared__ uint32_t s_wave[kWaves];
    __shared__ __attribute__((aligned(16))) uint8_t s_payload[kThreads * kMavlinkPayloadBytes];
    const uint64_t n = (uint64_t)a.n_frames;
    const uint64_t m = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t M = min((uint64_t)a.count[0], n);
    aof_seq_record rec = {};
    if (m < M) rec = a.records[m];
    const bool sent = m < M && rec.quality >= 0;   // (what k_seq_imu_records dropped is negative now)
    uint32_t total;
    uint32_t seq = workgroup_rank(sent, s_wave, total) + a.sums[0][blockIdx.x];
    if (levels > 1) seq += a.sums[1][blockIdx.x >> 8];
    if (levels > 2) seq += a.sums[2][blockIdx.x >> 16];
    if (m >= M) return;
    uint8_t len = 0;
    if (sent) {
        const uint32_t frame = min(rec.frame, (uint32_t)(n - 1));
        const uint32_t first = first_timed_sample(a);
        const uint64_t offset = a.offset0 ? a.offset0 : first < a.n_samples ? sample_words(a.samples, first)[0] : 0u;
        // (the float sums widened again: the packer narrows them, and narrowing commutes with the sign of the axis switch)
        len = (uint8_t)pack_optical_flow_rad(a.frames + (size_t)m * AOF_SEQ_FRAME_BYTES, s_payload + threadIdx.x * kMavlinkPayloadBytes,
                                             offset + a.time_us[frame], rec.dt_us, rec.flow_x, rec.flow_y, (double)rec.gyro_x,
                                             (double)rec.gyro_y, (double)rec.gyro_z, rec.quality, (uint8_t)(a.first_seq + seq),
                                             a.system_id, a.component_id);
    }
    a.frame_len[m] = len;
}

}  // namespace

int launch_sequence_imu(const SeqImuArgs &a, void *stream)
{
    if (a.n_frames < 1 || a.n_frames >= 0x7FFFFFF0ll || !a.time_us || !a.sample_end || !a.count || !a.records || !a.frames ||
        !a.frame_len || !a.words || (!a.samples && a.n_samples > 0))
        return (int)hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // entries per level: workgroups of the record pass, then one total per kSeqImuThreads entries
    int64_t entries[kSeqImuLevels];
    int levels = 0;
    for (int64_t e = seq_imu_groups(a.n_frames + 1);; e = seq_imu_groups(e)) {
        if (levels == kSeqImuLevels) return (int)hipErrorInvalidValue;
        if (!a.sums[levels]) return (int)hipErrorInvalidValue;
        entries[levels++] = e;
        if (e <= (int64_t)kSeqImuThreads) break;
    }
    const dim3 block(kThreads), records((uint32_t)entries[0]);
    hipLaunchKernelGGL(k_seq_imu_init, dim3(1), dim3(64), 0, s, a);
    if (a.n_samples > 0)
        hipLaunchKernelGGL(k_seq_imu_samples, dim3((uint32_t)seq_imu_groups((int64_t)a.n_samples)), block, 0, s, a);
    hipLaunchKernelGGL(k_seq_imu_records, records, block, 0, s, a);
    for (int l = 0; l < levels; l++)
        hipLaunchKernelGGL(k_seq_imu_scan, dim3((uint32_t)seq_imu_groups(entries[l])), block, 0, s, a, l, (uint32_t)entries[l],
                           l == levels - 1 ? 1 : 0);
    hipLaunchKernelGGL(k_seq_imu_pack, records, block, 0, s, a, levels);
    return (int)hipGetLastError();
}

}  // namespace aof
