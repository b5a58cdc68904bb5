// The MAVLink receive of a stream bank (aof_bank_mavlink_rx_device / aof_bank_mavlink_rx_reset_device, include/aof.h
// "the stream bank's MAVLink receive"): what mavlink_tcp.cpp:100-129 does for one connection -- mavlink_parse_char byte
// by byte, HIGHRES_IMU decoded -- for S connections, ONE launch, a lane per stream (framing is serial per stream):
//   * a workgroup is ONE wave of 64 streams with LDS of its own.  There is no workgroup barrier anywhere: a wave runs
//     its ds instructions in order, so what its lanes stored is there for its lanes' loads, and the only thing between
//     the two is a workgroup-scope fence for the compiler.  Nothing waits on another lane, workgroup or the host;
//   * a round's bytes come through LDS in pieces of 128 bytes per stream: eight 16-byte loads per lane, each one
//     covering eight streams' whole 128-byte lines (lane l: stream l / 8 of the eight, 16-byte unit l % 8), four in
//     flight together, then their four 16-byte stores.  A lane never fetches its own bytes from memory: that would be
//     64 cache lines per load instruction;
//   * a stream's piece lies at 144 * lane in LDS: nine 16-byte slots, and 9 is odd, so the sixteen lanes a 16-byte read
//     serves per cycle fall on sixteen different slots of the 256-byte bank row;
//   * the lane walks its piece in chunks of 16 bytes, one 16-byte LDS read each.  Per chunk, in this order: nothing left
//     of the stream's length -> nothing; the rest of a frame of another message covers the chunk -> rx_skip, 16 bytes in
//     one step; idle and no byte of the chunk can be a start byte -> rx_skip_idle, likewise; else byte by byte with the
//     same two bulk steps inside (rx_byte, aof_mavlink_rx_step.hpp: the state machine the host function runs);
//   * trip counts: pieces and chunks count up to B, which is uniform; a piece no lane of the wave has bytes in ends
//     the round for the wave (a ballot: uniform by construction); the walk inside a chunk is bounded by its 16 bytes.
//     Every loop is bounded by K * B.  The state machine is resumable, so piece and chunk edges need no special case;
//   * the state (its 64 live bytes) is loaded once and stored once; the frame in progress lives in registers as 32-bit
//     fields (MavRx), never in an array: no scratch memory;
//   * a sample is stored from inside the walk (six words, slot `count` of the round); the count of every (k, s) is
//     stored behind the round, and the kernel ends with a system-scope release behind its stores.
#include <hip/hip_runtime.h>

#include "aof_bank_calls.hpp"
#include "aof_mavlink_rx_step.hpp"

namespace aof {

namespace {

constexpr uint32_t kWave = 64;            // streams per workgroup: one wave
constexpr uint32_t kPiece = 128;          // bytes of a stream staged at a time: a cache line
constexpr uint32_t kStride = kPiece + 16; // a stream's piece in LDS: nine 16-byte slots
constexpr uint32_t kChunk = 16;
constexpr uint32_t kLoads = 4;            // 16-byte loads a lane has in flight while staging: 16 VGPRs
static_assert(sizeof(aof_imu_sample) == 24, "a sample is six words");

// byte i of a chunk held as two 64-bit words (two shifts of registers: an indexed vector would become scratch memory)
__device__ __forceinline__ uint32_t chunk_byte(uint64_t lo, uint64_t hi, uint32_t i)
{
    return (uint32_t)((i < 8u ? lo : hi) >> (8u * (i & 7u))) & 0xFFu;
}

// (a one-wave workgroup would be given up to 512 registers; four waves per SIMD as every kernel here: at most 128)
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(4))) void k_bank_mavlink_rx(MavlinkRxArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_piece[kWave * kStride];
    const uint32_t lane = threadIdx.x, s0 = blockIdx.x * kWave, s = s0 + lane;
    const bool live = s < a.n_streams;
    const size_t S = a.n_streams;
    const uint32_t B = a.max_bytes, M = a.max_samples;

    // (a lane without a stream walks nothing, but fetches and stages its share of the others' lines)
    MavRxBytes *mem = reinterpret_cast<MavRxBytes *>(a.state + (live ? s : 0u));
    MavRx r;
    rx_load(r, *mem);

    // what this lane fetches of a piece: unit `unit` of the lines of streams s0 + i * 8 + lane / 8, i = 0 .. 7
    const uint32_t unit = lane & 7u, row = lane >> 3;

    for (uint32_t k = 0; k < a.n_rounds; k++) {
        const size_t o = (size_t)k * S + s;
        uint32_t n = 0;
        if (live) n = a.len ? min((uint32_t)a.len[o], B) : B;
        uint32_t count = 0;
        for (uint32_t p0 = 0; p0 < B; p0 += kPiece) {
            if (__ballot(n > p0) == 0ull) break;          // no lane of the wave has a byte at or behind p0
            // (the previous piece's reads are behind us: every lane's walk ended before this point in program order)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            const bool in_slot = p0 + unit * 16u < B;
            const uint8_t *src = a.bytes + ((size_t)k * S + s0 + row) * B + p0 + unit * 16u;
            uint8_t *dst = s_piece + row * kStride + unit * 16u;
#pragma unroll 1
            for (uint32_t h = 0; h < 8u; h += kLoads) {   // kLoads lines in flight per lane
                uint4 line[kLoads];
#pragma unroll
                for (uint32_t i = 0; i < kLoads; i++) {
                    line[i] = make_uint4(0u, 0u, 0u, 0u);
                    if (in_slot && s0 + (h + i) * 8u + row < a.n_streams)
                        line[i] = *reinterpret_cast<const uint4 *>(src + (size_t)(h + i) * 8u * B);
                }
#pragma unroll
                for (uint32_t i = 0; i < kLoads; i++) *reinterpret_cast<uint4 *>(dst + (h + i) * 8u * kStride) = line[i];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

#pragma unroll 1
            for (uint32_t c0 = 0; c0 < kPiece; c0 += kChunk) {
                const uint32_t at = p0 + c0;
                if (__ballot(n > at) == 0ull) break;
                if (n <= at) continue;
                const uint32_t m = min(n - at, kChunk);   // bytes of this chunk the stream received: 1..16
                const uint4 c = *reinterpret_cast<const uint4 *>(s_piece + lane * kStride + c0);
                const uint64_t lo = (uint64_t)c.y << 32 | c.x, hi = (uint64_t)c.w << 32 | c.z;
                if (rx_skippable(r) >= m) {
                    rx_skip(r, m);
                    continue;
                }
                if (!r.start && m == kChunk && rx_no_start_in(lo) && rx_no_start_in(hi)) {
                    rx_skip_idle(r, kChunk);
                    continue;
                }
#pragma unroll 1
                for (uint32_t i = 0; i < m;) {
                    if (const uint32_t left = rx_skippable(r)) {
                        const uint32_t take = min(left, m - i);
                        rx_skip(r, take);
                        i += take;
                        continue;
                    }
                    uint64_t t = 0;
                    uint32_t x = 0, y = 0, z = 0;
                    if (rx_byte(r, chunk_byte(lo, hi, i), t, x, y, z) && rx_take(r, count, M)) {
                        uint32_t *out = reinterpret_cast<uint32_t *>(a.samples + (((size_t)k * M + count) * S + s) * sizeof(aof_imu_sample));
                        out[0] = (uint32_t)t; out[1] = (uint32_t)(t >> 32);
                        out[2] = x; out[3] = y; out[4] = z; out[5] = 0u;
                        count++;
                    }
                    i++;
                }
            }
        }
        if (live) a.sample_count[o] = (uint8_t)count;
    }

    if (live) rx_store(*mem, r);
    // the outputs out to where a host reads them, before the launch counts as done
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

__global__ __launch_bounds__(256) void k_bank_mavlink_rx_reset(aof_mavlink_rx_state *state, const uint8_t *mask, uint32_t n)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n || (mask && !mask[s])) return;
    uint4 *p = reinterpret_cast<uint4 *>(state + s);
#pragma unroll
    for (uint32_t i = 0; i < sizeof(aof_mavlink_rx_state) / 16; i++) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace

int launch_bank_mavlink_rx(const MavlinkRxArgs &a, void *stream)
{
    if (a.n_streams < 1 || a.n_rounds < 1 || a.n_rounds > AOF_BANK_BURST_MAX || a.max_bytes < 16 ||
        a.max_bytes > AOF_MAVLINK_RX_BYTES_MAX || a.max_bytes % 16 || a.max_samples < 1 || a.max_samples > AOF_IMU_SLOTS_MAX ||
        !a.bytes || !a.state || !a.samples || !a.sample_count)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bank_mavlink_rx, dim3((a.n_streams + kWave - 1) / kWave), dim3(kWave), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

int launch_bank_mavlink_rx_reset(aof_mavlink_rx_state *state, const uint8_t *mask, uint32_t n_streams, void *stream)
{
    if (n_streams < 1 || !state) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bank_mavlink_rx_reset, dim3((n_streams + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), state,
                       mask, n_streams);
    return (int)hipGetLastError();
}

}  // namespace aof
