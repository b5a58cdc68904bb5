// The outbox of a stream bank push (aof_bank_collect_device, include/aof.h "the stream bank's outbox"): the published
// records of a push's [K][S] outputs, and the exposure records that are due, compacted into two dense lists in the
// order of o = round * S + stream, with a tag behind them that a host may poll.  ONE launch, no device-side waiting:
//   * a workgroup owns kOutboxTile consecutive records.  The slot of its first selected record is the number of
//     selected records in front of its tile, and it counts them itself from the input (written by an earlier launch, so
//     visible): a strided pass over the quality words and the `due` words, one ballot per 64 records;
//   * inside the tile, wave ballots and a prefix over the (pass, wave) counts give every selected record its slot, and
//     the record's index goes to a list in LDS at that slot;
//   * the entries are then written slot by slot, a lane per 16 bytes: eight lanes build one message entry, four one
//     exposure entry, each fetching its own sixteen bytes of the sources, so a wave's store covers 1 KB of consecutive
//     outbox bytes.  Slots at or behind the capacity are not written;
//   * the only step between workgroups is the tag.  Every wave that stored runs a system-scope release fence and waits
//     for it, the workgroup meets at a barrier, and one lane adds the tile's counts and then itself to the context's
//     counter (agent-scope atomics, the arrival acquire-release).  Nobody waits: the workgroup whose arrival was the
//     last takes the counts out, leaves the counter zero for the next launch or replay, stores the header and, behind
//     another system-scope release, the tag.  The host is a reader that no agent-scope fence covers.
// Two instantiations: the sources 16- / 8-byte aligned (16-byte loads), or only as aligned as the push demands.
#include <hip/hip_runtime.h>

#include "aof_bank_calls.hpp"
#include "aof_host.hpp"

namespace aof {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPasses = (int)kOutboxTile / kThreads;
constexpr uint32_t kFrontTiles = 4;   // tiles per step of the counting pass in front of a tile: 16 loads per lane in flight
constexpr uint32_t kRecordBytes = sizeof(aof_tick_record), kExposureBytes = sizeof(aof_exposure_record);
constexpr uint32_t kEntryBytes = sizeof(aof_outbox_entry), kExposureEntryBytes = sizeof(aof_outbox_exposure);
static_assert(kRecordBytes == 48 && kExposureBytes == 48 && kEntryBytes == 128 && kExposureEntryBytes == 64 &&
              sizeof(aof_outbox_header) == 64, "outbox layout");
static_assert(kOutboxTile % kThreads == 0 && kOutboxTile <= 65536, "tile indices are u16");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// ALIGNED: p is 16-byte aligned; else 4-byte aligned
template <bool ALIGNED>
__device__ __forceinline__ u32x4 load16(const uint8_t *p)
{
    if (ALIGNED) return *reinterpret_cast<const u32x4 *>(p);
    const uint32_t *w = reinterpret_cast<const uint32_t *>(p);
    return u32x4{w[0], w[1], w[2], w[3]};
}
// ALIGNED: p is 8-byte aligned; else 4-byte aligned
template <bool ALIGNED>
__device__ __forceinline__ u32x2 load8(const uint8_t *p)
{
    if (ALIGNED) return *reinterpret_cast<const u32x2 *>(p);
    const uint32_t *w = reinterpret_cast<const uint32_t *>(p);
    return u32x2{w[0], w[1]};
}
// Bytes 8k .. 8k+7 of a MAVLink frame of `len` bytes, the bytes from `len` on zero.  ALIGNED: the frame is 8-byte aligned.
template <bool ALIGNED>
__device__ __forceinline__ u32x2 frame_word(const uint8_t *frame, uint32_t k, uint32_t len)
{
    if (len <= 8 * k) return u32x2{0u, 0u};
    const uint32_t keep = len - 8 * k;
    unsigned long long v;
    if (ALIGNED) {
        v = *reinterpret_cast<const unsigned long long *>(frame + 8 * k);
    } else {
        v = 0;
        for (uint32_t b = 0; b < 8; b++) v |= (unsigned long long)frame[8 * k + b] << (8 * b);
    }
    if (keep < 8) v &= (1ull << (8 * keep)) - 1ull;
    return u32x2{(uint32_t)v, (uint32_t)(v >> 32)};
}

// The 32-bit word that selects record o: the quality of a tick record (QUALITY), or the `due` word of an exposure record.
// ALIGNED: the 16 bytes around it in one load.
template <bool ALIGNED, bool QUALITY>
__device__ __forceinline__ uint32_t selection_word(const uint8_t *records, uint32_t o)
{
    const uint8_t *p = records + (size_t)o * 48u;
    if (ALIGNED) return QUALITY ? load16<true>(p).x : load16<true>(p + 32).w;
    return *reinterpret_cast<const uint32_t *>(p + (QUALITY ? 0 : 44));
}
// How many of the records o, o + kThreads, ... (N per lane) are selected, over the wave: all N loads in flight before
// the first ballot.  Wave-uniform.
template <bool ALIGNED, int N, bool QUALITY>
__device__ __forceinline__ uint32_t count_selected(const uint8_t *records, uint32_t o)
{
    uint32_t word[N];
#pragma unroll
    for (int i = 0; i < N; i++) word[i] = selection_word<ALIGNED, QUALITY>(records, o + (uint32_t)i * kThreads);
    uint32_t count = 0;
#pragma unroll
    for (int i = 0; i < N; i++) count += (uint32_t)__popcll(__ballot(QUALITY ? (int32_t)word[i] >= 0 : word[i] != 0u));
    return count;
}

template <bool ALIGNED>
__global__ __launch_bounds__(kThreads) void k_bank_outbox(OutboxArgs a)
{
    __shared__ uint32_t s_front[2][kWaves];              // selected records in front of the tile, per wave's share
    __shared__ uint32_t s_tile[2][kPasses * kWaves];     // selected records of the tile per (pass, wave)
    __shared__ uint16_t s_index[2][kOutboxTile];         // slot inside the tile -> record inside the tile
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const uint32_t start = blockIdx.x * kOutboxTile;

    // selected records in front of the tile (start is a multiple of the tile: both loops are uniform)
    uint32_t front_m = 0, front_e = 0;
    for (uint32_t t0 = 0; t0 < start;) {
        if (start - t0 >= kFrontTiles * kOutboxTile) {
            front_m += count_selected<ALIGNED, kFrontTiles * kPasses, true>(a.records, t0 + tid);
            t0 += kFrontTiles * kOutboxTile;
        } else {
            front_m += count_selected<ALIGNED, kPasses, true>(a.records, t0 + tid);
            t0 += kOutboxTile;
        }
    }
    if (a.exposure) {
        for (uint32_t t0 = 0; t0 < start;) {
            if (start - t0 >= kFrontTiles * kOutboxTile) {
                front_e += count_selected<ALIGNED, kFrontTiles * kPasses, false>(a.exposure, t0 + tid);
                t0 += kFrontTiles * kOutboxTile;
            } else {
                front_e += count_selected<ALIGNED, kPasses, false>(a.exposure, t0 + tid);
                t0 += kOutboxTile;
            }
        }
    }
    // the tile's own (records behind the end are loaded as the last record and not selected)
    unsigned long long sel_m[kPasses], sel_e[kPasses];
    {
        uint32_t word[kPasses];
#pragma unroll
        for (int p = 0; p < kPasses; p++)
            word[p] = selection_word<ALIGNED, true>(a.records, min(start + (uint32_t)p * kThreads + tid, a.n - 1u));
#pragma unroll
        for (int p = 0; p < kPasses; p++) sel_m[p] = __ballot(start + (uint32_t)p * kThreads + tid < a.n && (int32_t)word[p] >= 0);
#pragma unroll
        for (int p = 0; p < kPasses; p++) sel_e[p] = 0ull;
        if (a.exposure) {
#pragma unroll
            for (int p = 0; p < kPasses; p++)
                word[p] = selection_word<ALIGNED, false>(a.exposure, min(start + (uint32_t)p * kThreads + tid, a.n - 1u));
#pragma unroll
            for (int p = 0; p < kPasses; p++) sel_e[p] = __ballot(start + (uint32_t)p * kThreads + tid < a.n && word[p] != 0u);
        }
    }
    if ((tid & 63) == 0) {
        s_front[0][wave] = front_m;
        s_front[1][wave] = front_e;
#pragma unroll
        for (int p = 0; p < kPasses; p++) {
            s_tile[0][p * kWaves + wave] = (uint32_t)__popcll(sel_m[p]);
            s_tile[1][p * kWaves + wave] = (uint32_t)__popcll(sel_e[p]);
        }
    }
    __syncthreads();
    uint32_t base_m = 0, base_e = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
        base_m += s_front[0][w];
        base_e += s_front[1][w];
    }
    uint32_t tile_m = 0, tile_e = 0, off_m[kPasses], off_e[kPasses];
#pragma unroll
    for (int j = 0; j < kPasses * kWaves; j++) {
        if ((uint32_t)(j % kWaves) == wave) {
            off_m[j / kWaves] = tile_m;
            off_e[j / kWaves] = tile_e;
        }
        tile_m += s_tile[0][j];
        tile_e += s_tile[1][j];
    }
#pragma unroll
    for (int p = 0; p < kPasses; p++) {
        const uint32_t below_m = __builtin_amdgcn_mbcnt_hi((uint32_t)(sel_m[p] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)sel_m[p], 0u));
        const uint32_t below_e = __builtin_amdgcn_mbcnt_hi((uint32_t)(sel_e[p] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)sel_e[p], 0u));
        const uint32_t local = (uint32_t)p * kThreads + tid;
        if ((sel_m[p] >> (tid & 63)) & 1ull) s_index[0][off_m[p] + below_m] = (uint16_t)local;
        if ((sel_e[p] >> (tid & 63)) & 1ull) s_index[1][off_e[p] + below_e] = (uint16_t)local;
    }
    __syncthreads();

    // the tile's slots that the capacity still holds
    const uint32_t store_m = base_m >= a.cap_messages ? 0u : min(tile_m, a.cap_messages - base_m);
    const uint32_t store_e = base_e >= a.cap_exposures ? 0u : min(tile_e, a.cap_exposures - base_e);

    for (uint32_t w = tid; w < store_m * 8u; w += kThreads) {
        const uint32_t slot = w >> 3, c = w & 7u;
        const uint32_t o = start + s_index[0][slot];
        u32x4 v = {0u, 0u, 0u, 0u};
        if (c >= 4u && c < 7u) {
            v = load16<ALIGNED>(a.records + (size_t)o * kRecordBytes + 16u * (c - 4u));
        } else if (c == 7u) {
            if (a.derotated) {
                const u32x2 d = load8<ALIGNED>(a.derotated + (size_t)o * 8u);
                v.x = d.x; v.y = d.y;
            }
        } else {
            const uint32_t raw = (a.mavlink && a.mavlink_len) ? a.mavlink_len[o] : 0u;
            const uint32_t len = min(raw, (uint32_t)AOF_SEQ_FRAME_BYTES);
            const uint8_t *frame = a.mavlink + (size_t)o * AOF_SEQ_FRAME_BYTES;   // (not read with len == 0)
            if (c == 0u) {
                const uint32_t round = o / a.n_streams;
                const u32x2 f = frame_word<ALIGNED>(frame, 0u, len);
                v = u32x4{o - round * a.n_streams, round | raw << 16, f.x, f.y};
            } else {
                const u32x2 f = frame_word<ALIGNED>(frame, 2u * c - 1u, len), g = frame_word<ALIGNED>(frame, 2u * c, len);
                v = u32x4{f.x, f.y, g.x, g.y};
            }
        }
        *reinterpret_cast<u32x4 *>(a.messages + (size_t)(base_m + slot) * kEntryBytes + 16u * c) = v;
    }
    for (uint32_t w = tid; w < store_e * 4u; w += kThreads) {
        const uint32_t slot = w >> 2, c = w & 3u;
        const uint32_t o = start + s_index[1][slot];
        const uint8_t *rec = a.exposure + (size_t)o * kExposureBytes;
        u32x4 v;
        if (c == 0u) {
            const uint32_t round = o / a.n_streams;
            const u32x2 h = load8<ALIGNED>(rec);
            v = u32x4{o - round * a.n_streams, round, h.x, h.y};
        } else if (c == 3u) {
            const u32x2 h = load8<ALIGNED>(rec + 40);
            v = u32x4{h.x, h.y, 0u, 0u};
        } else {
            const u32x2 f = load8<ALIGNED>(rec + 16u * c - 8u), g = load8<ALIGNED>(rec + 16u * c);
            v = u32x4{f.x, f.y, g.x, g.y};
        }
        *reinterpret_cast<u32x4 *>(a.exposures + (size_t)(base_e + slot) * kExposureEntryBytes + 16u * c) = v;
    }

    // every wave that stored: its bytes out to where the host reads them, before the workgroup arrives
    if (wave * 64u < store_m * 8u || wave * 64u < store_e * 4u) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (tid != 0) return;
    if (tile_m | tile_e)
        __hip_atomic_fetch_add(&a.counter->found, (unsigned long long)tile_m | (unsigned long long)tile_e << 32, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t before = __hip_atomic_fetch_add(&a.counter->arrivals, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (before != gridDim.x - 1u) return;
    // the last arriver: the counter back to zero, the header, and behind everything the tag
    const unsigned long long found = __hip_atomic_exchange(&a.counter->found, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.counter->arrivals, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t found_m = (uint32_t)found, found_e = (uint32_t)(found >> 32);
    *reinterpret_cast<u32x2 *>(a.outbox + 8) = u32x2{min(found_m, a.cap_messages), found_m};
    *reinterpret_cast<u32x4 *>(a.outbox + 16) = u32x4{min(found_e, a.cap_exposures), found_e, 0u, 0u};
    *reinterpret_cast<u32x4 *>(a.outbox + 32) = u32x4{0u, 0u, 0u, 0u};
    *reinterpret_cast<u32x4 *>(a.outbox + 48) = u32x4{0u, 0u, 0u, 0u};
    const unsigned long long tag = a.d_tag ? *a.d_tag : a.tag;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(a.outbox), tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

int launch_bank_outbox(const OutboxArgs &a, void *stream)
{
    if (a.n < 1 || a.n_streams < 1 || !a.records || !a.outbox || !a.counter) return (int)hipErrorInvalidValue;
    const bool wide = aligned(a.records, 16) && aligned(a.exposure, 16) && aligned(a.mavlink, 8) && aligned(a.derotated, 8);
    const uint32_t tiles = (a.n + kOutboxTile - 1) / kOutboxTile;
    hipLaunchKernelGGL(wide ? k_bank_outbox<true> : k_bank_outbox<false>, dim3(tiles), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

}  // namespace aof
