// The sequence pipeline's MAVLink receive (aof_sequence_mavlink_rx_device, include/aof_sequence_mavlink_rx.h): the receive
// state machine of aof_mavlink_rx_step.hpp over ONE recorded connection of N bytes.  The stream bank walks a stream serially,
// a lane per stream; a recording is one stream, so the serial run is restated in parallel ("Sequence
// MAVLink receive"; exact, not approximate).  In idle the machine's next idle position is a function of at most three bytes
// at the current one -- p + 1 for a byte that starts nothing, p + 3 for a MAVLink 2 start with an incompat flag the parser
// cannot size, else p + the frame's length, which its header states; checksums never move a frame's end -- so the frame
// starts are the positions reached from 0 along that successor, and a frame N cuts goes to an END node.  With C =
// kSeqRxChunk bytes per chunk (aof_sequence_rx_plan.hpp):
//   k_seq_rx_chunk       a workgroup per chunk: the chunk and its look-ahead into LDS, the successor of every position,
//                        pointer doubling on 16-bit offsets until every pointer has left the chunk; stores, for each entry
//                        offset 0 .. 287, the offset at which the chain enters the next chunk, or END;
//   k_seq_rx_entry       one launch per round k: table F(k+1)[c][o] = F(k)[c + 2^k][F(k)[c][o]], and every chunk c < 2^k
//                        hands entry[c + 2^k] = F(k)[c][entry[c]];
//   k_seq_rx_frames      a workgroup per chunk: the same doubling, now marking what is reached from entry[c]; a reached byte
//                        that starts nothing counts one `skipped`; the reached start bytes are gathered and each gets a lane
//                        that runs its frame from an idle MavRx (rx_byte, and rx_skip for what is not HIGHRES_IMU) out of
//                        LDS; the counters are summed per workgroup and added to the call's words; the lane whose frame N
//                        cuts stores the frame in progress; the start offsets of the frames that delivered a sample go to
//                        the chunk's list in position order, their number to count[c];
//   k_seq_rx_scan        exclusive scan of up to 256 counts per workgroup in place, its total to the next level; launched
//                        once per level (the sequence IMU call's scan);
//   k_seq_rx_pack        a workgroup per chunk with samples: a lane per sample runs its frame again (the state machine
//                        decodes, nothing of the payload's layout is written here), stores it at base + rank where that is
//                        below max_samples, and turns its list entry into the delivery offset;
//   k_seq_rx_sample_end  a lane per frame k: samples delivered at or before min(byte_end[k], N) = the scanned base of the
//                        two chunks a frame ending there can have started in + a binary search in the list of each;
//                        lane 0 of workgroup 0 finishes the counters of the state.
// No workgroup waits for another inside a launch: the order is the stream's.  Trip counts: the doubling rounds (at most 12),
// a frame's bytes (at most 280), the starts of a chunk over the lanes of a workgroup (at most 6), a binary search over 512.
// Every index read from device memory is clamped: entry offsets and table values below kSeqRxTable, list entries into the
// staged bytes, counts to kSeqRxChunkSamples, byte_end to N.
#include <hip/hip_runtime.h>

#include "aof_device.hpp"
#include "aof_mavlink_rx_step.hpp"
#include "aof_sequence_mavlink_rx_args.hpp"

namespace aof {

namespace {

constexpr uint32_t C = kSeqRxChunk, kThreads = kSeqRxThreads, kWaves = kThreads / 64, kPer = C / kThreads;
constexpr uint32_t kStaged = C + kSeqRxLookahead, kEnd = kSeqRxEnd;
static_assert(sizeof(aof_imu_sample) == 24, "a sample is three 8-byte words");
static_assert(kStaged % 16 == 0 && C % kThreads == 0 && kPer <= 32 && C / 32 == 2 * 64,
              "the chunk in 16-byte units, positions per lane and 32-bit mask words (two per lane of a wave)");

// The chunk's bytes and what is staged behind them: 16-byte loads of the units that begin in front of N, zero elsewhere.
__device__ __forceinline__ void stage_chunk(const SeqRxArgs &a, uint32_t base, uint8_t *s_bytes)
{
    for (uint32_t u = threadIdx.x; u < kStaged / 16; u += kThreads) {
        const uint64_t at = (uint64_t)base + u * 16u;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (at < a.n_bytes) v = *reinterpret_cast<const uint4 *>(a.bytes + at);
        *reinterpret_cast<uint4 *>(s_bytes + u * 16u) = v;
    }
}

// Where the idle machine is next after local position o of the chunk at `base` (o < C, base + o < N): a local offset
// (up to C + 279), or kEnd where N cuts the frame that starts here.
__device__ __forceinline__ uint32_t successor(const uint8_t *s_bytes, uint32_t o, uint32_t left /* N - (base + o) >= 1 */)
{
    const uint32_t b = s_bytes[o];
    if (b != kRxStartV2 && b != kRxStartV1) return o + 1u;
    if (left < 2u) return kEnd;
    MavRx r = {};
    r.start = b;
    r.len = s_bytes[o + 1u];
    if (b == kRxStartV2) {
        if (left < 3u) return kEnd;
        r.incompat = s_bytes[o + 2u];
        if (r.incompat & ~1u) return o + 3u;
    }
    const uint32_t whole = 1u + rx_frame_bytes(r);
    return whole <= left ? o + whole : kEnd;
}

__device__ __forceinline__ bool bit_of(const uint32_t *mask, uint32_t o) { return (mask[o >> 5] >> (o & 31u)) & 1u; }

// The successors of the chunk's positions into s_next, then pointer doubling until every pointer has left the chunk.
// MARK: s_mark holds the bit of the entry position on entry and of every position reached from it on return.
template <bool MARK>
__device__ __forceinline__ void follow_chunk(const uint8_t *s_bytes, uint16_t *s_next, uint32_t *s_mark, uint32_t base, uint32_t N)
{
    for (uint32_t i = 0; i < kPer; i++) {
        const uint32_t o = i * kThreads + threadIdx.x;
        // (positions at and behind N, in the last chunk: they leave at once, nothing is behind them)
        s_next[o] = (uint16_t)(base + o < N ? successor(s_bytes, o, N - (base + o)) : C);
    }
    __syncthreads();
    for (uint32_t round = 0; round < kSeqRxDoublings; round++) {
        uint32_t t[kPer], tt[kPer], reached = 0;
        int live = 0;
#pragma unroll
        for (uint32_t i = 0; i < kPer; i++) {
            const uint32_t o = i * kThreads + threadIdx.x;
            t[i] = s_next[o];
            tt[i] = t[i] < C ? s_next[t[i]] : t[i];
            live |= t[i] < C;
            if (MARK) reached |= (uint32_t)bit_of(s_mark, o) << i;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < kPer; i++) {
            if (t[i] >= C) continue;
            s_next[i * kThreads + threadIdx.x] = (uint16_t)tt[i];
            if (MARK && ((reached >> i) & 1u)) atomicOr(&s_mark[t[i] >> 5], 1u << (t[i] & 31u));
        }
        if (!__syncthreads_or(live)) break;
    }
}

// The frame that starts at local position o, from an idle machine, out of the staged bytes: ends where the machine is idle
// again or at `limit` (N as a local offset, inside what is staged).  True where it delivered a sample; `end`: the local
// offset behind the last byte taken; r.start != 0 on return: N cut the frame and r is the state in progress.
__device__ __forceinline__ bool run_frame(const uint8_t *s_bytes, uint32_t o, uint32_t limit, MavRx &r, uint64_t &t, uint32_t &x,
                                          uint32_t &y, uint32_t &z, uint32_t &end)
{
    bool sample = false;
    uint32_t i = o;
#pragma unroll 1
    while (i < limit) {
        if (const uint32_t left = rx_skippable(r)) {
            const uint32_t take = min(left, limit - i);
            rx_skip(r, take);
            i += take;
        } else {
            sample = rx_byte(r, s_bytes[i], t, x, y, z);
            i++;
        }
        if (!r.start) break;
    }
    end = i;
    return sample;
}

// N as a local offset of the chunk at `base`, inside what is staged
__device__ __forceinline__ uint32_t staged_limit(uint32_t base, uint32_t N) { return min(N - base, kStaged); }

__global__ __launch_bounds__(kThreads) void k_seq_rx_chunk(SeqRxArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_bytes[kStaged];
    __shared__ uint16_t s_next[C];
    const uint32_t c = blockIdx.x, base = c * C;
    if (c == 0) {   // what the later launches start from
        if (threadIdx.x < (uint32_t)kSeqRxWords) a.words[threadIdx.x] = 0u;
        if (threadIdx.x == 0) a.entry[0] = 0;
        if (a.state && threadIdx.x >= 8u && threadIdx.x < 32u) reinterpret_cast<uint32_t *>(a.state)[threadIdx.x] = 0u;
    }
    stage_chunk(a, base, s_bytes);
    __syncthreads();
    follow_chunk<false>(s_bytes, s_next, nullptr, base, a.n_bytes);
    uint16_t *table = a.tables[0] + (size_t)c * kSeqRxTable;
    for (uint32_t o = threadIdx.x; o < kSeqRxTable; o += kThreads) {
        const uint32_t v = s_next[o];
        table[o] = (uint16_t)(v == kEnd ? kEnd : min(v - C, kSeqRxTable - 1u));   // (v >= C: every pointer has left)
    }
}

__global__ __launch_bounds__(kSeqRxEntryThreads) void k_seq_rx_entry(SeqRxArgs a, uint32_t k, int compose)
{
    const uint32_t c = blockIdx.x, o = threadIdx.x, step = 1u << k;
    const uint16_t *src = a.tables[k & 1u];
    uint16_t *dst = a.tables[(k & 1u) ^ 1u];
    const bool ahead = c + step < a.chunks;
    if (compose && o < kSeqRxTable) {
        uint32_t v = src[(size_t)c * kSeqRxTable + o];
        if (ahead && v != kEnd) v = src[(size_t)(c + step) * kSeqRxTable + min(v, kSeqRxTable - 1u)];
        dst[(size_t)c * kSeqRxTable + o] = (uint16_t)v;
    }
    if (o == 0 && c < step && ahead) {
        const uint32_t e = a.entry[c];
        a.entry[c + step] = (uint16_t)(e == kEnd ? kEnd : src[(size_t)c * kSeqRxTable + min(e, kSeqRxTable - 1u)]);
    }
}

__global__ __launch_bounds__(kThreads) void k_seq_rx_frames(SeqRxArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_bytes[kStaged];
    __shared__ uint16_t s_next[C];
    __shared__ uint32_t s_mark[C / 32], s_sample[C / 32], s_before[C / 32];
    __shared__ uint16_t s_starts[kSeqRxChunkStarts];
    __shared__ uint32_t s_n, s_words[kSeqRxWords];
    const uint32_t c = blockIdx.x, base = c * C, N = a.n_bytes;
    const uint32_t here = min(N - base, C);   // positions of this chunk in front of N
    const uint32_t entry = a.entry[c];
    if (threadIdx.x < C / 32) {
        s_mark[threadIdx.x] = entry < here && (entry >> 5) == threadIdx.x ? 1u << (entry & 31u) : 0u;
        s_sample[threadIdx.x] = 0u;
    }
    if (threadIdx.x < (uint32_t)kSeqRxWords) s_words[threadIdx.x] = 0u;
    if (threadIdx.x == 0) s_n = 0u;
    stage_chunk(a, base, s_bytes);
    __syncthreads();
    follow_chunk<true>(s_bytes, s_next, s_mark, base, N);

    // reached bytes in front of N: a start byte is gathered, any other byte was skipped in idle
    uint32_t skipped = 0;
    for (uint32_t i = 0; i < kPer; i++) {
        const uint32_t o = i * kThreads + threadIdx.x;
        if (o >= here || !bit_of(s_mark, o)) continue;
        const uint32_t b = s_bytes[o];
        if (b == kRxStartV2 || b == kRxStartV1) {
            const uint32_t slot = atomicAdd(&s_n, 1u);
            if (slot < kSeqRxChunkStarts) s_starts[slot] = (uint16_t)o;
        } else {
            skipped++;
        }
    }
    __syncthreads();
    const uint32_t n_starts = min(s_n, kSeqRxChunkStarts), limit = staged_limit(base, N);
    uint32_t frames = 0, samples = 0, bad_check = 0, rejected = 0;
    for (uint32_t j = threadIdx.x; j < n_starts; j += kThreads) {
        const uint32_t o = s_starts[j];
        MavRx r = {};
        uint64_t t = 0;
        uint32_t x = 0, y = 0, z = 0, end = 0;
        if (run_frame(s_bytes, o, limit, r, t, x, y, z, end)) atomicOr(&s_sample[o >> 5], 1u << (o & 31u));
        frames += r.frames; samples += r.imu_samples; bad_check += r.bad_check; rejected += r.rejected_flags;
        // (the one frame N cuts, if any; its counter words are rewritten by the last launch)
        if (r.start && a.state) rx_store(*reinterpret_cast<MavRxBytes *>(a.state), r);
    }
    frames = wave_sum_u32(frames); samples = wave_sum_u32(samples); bad_check = wave_sum_u32(bad_check);
    rejected = wave_sum_u32(rejected); skipped = wave_sum_u32(skipped);
    if ((threadIdx.x & 63u) == 0u) {
        if (frames) atomicAdd(&s_words[kSeqRxFrames], frames);
        if (samples) atomicAdd(&s_words[kSeqRxSamples], samples);
        if (bad_check) atomicAdd(&s_words[kSeqRxBadCheck], bad_check);
        if (rejected) atomicAdd(&s_words[kSeqRxRejected], rejected);
        if (skipped) atomicAdd(&s_words[kSeqRxSkipped], skipped);
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)kSeqRxWords && s_words[threadIdx.x]) atomicAdd(&a.words[threadIdx.x], s_words[threadIdx.x]);

    // the rank of a sample among the chunk's: the sample bits in front of its own
    if (threadIdx.x < 64u) {
        const uint32_t w0 = (uint32_t)__popc(s_sample[2u * threadIdx.x]), w1 = (uint32_t)__popc(s_sample[2u * threadIdx.x + 1u]);
        uint32_t incl = w0 + w1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
            incl += threadIdx.x >= (uint32_t)d ? up : 0u;
        }
        s_before[2u * threadIdx.x] = incl - w0 - w1;
        s_before[2u * threadIdx.x + 1u] = incl - w1;
        if (threadIdx.x == 63u) {
            const uint32_t total = min(incl, kSeqRxChunkSamples);
            a.count[c] = total;
            a.sums[0][c] = total;
        }
    }
    __syncthreads();
    uint16_t *list = a.list + (size_t)c * kSeqRxChunkSamples;
    for (uint32_t i = 0; i < kPer; i++) {
        const uint32_t o = i * kThreads + threadIdx.x;
        if (!bit_of(s_sample, o)) continue;
        const uint32_t rank = s_before[o >> 5] + (uint32_t)__popc(s_sample[o >> 5] & ((1u << (o & 31u)) - 1u));
        if (rank < kSeqRxChunkSamples) list[rank] = (uint16_t)o;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
}

// level[i] becomes the sum of the entries in front of it inside its group of kThreads; the group's total goes to the next
// level (the top level's is not needed: the frame pass counted the samples).
__global__ __launch_bounds__(kThreads) void k_seq_rx_scan(SeqRxArgs a, int level, uint32_t entries, int top)
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
    for (uint32_t w = 0; w < kWaves; w++) {
        const uint32_t n = s_wave[w];
        before += w < wave ? n : 0u;
        total += n;
    }
    if (i < entries) v[i] = before + incl - mine;
    if (threadIdx.x == 0 && !top) a.sums[level + 1][blockIdx.x] = total;
}

// samples whose frames start in front of chunk c
__device__ __forceinline__ uint32_t samples_before_chunk(const SeqRxArgs &a, uint32_t c, int levels)
{
    uint32_t n = a.sums[0][c];
    if (levels > 1) n += a.sums[1][c >> 8];
    if (levels > 2) n += a.sums[2][c >> 16];
    return n;
}

__global__ __launch_bounds__(kThreads) void k_seq_rx_pack(SeqRxArgs a, int levels)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_bytes[kStaged];
    const uint32_t c = blockIdx.x, base = c * C, N = a.n_bytes;
    const uint32_t n = min(a.count[c], kSeqRxChunkSamples);
    if (n == 0) return;   // (the same in every lane)
    stage_chunk(a, base, s_bytes);
    __syncthreads();
    const uint32_t first = samples_before_chunk(a, c, levels), limit = staged_limit(base, N);
    uint16_t *list = a.list + (size_t)c * kSeqRxChunkSamples;
    for (uint32_t j = threadIdx.x; j < n; j += kThreads) {
        const uint32_t o = min((uint32_t)list[j], C - 1u);
        MavRx r = {};
        uint64_t t = 0;
        uint32_t x = 0, y = 0, z = 0, end = o;
        const bool sample = run_frame(s_bytes, o, limit, r, t, x, y, z, end);
        list[j] = (uint16_t)end;
        const uint64_t slot = (uint64_t)first + j;
        if (sample && slot < a.max_samples) {
            uint64_t *out = reinterpret_cast<uint64_t *>(a.samples + slot * sizeof(aof_imu_sample));
            out[0] = t;
            out[1] = (uint64_t)y << 32 | x;
            out[2] = z;   // (reserved = 0)
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
}

// entries of chunk c's list (delivery offsets, ascending) that are <= at
__device__ __forceinline__ uint32_t delivered_in_chunk(const SeqRxArgs &a, uint32_t c, uint32_t at)
{
    const uint16_t *list = a.list + (size_t)c * kSeqRxChunkSamples;
    uint32_t lo = 0, hi = min(a.count[c], kSeqRxChunkSamples);
    while (lo < hi) {   // (at most ten trips)
        const uint32_t mid = (lo + hi) >> 1;
        if (list[mid] <= at) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kThreads) void k_seq_rx_sample_end(SeqRxArgs a, int levels)
{
    const uint32_t N = a.n_bytes;
    const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k < a.n_frames) {
        uint32_t before = 0;
        if (a.chunks > 0) {
            // a frame that ends at or in front of q started in chunk q / C or the one in front of it, or is counted whole:
            // frames of earlier chunks end in front of q (they are shorter than a chunk), those of later ones behind it
            const uint32_t q = min(a.byte_end[k], N);
            const uint32_t c1 = min(q / C, a.chunks - 1u), c0 = c1 > 0 ? c1 - 1u : 0u;
            before = samples_before_chunk(a, c0, levels) + delivered_in_chunk(a, c0, q - c0 * C);
            if (c1 != c0) before += delivered_in_chunk(a, c1, q - c1 * C);
        }
        a.sample_end[k] = min(before, a.max_samples);
    }
    if (k == 0 && a.state) {
        // (with no byte there was no launch in front of this one: every counter is 0)
        const bool any = a.chunks > 0;
        const uint32_t total = any ? a.words[kSeqRxSamples] : 0u;
        MavRxBytes *m = reinterpret_cast<MavRxBytes *>(a.state);
        m->bytes = N;
        m->frames = any ? a.words[kSeqRxFrames] : 0u;
        m->imu_samples = total;
        m->bad_check = any ? a.words[kSeqRxBadCheck] : 0u;
        m->overflowed = total > a.max_samples ? total - a.max_samples : 0u;
        m->skipped = any ? a.words[kSeqRxSkipped] : 0u;
        m->rejected_flags = any ? a.words[kSeqRxRejected] : 0u;
        if (!any) {
            uint32_t *w = reinterpret_cast<uint32_t *>(a.state);
            for (uint32_t i = 8; i < 32u; i++) w[i] = 0u;
        }
    }
    // the outputs out to where a host reads them, before the launch counts as done
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
}

}  // namespace

int launch_sequence_mavlink_rx(const SeqRxArgs &a, const SeqRxPlan &plan, void *stream)
{
    if (plan.n_bytes != (int64_t)a.n_bytes || plan.chunks != a.chunks || a.max_samples < 1 || !a.samples || !a.words || !a.entry ||
        !a.count || !a.tables[0] || !a.tables[1] || !a.list || (!a.bytes && a.n_bytes > 0) ||
        ((!a.byte_end || !a.sample_end) && a.n_frames > 0) || a.n_frames >= 0x7FFFFFF0u)
        return (int)hipErrorInvalidValue;
    for (int l = 0; l < plan.scan_levels; l++)
        if (!a.sums[l]) return (int)hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 block(kThreads), chunks(a.chunks);
    if (a.chunks > 0) {
        hipLaunchKernelGGL(k_seq_rx_chunk, chunks, block, 0, s, a);
        for (uint32_t k = 0; k < plan.rounds; k++)   // (the last round hands entries only: nobody reads its tables)
            hipLaunchKernelGGL(k_seq_rx_entry, chunks, dim3(kSeqRxEntryThreads), 0, s, a, k, k + 1 < plan.rounds ? 1 : 0);
        hipLaunchKernelGGL(k_seq_rx_frames, chunks, block, 0, s, a);
        for (int l = 0; l < plan.scan_levels; l++)
            hipLaunchKernelGGL(k_seq_rx_scan, dim3((plan.scan_entries[l] + kThreads - 1) / kThreads), block, 0, s, a, l,
                               plan.scan_entries[l], l == plan.scan_levels - 1 ? 1 : 0);
        hipLaunchKernelGGL(k_seq_rx_pack, chunks, block, 0, s, a, plan.scan_levels);
    }
    const uint32_t frame_groups = (a.n_frames + kThreads - 1) / kThreads;
    if (frame_groups > 0 || a.state)
        hipLaunchKernelGGL(k_seq_rx_sample_end, dim3(frame_groups > 0 ? frame_groups : 1u), block, 0, s, a, plan.scan_levels);
    return (int)hipGetLastError();
}

}  // namespace aof
