// The sequence pipeline's MAVLink receive (include/aof_sequence_mavlink_rx.h), host side: the argument checks, the scratch
// size and the launch of k_sequence_mavlink_rx.hip, and the same function as a plain SEQUENTIAL loop on host memory: one
// MavRx walked over the log with rx_byte and its bulk steps (aof_mavlink_rx_step.hpp), as the stream bank's host function
// walks a stream, with one cap for the whole log and the delivery position of every sample.  The kernels restate that loop
// in parallel ("Sequence MAVLink receive"); this file does not.  Nothing here synchronises, and nothing
// includes the HIP runtime: the file also builds for a host-only test program.
#include <algorithm>
#include <cerrno>
#include <cstring>
#include <new>
#include <vector>

#include "aof_host.hpp"
#include "aof_mavlink_rx_step.hpp"
#include "aof_sequence_mavlink_rx_args.hpp"

using namespace aof;

namespace {

// nullptr, or what is wrong with the arguments both forms of the call share
const char *bad_call(const aof_seq_rx_params *rp, int64_t n_frames, const void *bytes, const void *byte_end, const void *samples,
                     const void *sample_end)
{
    if (!rp || !samples) return "sequence mavlink rx: null params or sample pointer";
    if (rp->n_bytes < 0 || rp->n_bytes > kSeqRxBytesMax) return "sequence mavlink rx: n_bytes outside 0 .. 2^31 - 1";
    if (rp->max_samples < 1 || rp->max_samples > 0x7FFFFFFFll) return "sequence mavlink rx: max_samples outside 1 .. 2^31 - 1";
    if (n_frames < 0 || n_frames >= 0x7FFFFFF0ll) return "sequence mavlink rx: n_frames outside 0 .. 2^31 - 17";
    if (!bytes && rp->n_bytes > 0) return "sequence mavlink rx: null bytes with n_bytes > 0";
    if ((!byte_end || !sample_end) && n_frames > 0) return "sequence mavlink rx: null byte_end or sample_end with n_frames > 0";
    return nullptr;
}

}  // namespace

extern "C" {

size_t aof_sequence_mavlink_rx_scratch_bytes(int64_t n_bytes)
{
    SeqRxPlan P;
    return seq_rx_plan(n_bytes, &P) ? P.total_bytes : 0;
}

int aof_sequence_mavlink_rx_device(aof_ctx *ctx, const aof_seq_rx_params *rp, int64_t n_frames, const uint8_t *d_bytes,
                                   const uint32_t *d_byte_end, aof_imu_sample *d_samples, uint32_t *d_sample_end,
                                   aof_mavlink_rx_state *d_state_out, void *d_scratch, size_t scratch_bytes, void *stream)
{
    if (!ctx) return -EINVAL;
    if (const char *what = bad_call(rp, n_frames, d_bytes, d_byte_end, d_samples, d_sample_end)) return ctx_fail(ctx, -EINVAL, what);
    if (!d_scratch) return ctx_fail(ctx, -EINVAL, "sequence mavlink rx: null scratch pointer");
    if (!aligned(d_bytes, 16)) return ctx_fail(ctx, -EINVAL, "sequence mavlink rx: the bytes must be 16-byte aligned");
    if (!aligned(d_samples, 8) || !aligned(d_state_out, 8))
        return ctx_fail(ctx, -EINVAL, "sequence mavlink rx: samples and state must be 8-byte aligned");
    if (!aligned(d_byte_end, 4) || !aligned(d_sample_end, 4))
        return ctx_fail(ctx, -EINVAL, "sequence mavlink rx: byte_end and sample_end must be 4-byte aligned");
    if (!aligned(d_scratch, 256)) return ctx_fail(ctx, -EINVAL, "sequence mavlink rx: the scratch must be 256-byte aligned");
    SeqRxPlan P;
    if (!seq_rx_plan(rp->n_bytes, &P)) return ctx_fail(ctx, -EINVAL, "sequence mavlink rx: n_bytes outside 0 .. 2^31 - 1");
    if (scratch_bytes < P.total_bytes)
        return ctx_fail(ctx, -ENOSPC, "sequence mavlink rx: scratch smaller than aof_sequence_mavlink_rx_scratch_bytes(n_bytes)");
    if (const int rc = precheck(ctx)) return rc;

    uint8_t *ws = static_cast<uint8_t *>(d_scratch);
    SeqRxArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n_bytes = (uint32_t)rp->n_bytes;
    a.max_samples = (uint32_t)rp->max_samples;
    a.n_frames = (uint32_t)n_frames;
    a.chunks = P.chunks;
    a.bytes = d_bytes;
    a.byte_end = d_byte_end;
    a.samples = reinterpret_cast<uint8_t *>(d_samples);
    a.sample_end = d_sample_end;
    a.state = d_state_out;
    a.words = reinterpret_cast<uint32_t *>(ws + P.words);
    a.entry = reinterpret_cast<uint16_t *>(ws + P.entry);
    a.count = reinterpret_cast<uint32_t *>(ws + P.count);
    for (int l = 0; l < kSeqRxScanLevels; l++) a.sums[l] = reinterpret_cast<uint32_t *>(ws + P.sums[l]);
    for (int t = 0; t < 2; t++) a.tables[t] = reinterpret_cast<uint16_t *>(ws + P.tables[t]);
    a.list = reinterpret_cast<uint16_t *>(ws + P.list);
    if (launch_sequence_mavlink_rx(a, P, stream)) return ctx_fail(ctx, -EIO, "sequence mavlink rx launch failed");
    return 0;
}

int aof_sequence_mavlink_rx_host(const aof_seq_rx_params *rp, int64_t n_frames, const uint8_t *bytes, const uint32_t *byte_end,
                                 aof_imu_sample *samples, uint32_t *sample_end, aof_mavlink_rx_state *state_out)
{
    if (bad_call(rp, n_frames, bytes, byte_end, samples, sample_end)) return -EINVAL;
    const size_t N = (size_t)rp->n_bytes;
    const uint32_t M = (uint32_t)rp->max_samples;

    // where every sample of the log is delivered (index of its frame's last byte + 1), in order.  A sample's frame is at
    // least 8 bytes: the one allocation, made before anything is written, holds them all.
    std::vector<uint32_t> delivered;
    try {
        delivered.reserve(N / 8 + 1);
    } catch (const std::bad_alloc &) {
        return -ENOMEM;
    }
    MavRx r;
    std::memset(&r, 0, sizeof(r));
    uint32_t count = 0;   // samples written
    for (size_t i = 0; i < N;) {
        if (const uint32_t left = rx_skippable(r)) {
            const uint32_t take = left < N - i ? left : (uint32_t)(N - i);
            rx_skip(r, take);
            i += take;
            continue;
        }
        if (!r.start) {
            size_t j = i;
            while (j < N && bytes[j] != kRxStartV2 && bytes[j] != kRxStartV1) j++;
            if (j > i) {
                rx_skip_idle(r, (uint32_t)(j - i));
                i = j;
                continue;
            }
        }
        uint64_t t = 0;
        uint32_t x = 0, y = 0, z = 0;
        const bool sample = rx_byte(r, bytes[i], t, x, y, z);
        i++;
        if (!sample) continue;
        delivered.push_back((uint32_t)i);
        if (rx_take(r, count, M)) {
            aof_imu_sample &m = samples[count];
            m.time_usec = t;
            std::memcpy(&m.xgyro, &x, 4);
            std::memcpy(&m.ygyro, &y, 4);
            std::memcpy(&m.zgyro, &z, 4);
            m.reserved = 0;
            count++;
        }
    }
    for (int64_t k = 0; k < n_frames; k++) {
        const uint32_t q = byte_end[k] < N ? byte_end[k] : (uint32_t)N;
        const size_t before = (size_t)(std::upper_bound(delivered.begin(), delivered.end(), q) - delivered.begin());
        sample_end[k] = before < M ? (uint32_t)before : M;
    }
    if (state_out) {
        MavRxBytes mem;
        std::memset(&mem, 0, sizeof(mem));
        rx_store(mem, r);
        std::memcpy(state_out, &mem, sizeof(mem));
    }
    return 0;
}

}  // extern "C"
