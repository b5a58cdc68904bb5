// The stream bank's MAVLink receive (include/aof.h, "the stream bank's MAVLink receive"), host side: the argument
// checks and the launches of k_bank_mavlink_rx.hip, and the same function as a plain loop on host memory.  The device
// calls know nothing about the bank: bytes and lengths in, a state array of the caller's, samples and counts out in the
// form aof_bank_imu_device takes.  Nothing here synchronises or allocates.
#include <cerrno>
#include <cstring>

#include "aof_bank_calls.hpp"
#include "aof_ctx.hpp"
#include "aof_host.hpp"
#include "aof_mavlink_rx_step.hpp"

using namespace aof;

namespace {

// nullptr, or what is wrong with the arguments both forms of the call share
const char *bad_call(const aof_mavlink_rx_params *rp, const void *bytes, const void *len, const void *states, const void *samples,
                     const void *sample_count)
{
    if (!rp || !bytes || !states || !samples || !sample_count) return "mavlink rx: null params, byte, state, sample or count pointer";
    if (rp->n_streams < 1) return "mavlink rx: n_streams < 1";
    if (rp->n_rounds < 1 || rp->n_rounds > AOF_BANK_BURST_MAX) return "mavlink rx: n_rounds outside 1..AOF_BANK_BURST_MAX";
    if (rp->max_bytes < 16 || rp->max_bytes > AOF_MAVLINK_RX_BYTES_MAX || rp->max_bytes % 16)
        return "mavlink rx: max_bytes outside 16..AOF_MAVLINK_RX_BYTES_MAX or no multiple of 16";
    if (rp->max_samples < 1 || rp->max_samples > AOF_IMU_SLOTS_MAX) return "mavlink rx: max_samples outside 1..AOF_IMU_SLOTS_MAX";
    if (!aligned(bytes, 16)) return "mavlink rx: the bytes must be 16-byte aligned";
    if (!aligned(states, 8) || !aligned(samples, 8)) return "mavlink rx: states and samples must be 8-byte aligned";
    if (!aligned(len, 2)) return "mavlink rx: the lengths must be 2-byte aligned";
    return nullptr;
}

}  // namespace

extern "C" {

int aof_bank_mavlink_rx_reset_device(aof_ctx *ctx, int32_t n_streams, const uint8_t *d_mask, aof_mavlink_rx_state *d_state,
                                     void *stream)
{
    if (!ctx) return -EINVAL;
    if (!d_state) return ctx_fail(ctx, -EINVAL, "mavlink rx reset: null state pointer");
    if (n_streams < 1) return ctx_fail(ctx, -EINVAL, "mavlink rx reset: n_streams < 1");
    if (!aligned(d_state, 8)) return ctx_fail(ctx, -EINVAL, "mavlink rx reset: the state must be 8-byte aligned");
    if (const int rc = precheck(ctx)) return rc;
    if (launch_bank_mavlink_rx_reset(d_state, d_mask, (uint32_t)n_streams, stream))
        return ctx_fail(ctx, -EIO, "mavlink rx reset launch failed");
    return 0;
}

int aof_bank_mavlink_rx_device(aof_ctx *ctx, const aof_mavlink_rx_params *rp, const uint8_t *d_bytes, const uint16_t *d_len,
                               aof_mavlink_rx_state *d_state, aof_imu_sample *d_samples, uint8_t *d_sample_count,
                               void *stream)
{
    if (!ctx) return -EINVAL;
    if (const char *what = bad_call(rp, d_bytes, d_len, d_state, d_samples, d_sample_count)) return ctx_fail(ctx, -EINVAL, what);
    if (const int rc = precheck(ctx)) return rc;

    MavlinkRxArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n_streams = (uint32_t)rp->n_streams;
    a.n_rounds = (uint32_t)rp->n_rounds;
    a.max_bytes = (uint32_t)rp->max_bytes;
    a.max_samples = (uint32_t)rp->max_samples;
    a.bytes = d_bytes;
    a.len = d_len;
    a.state = d_state;
    a.samples = reinterpret_cast<uint8_t *>(d_samples);
    a.sample_count = d_sample_count;
    if (launch_bank_mavlink_rx(a, stream)) return ctx_fail(ctx, -EIO, "mavlink rx launch failed");
    return 0;
}

int aof_bank_mavlink_rx_host(const aof_mavlink_rx_params *rp, const uint8_t *bytes, const uint16_t *len,
                             aof_mavlink_rx_state *states, aof_imu_sample *samples, uint8_t *sample_count)
{
    if (bad_call(rp, bytes, len, states, samples, sample_count)) return -EINVAL;
    const size_t S = (size_t)rp->n_streams, B = (size_t)rp->max_bytes, M = (size_t)rp->max_samples;
    for (size_t s = 0; s < S; s++) {
        MavRxBytes mem;
        std::memcpy(&mem, states + s, kRxLiveBytes);
        MavRx r;
        rx_load(r, mem);
        for (size_t k = 0; k < (size_t)rp->n_rounds; k++) {
            const size_t o = k * S + s;
            const uint8_t *p = bytes + o * B;
            size_t n = len ? len[o] : B;
            if (n > B) n = B;
            uint32_t count = 0;
            for (size_t i = 0; i < n;) {
                if (const uint32_t left = rx_skippable(r)) {
                    const uint32_t take = left < n - i ? left : (uint32_t)(n - i);
                    rx_skip(r, take);
                    i += take;
                    continue;
                }
                if (!r.start) {
                    size_t j = i;
                    while (j < n && p[j] != kRxStartV2 && p[j] != kRxStartV1) j++;
                    if (j > i) {
                        rx_skip_idle(r, (uint32_t)(j - i));
                        i = j;
                        continue;
                    }
                }
                uint64_t t = 0;
                uint32_t x = 0, y = 0, z = 0;
                if (rx_byte(r, p[i], t, x, y, z) && rx_take(r, count, (uint32_t)M)) {
                    aof_imu_sample &m = samples[(k * M + count) * S + s];
                    m.time_usec = t;
                    std::memcpy(&m.xgyro, &x, 4);
                    std::memcpy(&m.ygyro, &y, 4);
                    std::memcpy(&m.zgyro, &z, 4);
                    m.reserved = 0;
                    count++;
                }
                i++;
            }
            sample_count[o] = (uint8_t)count;
        }
        rx_store(mem, r);
        std::memcpy(states + s, &mem, kRxLiveBytes);
    }
    return 0;
}

}  // extern "C"
