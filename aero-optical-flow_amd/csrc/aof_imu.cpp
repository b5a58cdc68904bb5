// The stream bank's IMU (include/aof.h, "the stream bank's IMU"), host side: the argument checks and the launches of
// k_bank_imu.hip behind a push, and the same function as a plain loop on host memory.  The device calls know nothing
// about the bank: they read the push's records and times, the caller's samples and a state array of the caller's.
// Nothing here synchronises or allocates.  This file is compiled with floating-point contraction off:
// aof_bank_imu_host rounds every operation on its own, as the kernel does.
#include <cerrno>
#include <cstring>

#include "aof_bank_calls.hpp"
#include "aof_bank_tables.hpp"
#include "aof_ctx.hpp"
#include "aof_host.hpp"
#include "aof_imu_step.hpp"
#include "aof_mavlink.hpp"

using namespace aof;

namespace {

// nullptr, or what is wrong with the arguments both forms of the call share
const char *bad_call(const aof_imu_params *ip, const void *samples, const void *time_us, const void *records_in, const void *states,
                     const void *records_out, const void *mavlink, const void *mavlink_len)
{
    if (!ip || !samples || !time_us || !records_in || !states || !records_out)
        return "imu: null params, sample, time, record or state pointer";
    if (ip->n_streams < 1) return "imu: n_streams < 1";
    if (ip->n_rounds < 1 || ip->n_rounds > AOF_BANK_BURST_MAX) return "imu: n_rounds outside 1..AOF_BANK_BURST_MAX";
    if (ip->max_samples < 1 || ip->max_samples > AOF_IMU_SLOTS_MAX) return "imu: max_samples outside 1..AOF_IMU_SLOTS_MAX";
    if (!mavlink != !mavlink_len) return "imu: frames and their lengths come together";
    if (!aligned(samples, 8) || !aligned(states, 8) || !aligned(time_us, 8))
        return "imu: samples, states and times must be 8-byte aligned";
    if (!aligned(records_in, 4) || !aligned(records_out, 4)) return "imu: records must be 4-byte aligned";
    return nullptr;
}

}  // namespace

extern "C" {

int aof_bank_imu_reset_device(aof_ctx *ctx, int32_t n_streams, const uint8_t *d_mask, uint64_t offset0,
                              aof_imu_state *d_state, void *stream)
{
    if (!ctx) return -EINVAL;
    if (!d_state) return ctx_fail(ctx, -EINVAL, "imu reset: null state pointer");
    if (n_streams < 1) return ctx_fail(ctx, -EINVAL, "imu reset: n_streams < 1");
    if (!aligned(d_state, 8)) return ctx_fail(ctx, -EINVAL, "imu reset: the state must be 8-byte aligned");
    if (const int rc = precheck(ctx)) return rc;
    if (launch_bank_imu_reset(d_state, d_mask, (uint32_t)n_streams, offset0, stream)) return ctx_fail(ctx, -EIO, "imu reset launch failed");
    return 0;
}

int aof_bank_imu_device(aof_ctx *ctx, const aof_imu_params *ip, const aof_imu_sample *d_samples,
                        const uint8_t *d_sample_count, const uint64_t *d_time_us, const aof_tick_record *d_records_in,
                        aof_imu_state *d_state, aof_tick_record *d_records_out, uint8_t *d_mavlink,
                        uint8_t *d_mavlink_len, void *stream)
{
    if (!ctx) return -EINVAL;
    if (const char *what = bad_call(ip, d_samples, d_time_us, d_records_in, d_state, d_records_out, d_mavlink, d_mavlink_len))
        return ctx_fail(ctx, -EINVAL, what);
    // a bound per-stream array (aof_set_bank_streams) gives every stream its own identity; it is for one stream count
    const aof_bank_stream *d_streams = nullptr;
    if (const char *what = bank_tables_for_imu(bank_ctx(ctx).tables, ip->n_streams, &d_streams)) return ctx_fail(ctx, -EINVAL, what);
    if (const int rc = precheck(ctx)) return rc;

    ImuArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n_streams = (uint32_t)ip->n_streams;
    a.n_rounds = (uint32_t)ip->n_rounds;
    a.max_samples = (uint32_t)ip->max_samples;
    a.system_id = ip->system_id;
    a.component_id = ip->component_id;
    a.first_seq = ip->first_seq;
    a.streams = d_streams;
    a.samples = reinterpret_cast<const uint8_t *>(d_samples);
    a.sample_count = d_sample_count;
    a.time_us = d_time_us;
    a.records_in = reinterpret_cast<const uint8_t *>(d_records_in);
    a.records_out = reinterpret_cast<uint8_t *>(d_records_out);
    a.state = d_state;
    a.mavlink = d_mavlink;
    a.mavlink_len = d_mavlink_len;
    if (launch_bank_imu(a, stream)) return ctx_fail(ctx, -EIO, "imu launch failed");
    return 0;
}

int aof_bank_imu_host(const aof_imu_params *ip, const aof_imu_sample *samples, const uint8_t *sample_count,
                      const uint64_t *time_us, const aof_tick_record *records_in, aof_imu_state *states,
                      aof_tick_record *records_out, uint8_t *mavlink, uint8_t *mavlink_len)
{
    if (bad_call(ip, samples, time_us, records_in, states, records_out, mavlink, mavlink_len)) return -EINVAL;
    const size_t S = (size_t)ip->n_streams, M = (size_t)ip->max_samples;
    for (size_t k = 0; k < (size_t)ip->n_rounds; k++) {
        for (size_t s = 0; s < S; s++) {
            const size_t o = k * S + s;
            aof_imu_state &st = states[s];
            size_t n = sample_count ? sample_count[o] : M;
            if (n > M) n = M;
            for (size_t j = 0; j < n; j++) {
                const aof_imu_sample &m = samples[(k * M + j) * S + s];
                imu_sample(st, m.time_usec, m.xgyro, m.ygyro, m.zgyro);
            }
            aof_tick_record rec = records_in[o];
            ImuFrame f;
            uint8_t len = 0, payload[kMavlinkPayloadBytes];
            if (imu_take(st, rec, time_us[o], ip->first_seq, f) && mavlink)
                len = (uint8_t)pack_optical_flow_rad(mavlink + o * AOF_SEQ_FRAME_BYTES, payload, f.time_usec, rec.dt_us, rec.flow_x,
                                                     rec.flow_y, f.gx, f.gy, f.gz, rec.quality, f.seq, ip->system_id, ip->component_id);
            records_out[o] = rec;
            if (mavlink_len) mavlink_len[o] = len;
        }
    }
    return 0;
}

}  // extern "C"
