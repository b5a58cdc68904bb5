// The sequence pipeline's IMU (include/aof_sequence_imu.h), host side: the argument checks and the launch of
// k_sequence_imu.hip behind a records-only aof_sequence_device call, and the same function as a plain SEQUENTIAL loop on
// host memory: one aof_imu_state walked sample by sample and record by record with the steps of aof_imu_step.hpp, as the
// stream bank's host function walks a stream.  The kernels restate that loop in parallel ("Sequence
// IMU"); this file does not.  Nothing here synchronises or allocates, and nothing includes the HIP runtime: the file also
// builds for a host-only test program.  Compiled with floating-point contraction off: every operation is rounded on its
// own, as in the kernel.
#include <cerrno>
#include <cstring>

#include "aof_host.hpp"
#include "aof_imu_step.hpp"
#include "aof_mavlink.hpp"
#include "aof_sequence_args.hpp"
#include "aof_sequence_imu_args.hpp"

using namespace aof;

namespace {

bool bad_sample_count(const aof_seq_imu_params *ip) { return ip->n_samples < 0 || ip->n_samples > 0xFFFFFFFFll; }

}  // namespace

extern "C" {

int aof_sequence_imu_device(aof_ctx *ctx, const aof_sequence_params *sp, const aof_seq_imu_params *ip, int64_t n_frames,
                            const uint64_t *d_time_us, const aof_imu_sample *d_samples, const uint32_t *d_sample_end,
                            void *d_workspace, size_t workspace_bytes, aof_imu_state *d_state_out, void *stream)
{
    if (!ctx) return -EINVAL;
    if (!sp || !ip || !d_time_us || !d_sample_end || !d_workspace)
        return ctx_fail(ctx, -EINVAL, "sequence imu: null sequence params, imu params, time, sample_end or workspace pointer");
    if (bad_sample_count(ip)) return ctx_fail(ctx, -EINVAL, "sequence imu: n_samples outside 0 .. 2^32 - 1");
    if (!d_samples && ip->n_samples > 0) return ctx_fail(ctx, -EINVAL, "sequence imu: null samples with n_samples > 0");
    if (sp->offset_timestamp_usec != 0 || sp->derotate)
        return ctx_fail(ctx, -EINVAL, "sequence imu: the sequence call in front is for records only (offset_timestamp_usec 0, no de-rotation)");
    aof_params p;
    int rc = aof_get_params(ctx, &p);
    if (rc) return rc;
    aof_seq_layout L;
    rc = aof_sequence_layout(&p, sp, n_frames, &L);
    if (rc) return ctx_fail(ctx, rc, "sequence imu: sequence parameters do not match the context (crop size, frame count)");
    if (!aligned(d_workspace, 256)) return ctx_fail(ctx, -EINVAL, "sequence imu: the workspace must be 256-byte aligned");
    if (!aligned(d_samples, 8) || !aligned(d_time_us, 8) || !aligned(d_state_out, 8) || !aligned(d_sample_end, 4))
        return ctx_fail(ctx, -EINVAL, "sequence imu: samples, times and state must be 8-byte aligned, sample_end 4-byte aligned");
    if (workspace_bytes < L.total_bytes) return ctx_fail(ctx, -ENOSPC, "sequence imu: workspace smaller than aof_sequence_layout().total_bytes");
    if ((rc = precheck(ctx))) return rc;
    if (n_frames == 0) return 0;

    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    SeqImuArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n_frames = n_frames;
    a.n_samples = (uint32_t)ip->n_samples;
    a.offset0 = ip->offset0;
    a.system_id = ip->system_id; a.component_id = ip->component_id; a.first_seq = ip->first_seq;
    a.time_us = d_time_us;
    a.samples = reinterpret_cast<const uint8_t *>(d_samples);
    a.sample_end = d_sample_end;
    a.count = reinterpret_cast<uint32_t *>(ws + L.count);
    a.records = reinterpret_cast<aof_seq_record *>(ws + L.records);
    a.frames = ws + L.frames;
    a.frame_len = ws + L.frame_len;
    a.state = d_state_out;
    // the limiter's jump[0], jump[1], hops[0] take the scan's three levels, hops[1] the words: level l has at most
    // (n + 1) / 256^(l+1) + 1 entries, a slot (n + 1) words rounded up to 256 bytes
    const size_t slot = limiter_slot_bytes(n_frames);
    for (int l = 0; l < kSeqImuLevels; l++) a.sums[l] = reinterpret_cast<uint32_t *>(ws + L.scratch + (size_t)l * slot);
    a.words = reinterpret_cast<uint32_t *>(ws + L.scratch + (size_t)kSeqImuLevels * slot);
    static_assert(kSeqImuWords * 4 <= 256, "the words fit the smallest slot");
    if (launch_sequence_imu(a, stream)) return ctx_fail(ctx, -EIO, "sequence imu launch failed");
    return 0;
}

int aof_sequence_imu_host(const aof_seq_imu_params *ip, int64_t n_frames, const uint64_t *time_us, const aof_imu_sample *samples,
                          const uint32_t *sample_end, aof_seq_record *records, uint32_t *count, uint8_t *frames, uint8_t *frame_len,
                          aof_imu_state *state_out)
{
    if (!ip || !time_us || !sample_end || !records || !count || !frames || !frame_len) return -EINVAL;
    if (bad_sample_count(ip) || (!samples && ip->n_samples > 0)) return -EINVAL;
    if (n_frames < 0 || n_frames >= 0x7FFFFFF0ll) return -EINVAL;
    if (n_frames == 0) return 0;
    const uint32_t T = (uint32_t)ip->n_samples, M = count[0];
    if ((int64_t)M > n_frames) return -EINVAL;
    for (int64_t k = 1; k < n_frames; k++)
        if (sample_end[k] < sample_end[k - 1]) return -EINVAL;
    for (uint32_t m = 0; m < M; m++)
        if ((int64_t)records[m].frame >= n_frames) return -EINVAL;

    aof_imu_state st;
    std::memset(&st, 0, sizeof(st));
    st.offset_timestamp_usec = ip->offset0;
    uint32_t next = 0;   // the first sample not yet taken
    auto take_samples_before = [&](uint32_t end) {
        if (end > T) end = T;
        for (; next < end; next++) imu_sample(st, samples[next].time_usec, samples[next].xgyro, samples[next].ygyro, samples[next].zgyro);
    };
    for (uint32_t m = 0; m < M; m++) {
        aof_seq_record &rec = records[m];
        take_samples_before(sample_end[rec.frame]);
        ImuFrame f;
        uint8_t len = 0, payload[kMavlinkPayloadBytes];
        if (imu_take(st, rec, time_us[rec.frame], ip->first_seq, f))
            len = (uint8_t)pack_optical_flow_rad(frames + (size_t)m * AOF_SEQ_FRAME_BYTES, payload, f.time_usec, rec.dt_us, rec.flow_x,
                                                 rec.flow_y, f.gx, f.gy, f.gz, rec.quality, f.seq, ip->system_id, ip->component_id);
        frame_len[m] = len;
    }
    take_samples_before(sample_end[n_frames - 1]);
    count[1] = st.messages;
    if (state_out) *state_out = st;
    return 0;
}

}  // extern "C"
