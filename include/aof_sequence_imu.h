/*
 * aof_sequence_imu.h -- the sequence pipeline's IMU: a section of the C ABI (aof.h), which includes this file; do not
 * include it on its own.  Same conventions: plain C types, caller owns every buffer, 0 or a negative errno-style code.
 */
#ifndef AOF_SEQUENCE_IMU_H
#define AOF_SEQUENCE_IMU_H
#ifndef AOF_H
#error "include aof.h: aof_sequence_imu.h is a section of it"
#endif

/* ---- the sequence pipeline's IMU: raw HIGHRES_IMU samples in, gyro sums and the send gates for a whole recording ----
 * What aof_bank_imu_device is for a bank of live streams, for ONE recorded stream of n frames and T samples: the gyro
 * integrator of highres_imu_msg_callback (mainloop.cpp:383-405) and the two gates behind calcFlow() (the stale-gyro drop,
 * mainloop.cpp:336-342; "no vehicle time yet", mainloop.cpp:353-357, with the offset the first sample sets,
 * mainloop.cpp:403-404).  The sample, take and frame rules are those of "the stream bank's IMU" above, word for word
 * (csrc/aof_imu_step.hpp is the one text both calls compile), started from a reset state with offset_timestamp_usec =
 * offset0.
 * The call is enqueued behind an aof_sequence_device call on the same stream and workspace that was made with d_gyro =
 * NULL and sp->offset_timestamp_usec = 0: that call wrote records only (zero gyro sums, frame_len 0).  This call completes
 * the workspace in place, for the first count[0] records.  With E(m) = min(T, d_sample_end[frame of record m]), E(-1) = 0:
 *   * the samples of [E(m-1), E(m)) are taken in order, then record m: gyro_x/y/z = (float) of the double sums (of dropped
 *     records too), quality kept or turned into AOF_TICK_STALE_GYRO / AOF_TICK_NO_OFFSET;
 *   * a sent record gets its OPTICAL_FLOW_RAD frame at frames + 56 m, with time_usec = offset + d_time_us[frame], the
 *     record's dt_us, flows and quality, the double sums and sequence number (uint8_t)(first_seq + records sent before
 *     it); frame_len[m] is the frame's length, 0 for a dropped record;
 *   * frame bytes behind a length and frames of length 0 are not written; of a record only quality and gyro_x/y/z are
 *     stored (frame, dt_us, flow_x/y are read);
 *   * count[1] becomes the number of frames sent.
 * *d_state_out (or NULL) is the aof_imu_state the run ends in after frame n-1 and samples [0, E_last), E_last = min(T,
 * d_sample_end[n-1]): the sums of the tail window, prev_time_usec, last_taken_time_usec, offset_timestamp_usec, messages,
 * samples_integrated, samples_rejected, dropped.
 * d_sample_end[k]: the number of samples that arrived before frame k's callback; non-decreasing.  The device call cannot see
 * the array: its kernels clamp every index into [0, T) and every frame index into [0, n), and treat E(m) < E(m-1) as an
 * empty window; the outputs are then unspecified, every access stays inside the arrays.  The same holds for records whose
 * quality is negative on entry (aof_sequence_device writes none) and for a second call behind one sequence call.
 * Scratch: the call keeps its per-workgroup counts and three words in the limiter's jump / hops buffers of the sequence
 * scratch, which are dead once aof_sequence_device's kernels have run; no offset of aof_seq_layout moves.
 * Only enqueues (a handful of launches on `stream`): no allocation, no host synchronisation, capturable.  n_frames == 0:
 * returns 0 with nothing enqueued, as aof_sequence_device does.
 * -EINVAL with nothing enqueued and nothing written: NULL ctx, sp, ip, d_time_us, d_sample_end or d_workspace; NULL
 * d_samples with n_samples > 0; n_samples < 0 or >= 2^32; everything aof_sequence_layout refuses; a workspace that is not
 * 256-byte aligned; sp->offset_timestamp_usec != 0 or sp->derotate set (de-rotation needs per-frame gyro in front of the
 * flow); d_samples, d_time_us or d_state_out not 8-byte aligned, d_sample_end not 4-byte aligned.  -ENOSPC: a workspace
 * smaller than aof_sequence_layout().total_bytes.  -EIO: the context's sticky fault. */
typedef struct aof_seq_imu_params {
    int64_t  n_samples;     /* T >= 0, < 2^32 */
    uint64_t offset0;       /* initial vehicle time; 0 = learnt from the first sample with a non-zero time */
    uint8_t  system_id, component_id, first_seq;
} aof_seq_imu_params;

int aof_sequence_imu_device(aof_ctx *ctx, const aof_sequence_params *sp, const aof_seq_imu_params *ip, int64_t n_frames,
                            const uint64_t *d_time_us, const aof_imu_sample *d_samples, const uint32_t *d_sample_end,
                            void *d_workspace, size_t workspace_bytes, aof_imu_state *d_state_out, void *stream);
/* The same function on host memory, a plain sequential loop: no device, no context.  records: [n], the first count[0]
 * completed in place; count: the workspace's four words (count[0] read, count[1] written); frames: u8 [n][56]; frame_len:
 * u8 [n]; state_out: one record or NULL.  -EINVAL: a NULL ip, time_us, sample_end, records, count, frames or frame_len;
 * NULL samples with n_samples > 0; n_samples outside its range; n_frames < 0 or >= 2^31 - 16; count[0] > n_frames; a
 * record whose frame is >= n_frames; a sample_end that decreases.  A refused call writes nothing. */
int aof_sequence_imu_host(const aof_seq_imu_params *ip, int64_t n_frames, const uint64_t *time_us,
                          const aof_imu_sample *samples, const uint32_t *sample_end, aof_seq_record *records,
                          uint32_t *count, uint8_t *frames, uint8_t *frame_len, aof_imu_state *state_out);

#endif
