/*
 * aof_sequence_field.h -- the sequence pipeline's motion field: a section of the C ABI (aof.h), which includes this file; do
 * not include it on its own.  Same conventions: plain C types, caller owns every buffer, 0 or a negative errno-style code.
 */
#ifndef AOF_SEQUENCE_FIELD_H
#define AOF_SEQUENCE_FIELD_H
#ifndef AOF_H
#error "include aof.h: aof_sequence_field.h is a section of it"
#endif

/* ---- the sequence pipeline's motion field: zoom, rotation and centre flow per published message of a whole recording ----
 * What aof_bank_field_device is for a bank of live streams, for ONE recorded stream of n frames: the fit of every pair
 * ("the motion FIELD of a batch", above) and its integration over the rate limiter's windows ("the stream bank's motion
 * field", aof_bank_field.h), one aof_bank_field_record per record of the sequence call.
 * The call is enqueued behind an aof_sequence_device call on the same stream and workspace: after it the level-0 block
 * records of every pair (and, with a sub-pixel context, the sub-directions) lie in the flow engine's workspace inside the
 * scratch region, each pair's predictor rides in flows[k].pred_x / pred_y, and records / count[0] hold the limiter's
 * publications.  The workspace is only read; no offset of aof_seq_layout moves and no new region is needed.  The call may
 * stand in front of aof_sequence_imu_device or behind it (that call rewrites quality and the gyro sums only; this one reads
 * frame and dt_us), and it serves a sequence call made with or without sp->derotate.
 * The rule (aof_sequence_field_host IS this loop; csrc/aof_bank_field_step.hpp is the one text of the step):
 *   1. M = min(count[0], n), F(m) = records[m].frame; pair k is frames (k, k + 1).
 *   2. fields[k] is byte for byte what aof_field_batch_device / aof_field_host give for pair k's level-0 blocks, its
 *      sub-directions (sub-pixel context only) and flows[k].pred_x / pred_y.
 *   3. From a zero aof_bank_field_state, for the frames j = 0 .. n-1 in order, the bank's step runs with pair = (j >= 1),
 *      f = fields[j-1], the focal lengths sp->focal_x / focal_y, and a tick that is published with record m's dt_us if
 *      j == F(m) and AOF_TICK_HELD otherwise.
 *   4. For a record frame, out[m] is the step's result with frame = F(m): the sequence's 0-based index (the bank's frame
 *      counter is one more).
 *   5. Every record of the list closes its window, whatever the IMU call made of its quality (AOF_TICK_STALE_GYRO,
 *      AOF_TICK_NO_OFFSET).
 *   6. *state_out is the state after frame n-1: the sums of the pairs behind the last record, published = M.
 * out[m] and the final state equal, `frame` aside, what a one-stream bank with aof_bank_field_device behind every push leaves
 * when the same frames are pushed one by one.
 * In closed form, which is what the kernels compute and is exact: window m is the pairs F(m-1) <= k < F(m) with F(-1) = 0
 * (record 0 is frame 0: an empty window); a window's four sums are the (double) casts of its valid fits' floats added in
 * pair order from 0.0 -- one lane walks one window, since floating-point addition is not associative.  The tail window of a
 * stalled recording (AOF_SEQ_STATUS_STALLED) is one lane walking up to n-1 pairs.
 * The device call cannot see count[0] or the records: its kernels clamp count[0] to n and every frame index into [0, n),
 * and treat F(m) <= F(m-1) (m >= 1) as an empty window; the outputs are then unspecified, every access stays inside the
 * arrays.
 * d_fields: [n-1], written, the per-pair fits; d_out: [n], the first count[0] written; d_state_out: one record or NULL.
 * Only enqueues (the fit's launch and one launch over the windows, on `stream`): no allocation, no host synchronisation,
 * capturable; no workgroup waits on another.  n_frames == 0: returns 0 with nothing enqueued; n_frames == 1: no fit launch,
 * record 0 and the state only.
 * -EINVAL with nothing enqueued and nothing written: NULL ctx, sp, fp, d_workspace or d_out; NULL d_fields with n_frames > 1;
 * everything aof_sequence_layout refuses; field parameters outside aof_field_batch_device's ranges; a geometry
 * aof_field_supported refuses; a workspace that is not 256-byte aligned; d_fields or d_state_out not 8-byte aligned; d_out
 * not 4-byte aligned.  -ENOSPC: a workspace smaller than aof_sequence_layout().total_bytes.  -EIO: the context's sticky
 * fault. */
int aof_sequence_field_device(aof_ctx *ctx, const aof_sequence_params *sp, const aof_field_params *fp, int64_t n_frames,
                              void *d_workspace, size_t workspace_bytes, aof_field *d_fields, aof_bank_field_record *d_out,
                              aof_bank_field_state *d_state_out, void *stream);
/* The same function on host memory, the plain sequential loop of the rule: no device, no context.  blocks: [n-1][nb0],
 * subdirs: [n-1][nb0] or NULL (looked at only with a sub-pixel configuration), flows: [n-1], as the workspace holds them;
 * records: the first n_records (= count[0]) records; fields: [n-1]; out: [n_records]; state_out: one record or NULL.
 * -EINVAL, nothing written: NULL p, sp or out; NULL blocks, flows or fields with n_frames > 1; NULL records with
 * n_records > 0; n_frames < 0 or >= 2^31 - 16; n_records > n_frames; focal lengths that are not > 0; field parameters or a
 * geometry as above; a record whose frame is >= n_frames or not above the frame of the record in front of it. */
int aof_sequence_field_host(const aof_params *p, const aof_sequence_params *sp, const aof_field_params *fp,
                            int64_t n_frames, const aof_block *blocks, const uint8_t *subdirs, const aof_flow *flows,
                            const aof_seq_record *records, uint32_t n_records, aof_field *fields,
                            aof_bank_field_record *out, aof_bank_field_state *state_out);

#endif
