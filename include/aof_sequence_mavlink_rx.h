/*
 * aof_sequence_mavlink_rx.h -- the sequence pipeline's MAVLink receive: a section of the C ABI (aof.h), which includes this
 * file; do not include it on its own.  Same conventions: plain C types, caller owns every buffer, 0 or a negative
 * errno-style code.
 */
#ifndef AOF_SEQUENCE_MAVLINK_RX_H
#define AOF_SEQUENCE_MAVLINK_RX_H
#ifndef AOF_H
#error "include aof.h: aof_sequence_mavlink_rx.h is a section of it"
#endif

/* ---- the sequence pipeline's MAVLink receive: a recorded connection's bytes in, HIGHRES_IMU samples out ----
 * What aof_bank_mavlink_rx_device is for a bank of live connections, for ONE recorded connection of N bytes and a recording
 * of n frames: the call turns the log into exactly the two arrays aof_sequence_imu_device takes, aof_imu_sample [] and
 * sample_end u32 [n].  The wire rules are those of "the stream bank's MAVLink receive" above, word for word
 * (csrc/aof_mavlink_rx_step.hpp is the one text of the state machine; both sides of this call compile it).
 *   Order and counters.  The N bytes are taken in order from a reset state.  Sample j (0-based, in order of delivery) is
 *     written to samples[j] with reserved = 0 iff j < max_samples; later ones are lost and `overflowed` counts them.  So
 *     imu_samples - overflowed samples are written, and slots behind that are not written.  The cap is one for the whole
 *     log, not per round.
 *   Sample end.  byte_end[k] is the number of log bytes that had arrived before frame k's callback; it is clamped to N.
 *     sample_end[k] = min(max_samples, number of samples whose frame's last byte has index < byte_end[k]).  Each k is a
 *     function of its own byte_end[k] only: nothing requires the array to be monotone, and no value of it can take an
 *     access outside an array.  This is exactly what aof_sequence_imu_device takes as d_sample_end: called behind this
 *     call with ip->n_samples = max_samples it never reads an unwritten slot and needs no host round trip for the count.
 *   State out.  *state_out (or NULL) is all 128 bytes of the state the run ends in: the seven public counters, the frame
 *     in progress where N cuts one (the private layout of the bank's state), and zero in the reserved half.  It is byte
 *     for byte what a reset one-stream bank state holds after the same bytes, when no round overflowed.
 *   n_frames == 0 is allowed: no sample_end is written, d_byte_end and d_sample_end may be NULL; samples and state are
 *     still produced.
 *   n_bytes == 0 enqueues only the store of a reset state and of sample_end = 0.  Bytes behind N up to the next multiple
 *     of 16 may be loaded and are never interpreted.
 *   Scratch.  Caller-owned device memory of aof_sequence_mavlink_rx_scratch_bytes(n_bytes) bytes, 256-byte aligned; its
 *     contents afterwards are unspecified.  It is not the sequence workspace: the call may stand in front of
 *     aof_sequence_device or behind it.
 *   Execution.  Only enqueues: a fixed handful of launches on `stream` and one per doubling of the log's length in 4 096-byte
 *     chunks, no allocation, no host synchronisation, capturable; no workgroup waits on another.  It ends with a
 *     system-scope release behind its stores.
 * -EINVAL with nothing enqueued and nothing written: NULL ctx, rp, d_samples or d_scratch; NULL d_bytes with n_bytes > 0;
 * NULL d_byte_end or d_sample_end with n_frames > 0; n_bytes outside 0 .. 2^31 - 1, max_samples outside 1 .. 2^31 - 1,
 * n_frames outside 0 .. 2^31 - 17; d_bytes not 16-byte aligned; d_samples or d_state_out not 8-byte aligned; d_byte_end
 * or d_sample_end not 4-byte aligned; d_scratch not 256-byte aligned.  -ENOSPC: scratch_bytes smaller than
 * aof_sequence_mavlink_rx_scratch_bytes(n_bytes).  -EIO: the context's sticky fault. */
typedef struct aof_seq_rx_params {
    int64_t n_bytes;      /* N: 0 .. 2^31 - 1 */
    int64_t max_samples;  /* capacity of d_samples: 1 .. 2^31 - 1 */
} aof_seq_rx_params;

/* Bytes of scratch the device call needs for a log of n_bytes; 0 for an n_bytes the call refuses.  Host only. */
size_t aof_sequence_mavlink_rx_scratch_bytes(int64_t n_bytes);

int aof_sequence_mavlink_rx_device(aof_ctx *ctx, const aof_seq_rx_params *rp, int64_t n_frames,
                                   const uint8_t *d_bytes, const uint32_t *d_byte_end,
                                   aof_imu_sample *d_samples, uint32_t *d_sample_end, aof_mavlink_rx_state *d_state_out,
                                   void *d_scratch, size_t scratch_bytes, void *stream);
/* The same function on host memory, a plain sequential loop over the state machine and its bulk steps: no device, no
 * context.  -EINVAL, nothing written: NULL rp or samples; NULL bytes with n_bytes > 0; NULL byte_end or sample_end with
 * n_frames > 0; n_bytes, max_samples or n_frames outside the ranges above.  -ENOMEM, nothing written: no memory for the
 * delivery positions (one u32 per sample of the log). */
int aof_sequence_mavlink_rx_host(const aof_seq_rx_params *rp, int64_t n_frames, const uint8_t *bytes,
                                 const uint32_t *byte_end, aof_imu_sample *samples, uint32_t *sample_end,
                                 aof_mavlink_rx_state *state_out);

#endif
