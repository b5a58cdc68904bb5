/*
 * aof_bank_field.h -- the stream bank's motion field: a section of the C ABI (aof.h), which includes this file; do not
 * include it on its own.  Same conventions: plain C types, caller owns every buffer, 0 or a negative errno-style code.
 */
#ifndef AOF_BANK_FIELD_H
#define AOF_BANK_FIELD_H
#ifndef AOF_H
#error "include aof.h: aof_bank_field.h is a section of it"
#endif

/* ---- the stream bank's motion field: zoom, rotation and centre flow per stream, integrated over the limiter's window ----
 * A call behind a push, like the exposure control and the IMU call: after every tick the level-0 block records (and, with
 * a sub-pixel context, the sub-directions) of stream s lie in the bank's scratch region -- the engine's workspace for S
 * pairs, at scratch + aof_workspace_layout(p, S).l0_blocks / .l0_subdirs, [s][nb0], on both bank paths --, and the pair's
 * predictor rides in aof_tick_record.pixel.  This call fits the motion field (above) to the streams that ran a pair in
 * the tick and integrates it, per stream, over the rate limiter's window: a 15 Hz consumer of 75 Hz cameras gets one field
 * per published message, as it gets one flow.  The state is caller-owned device memory beside the bank, one record per
 * stream; aof_bank_field_reset_device zeroes the masked records (d_mask: u8 [S] or NULL = all) and a new array must be
 * reset once.
 * The rule, per stream s, with r = d_records[s] (csrc/aof_bank_field_step.hpp is the one text the kernel and
 * aof_bank_field_host compile):
 *   1. NO FRAME.  r.quality is AOF_TICK_IDLE or AOF_TICK_BAD_SENSOR: d_fields[s] and d_out[s] are all zero except
 *      status = r.quality; the state is not written.
 *   2. PAIR.  The stream ran a pair iff it is not in case 1 and r.frame >= 2.  Then f is the aof_field of the stream's block
 *      records, its sub-directions (with a sub-pixel context) and r.pixel.pred_x / pred_y -- byte for byte what
 *      aof_field_host / aof_field_batch_device give for those inputs --, and pairs++.  If f.flags & AOF_FIELD_VALID:
 *      fits++, used += f.used, and sum_zoom, sum_rotation, sum_centre_x and sum_centre_y each add (double) of f's published
 *      float: one addition each, no contraction.  Without a pair f is all zero and nothing is added (the blocks are stale
 *      or belong to nobody: they are not read).
 *   3. PUBLISHED.  The tick is published iff r.quality >= 0, or r.quality is AOF_TICK_STALE_GYRO or AOF_TICK_NO_OFFSET
 *      (records the limiter released and aof_bank_imu_device then dropped: the window closed all the same, so the call
 *      may run in front of the IMU call or behind it).  The output record takes status = fits, dt_us = r.dt_us, the four
 *      (float) casts of the sums, flow_x = aof_flow_angle(centre_x, focal_x) and flow_y = aof_flow_angle(centre_y, focal_y)
 *      with the stream's focal lengths (record s of an array bound with aof_set_bank_streams, else bp's scalars), the
 *      window's counts and frame = r.frame; then the sums and the window's counts go to zero and published++.
 *      Otherwise status = AOF_TICK_HELD, frame = r.frame and the rest of the record is zero.  With output_rate <= 0 every
 *      pair tick is published and its window is that one pair: no branch says so.
 *   4. Zoom over a window is the SUM of the per-pair a's (and likewise rotation and the centre flow): the composition of
 *      small changes to first order, as limitRate() sums the flows of the frames it integrates.
 * The call only enqueues on `stream`: no allocation, no host synchronisation, capturable into a hipGraph.  The bank and the
 * tick records are only read.  It must follow the push on the same stream.  It serves TICKS -- plain, camera or warped: a
 * burst push leaves only its last round's block records in the scratch region.
 * d_bank: the pushed bank (bp, bank_bytes as for the push; a camera bank has the same scratch offset); d_fields: [S], the
 * tick's per-pair fits, or NULL; d_out: [S].
 * -EINVAL with nothing enqueued: NULL ctx, bp, fp, d_bank, d_records, d_state or d_out, n_streams < 1 (or bank parameters the
 * push refuses), field parameters outside aof_field_batch_device's ranges, a geometry aof_field_supported refuses, a bank
 * that is not 256-byte aligned, d_records or d_out not 4-byte aligned, d_state or d_fields not 8-byte aligned, a stream
 * table bound for another n_streams; -ENOSPC: a bank smaller than aof_bank_layout().total_bytes; -EIO: the context's sticky
 * fault. */
typedef struct aof_bank_field_state {   /* 64 bytes, 8-byte aligned, one per stream, caller-owned device memory */
    double sum_zoom, sum_rotation, sum_centre_x, sum_centre_y;   /* of the window under way */
    uint32_t pairs, fits, used, published;                        /* window: pairs seen, valid fits, sum of aof_field.used; messages so far */
    uint8_t reserved[16];                                         /* 0 */
} aof_bank_field_state;
typedef struct aof_bank_field_record {  /* 48 bytes, one per stream and tick */
    int32_t status;       /* >= 0: published, the number of valid fits in the window; AOF_TICK_HELD; AOF_TICK_IDLE; AOF_TICK_BAD_SENSOR */
    int32_t dt_us;        /* the tick record's, published records only */
    float zoom, rotation; /* (float) of the window's sums: relative scale change, radians */
    float centre_x, centre_y;   /* (float) of the sums: level-0 pixels at the frame centre */
    float flow_x, flow_y;       /* aof_flow_angle(centre_x, focal_x), (centre_y, focal_y): rad, the stream's focal lengths */
    uint32_t pairs, fits, used, frame;   /* window counts; frame = the tick record's */
} aof_bank_field_record;
int aof_bank_field_reset_device(aof_ctx *ctx, int32_t n_streams, const uint8_t *d_mask, aof_bank_field_state *d_state,
                                void *stream);
int aof_bank_field_device(aof_ctx *ctx, const aof_bank_params *bp, const aof_field_params *fp, const void *d_bank,
                          size_t bank_bytes, const aof_tick_record *d_records, aof_bank_field_state *d_state,
                          aof_field *d_fields, aof_bank_field_record *d_out, void *stream);
/* The same function on host memory, a plain loop: no device, no context.  blocks: [S][nb0], subdirs: [S][nb0] or NULL,
 * as the scratch region holds them; streams: [S] per-stream records or NULL (bp's focal lengths).  -EINVAL as above
 * (alignment, bank size and binding aside). */
int aof_bank_field_host(const aof_params *p, const aof_bank_params *bp, const aof_bank_stream *streams,
                        const aof_field_params *fp, const aof_block *blocks, const uint8_t *subdirs,
                        const aof_tick_record *records, aof_bank_field_state *state, aof_field *fields,
                        aof_bank_field_record *out);

#endif
