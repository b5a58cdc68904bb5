// The stream bank's motion field (include/aof.h, "the stream bank's motion field"), the step both sides run on ONE stream
// and ONE tick: which streams have a frame, which ran a pair, what a pair adds to the window under way, and what a
// published tick takes out of it.  The kernel (k_bank_field.hip, lane 0 of a stream's group) and the host loop
// (aof_bank_field.cpp) compile this text; both are built with floating-point contraction off, and the functions that round
// say so themselves.  The fit of the pair itself is aof_field_step.hpp's.
#pragma once

#include <cstddef>
#include <cstdint>

#include "aof_field_step.hpp"
#include "aof_hd.hpp"
#include "aof_math.h"

namespace aof {

static_assert(sizeof(aof_bank_field_state) == 64 && alignof(aof_bank_field_state) == 8, "one field state is 64 bytes, 8-byte aligned");
static_assert(sizeof(aof_bank_field_record) == 48 && alignof(aof_bank_field_record) == 4, "one field record of a tick is 48 bytes");
static_assert(sizeof(aof_tick_record) == 48 && offsetof(aof_tick_record, frame) == 28 && offsetof(aof_tick_record, pixel) == 32,
              "a tick record is twelve words: quality, dt_us, ..., frame at 7, the pixel record from 8 on");

// What the step reads of a tick record.
struct BankFieldTick {
    int32_t quality, dt_us;
    uint32_t frame;
    int32_t pred_x, pred_y;    // r.pixel's predictor
};

// Rule 1: the stream was given no frame it could read; nothing about it changes.
AOF_HD_INLINE bool bank_field_no_frame(int32_t quality) { return quality == AOF_TICK_IDLE || quality == AOF_TICK_BAD_SENSOR; }
// Rule 2: the tick compared two frames of the stream (a first frame has nothing to compare with).
AOF_HD_INLINE bool bank_field_pair(const BankFieldTick &r) { return !bank_field_no_frame(r.quality) && r.frame >= 2u; }
// Rule 3: the limiter released the window, whether the IMU call then dropped the record or not.
AOF_HD_INLINE bool bank_field_published(int32_t quality)
{
    return quality >= 0 || quality == AOF_TICK_STALE_GYRO || quality == AOF_TICK_NO_OFFSET;
}

AOF_HD_INLINE aof_bank_field_record bank_field_record_zero(int32_t status)
{
    aof_bank_field_record o;
    o.status = status; o.dt_us = 0;
    o.zoom = o.rotation = o.centre_x = o.centre_y = o.flow_x = o.flow_y = 0.0f;
    o.pairs = o.fits = o.used = o.frame = 0u;
    return o;
}

// Rules 2 and 3 on a stream that has a frame (not rule 1).  f: the pair's fit, looked at only if `pair`.
AOF_HD_INLINE aof_bank_field_record bank_field_step(const BankFieldTick &r, bool pair, const aof_field &f, float focal_x, float focal_y,
                                                    aof_bank_field_state &st)
{
#pragma clang fp contract(off)
    if (pair) {
        st.pairs++;
        if (f.flags & AOF_FIELD_VALID) {
            st.fits++;
            st.used += f.used;
            st.sum_zoom += (double)f.zoom;
            st.sum_rotation += (double)f.rotation;
            st.sum_centre_x += (double)f.centre_x;
            st.sum_centre_y += (double)f.centre_y;
        }
    }
    aof_bank_field_record o = bank_field_record_zero(AOF_TICK_HELD);
    o.frame = r.frame;
    if (bank_field_published(r.quality)) {
        o.status = (int32_t)st.fits;
        o.dt_us = r.dt_us;
        o.zoom = (float)st.sum_zoom; o.rotation = (float)st.sum_rotation;
        o.centre_x = (float)st.sum_centre_x; o.centre_y = (float)st.sum_centre_y;
        o.flow_x = aof_atan2f(o.centre_x, focal_x);
        o.flow_y = aof_atan2f(o.centre_y, focal_y);
        o.pairs = st.pairs; o.fits = st.fits; o.used = st.used;
        st.sum_zoom = st.sum_rotation = st.sum_centre_x = st.sum_centre_y = 0.0;
        st.pairs = st.fits = st.used = 0u;
        st.published++;
    }
    return o;
}

// What one launch needs (k_bank_field.hip); by value.
struct BankFieldArgs {
    FieldGeom g;
    const uint32_t *blocks;            // [S][nb] the scratch region's level-0 records as words
    const uint8_t *subdirs;            // [S][nb], or nullptr without a sub-pixel context
    const uint32_t *records;           // aof_tick_record [S] as twelve words each
    aof_bank_field_state *state;       // [S], 8-byte aligned
    aof_field *fields;                 // [S], 8-byte aligned, or nullptr
    aof_bank_field_record *out;        // [S]
    const aof_bank_stream *streams;    // [S] the focal lengths of stream s (aof_set_bank_streams), or nullptr: the two below
    float focal_x, focal_y;
    int32_t n_streams;
    uint32_t div_nx_mul, div_nx_shift; // fastdiv_make(nx), filled by the launcher
};
int launch_bank_field(const BankFieldArgs &a, void *stream);   // hipError_t as int

}  // namespace aof
