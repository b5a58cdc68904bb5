// The stream bank's IMU (include/aof.h, "the stream bank's IMU"; mainloop.cpp:333-357 and 383-405), the ONE place its
// arithmetic and its gates are written: k_bank_imu.hip runs the two steps per lane, aof_bank_imu_host per element; the
// sequence pipeline's IMU call (k_sequence_imu.hip, aof_sequence_imu_host) runs the same two over a recording.
// IEEE double throughout, every operation rounded on its own: nothing is contracted into a multiply-add, on either
// side, and the division by 1e6 is a division.
#pragma once

#include "aof_hd.hpp"

namespace aof {

// One HIGHRES_IMU sample (time in microseconds, rates in rad/s) for the stream whose state is `st`.
AOF_HD_INLINE void imu_sample(aof_imu_state &st, uint64_t t, float x, float y, float z)
{
#pragma clang fp contract(off)
    const double dt = (double)(uint64_t)(t - st.prev_time_usec) / 1e6;   // (u64 wrap: time running backwards is a huge dt)
    const double ax = (double)__builtin_fabsf(x), ay = (double)__builtin_fabsf(y), az = (double)__builtin_fabsf(z);
    // (every comparison with a NaN is false: it is rejected)
    if (st.prev_time_usec != 0 && dt < 0.05 && ax < 20.0 && ay < 20.0 && az < 20.0) {
        st.gyro_x += (double)x * dt;
        st.gyro_y += (double)y * dt;
        st.gyro_z += (double)z * dt;
        st.samples_integrated += 1u;
    } else {
        st.samples_rejected += 1u;
    }
    st.prev_time_usec = t;
    if (st.offset_timestamp_usec == 0) st.offset_timestamp_usec = t;
}

// What the frame of a sent record carries beside the record's own fields.
struct ImuFrame {
    uint64_t time_usec;    // offset + the frame's time
    double gx, gy, gz;     // the gyro sums taken, before the axis switch
    uint8_t seq;
};

// The record of a frame with time `t` (what the push wrote, `rec`, completed in place).  Returns true where the record
// is sent: `f` then says what its frame carries, and the caller packs it.  A record with quality < 0 is left as it is.
// Record: the bank's aof_tick_record or the sequence pipeline's aof_seq_record -- the gate reads and writes `quality` and
// writes the three gyro floats, which both have.
template <typename Record>
AOF_HD_INLINE bool imu_take(aof_imu_state &st, Record &rec, uint64_t t, uint8_t first_seq, ImuFrame &f)
{
    if (rec.quality < 0) return false;   // held or idle: nothing is taken
    f.gx = st.gyro_x; f.gy = st.gyro_y; f.gz = st.gyro_z;
    st.gyro_x = 0.0; st.gyro_y = 0.0; st.gyro_z = 0.0;
    rec.gyro_x = (float)f.gx; rec.gyro_y = (float)f.gy; rec.gyro_z = (float)f.gz;
    if (st.last_taken_time_usec == st.prev_time_usec) {   // no sample since the previous take (mainloop.cpp:337-341)
        rec.quality = AOF_TICK_STALE_GYRO;
        st.dropped += 1u;
        return false;
    }
    st.last_taken_time_usec = st.prev_time_usec;
    if (st.offset_timestamp_usec == 0) {                  // no vehicle time yet (mainloop.cpp:353-357)
        rec.quality = AOF_TICK_NO_OFFSET;
        st.dropped += 1u;
        return false;
    }
    f.time_usec = st.offset_timestamp_usec + t;
    f.seq = (uint8_t)(first_seq + st.messages);
    st.messages += 1u;
    return true;
}

}  // namespace aof
