// OPTICAL_FLOW_RAD, the ONE place the library writes it: the field mapping of mainloop.cpp:359-371 and the MAVLink 2
// frame of mavlink_tcp.cpp:142-162, for the kernels (one lane per message: the sequence pipeline, k_sequence.hip and
// k_sequence_imu.hip; the stream bank, k_bank.hip, k_bank_burst.hip, k_bank_imu.hip) and for the host twins alike.  All of
// them write the bytes fillOpticalFlowRad + packOpticalFlowRad do.  Those (facade/src/optical_flow_rad.cpp) stay a
// second implementation on purpose: the facade is a library that sees only include/, and it is the independent packer
// the tests hold this one against.
#pragma once

#include "aof_hd.hpp"

namespace aof {

// The checksum's accumulate step (mavlinkCrcAccumulate) in TWO forms: on the wire's own widths for the packer, on
// 32-bit values for the receive's state machine (aof_mavlink_rx_step.hpp: its state lives in 32-bit registers).
// Neither is written through the other: either way the compiler emits other code for the kernels that use it (the
// packer's through a 32-bit step moves the bank's tick, commit, burst and IMU kernels; rx_crc through the 16-bit
// step moves k_bank_mavlink_rx).  tests/native/host_selftest.cpp holds them equal on all 65 536 x 256 inputs.
AOF_HD_INLINE uint32_t rx_crc(uint32_t byte, uint32_t crc)
{
    uint32_t tmp = (byte ^ crc) & 0xFFu;
    tmp = (tmp ^ (tmp << 4)) & 0xFFu;
    return ((crc >> 8) ^ (tmp << 8) ^ (tmp << 3) ^ (tmp >> 4)) & 0xFFFFu;
}

namespace {

AOF_HD_INLINE uint16_t crc_accumulate(uint8_t byte, uint16_t crc)
{
    uint8_t tmp = (uint8_t)(byte ^ (uint8_t)(crc & 0xFF));
    tmp = (uint8_t)(tmp ^ (uint8_t)(tmp << 4));
    return (uint16_t)((crc >> 8) ^ ((uint16_t)tmp << 8) ^ ((uint16_t)tmp << 3) ^ (tmp >> 4));
}

template <typename T> AOF_HD_INLINE void put(uint8_t *&p, T v)
{
    __builtin_memcpy(p, &v, sizeof(T));   // little-endian wire order = the device's own, and the hosts' this library builds for
    p += sizeof(T);
}

// Writes one frame (at most AOF_SEQ_FRAME_BYTES) to `out` and returns its length.  payload: kMavlinkPayloadBytes of the
// caller's (a lane's own array, or LDS where one lane of a workgroup packs: a kernel with dynamic LDS gets scratch
// memory for an array otherwise; a local array on the host).  gx / gy / gz: the gyro sums
// before the axis switch (gyro axes are switched here to match pixel directions); wire order of OPTICAL_FLOW_RAD
// (message 106): by field size, then declaration.
constexpr int kMavlinkPayloadBytes = 44;
AOF_HD_INLINE int pack_optical_flow_rad(uint8_t *out, uint8_t *payload, uint64_t time_usec, int dt_us, float ang_x, float ang_y,
                                        double gx, double gy, double gz, int quality, uint8_t seq,
                                        uint8_t system_id, uint8_t component_id)
{
    uint8_t *p = payload;
    put(p, time_usec);
    put(p, (uint32_t)dt_us);
    put(p, ang_x);
    put(p, ang_y);
    put(p, (float)(-gy));
    put(p, (float)gx);
    put(p, (float)gz);
    put(p, (uint32_t)0);        // time_delta_distance_us
    put(p, -1.0f);              // distance
    put(p, (int16_t)0);         // temperature
    put(p, (uint8_t)0);         // sensor_id
    put(p, (uint8_t)quality);
    int len = 44;
    while (len > 1 && payload[len - 1] == 0) len--;   // MAVLink 2 payload truncation
    uint8_t head[10] = {0xFD, (uint8_t)len, 0, 0, seq, system_id, component_id, 106, 0, 0};
    uint16_t crc = 0xFFFF;
#if defined(__clang__)
#pragma unroll
#endif
    for (int b = 0; b < 10; b++) {
        out[b] = head[b];
        if (b) crc = crc_accumulate(head[b], crc);
    }
    for (int b = 0; b < len; b++) {
        out[10 + b] = payload[b];
        crc = crc_accumulate(payload[b], crc);
    }
    crc = crc_accumulate(138, crc);   // CRC_EXTRA of OPTICAL_FLOW_RAD
    out[10 + len] = (uint8_t)(crc & 0xFF);
    out[11 + len] = (uint8_t)(crc >> 8);
    return 12 + len;
}

}  // namespace

}  // namespace aof
