// OPTICAL_FLOW_RAD on the device: the field mapping of mainloop.cpp:359-371 and the MAVLink 2 frame of
// mavlink_tcp.cpp:142-162 (facade/src/optical_flow_rad.cpp), one lane per message.  Shared by the sequence pipeline
// (k_sequence.hip) and the stream bank (k_bank.hip): both write the bytes fillOpticalFlowRad + packOpticalFlowRad do.
#pragma once

#include "aof_device.hpp"

namespace aof {

namespace {

__device__ __forceinline__ uint16_t crc_accumulate(uint8_t byte, uint16_t crc)
{
    uint8_t tmp = (uint8_t)(byte ^ (uint8_t)(crc & 0xFF));
    tmp = (uint8_t)(tmp ^ (uint8_t)(tmp << 4));
    return (uint16_t)((crc >> 8) ^ ((uint16_t)tmp << 8) ^ ((uint16_t)tmp << 3) ^ (tmp >> 4));
}

template <typename T> __device__ __forceinline__ void put(uint8_t *&p, T v)
{
    __builtin_memcpy(p, &v, sizeof(T));   // little-endian wire order = the device's own
    p += sizeof(T);
}

// Writes one frame (at most AOF_SEQ_FRAME_BYTES) to `out` and returns its length.  payload: kMavlinkPayloadBytes of the
// caller's (a lane's own array, or LDS where one lane of a workgroup packs: a kernel with dynamic LDS gets scratch
// memory for an array otherwise).  gx / gy / gz: the gyro sums
// before the axis switch (gyro axes are switched here to match pixel directions); wire order of OPTICAL_FLOW_RAD
// (message 106): by field size, then declaration.
constexpr int kMavlinkPayloadBytes = 44;
__device__ __forceinline__ int pack_optical_flow_rad(uint8_t *out, uint8_t *payload, uint64_t time_usec, int dt_us, float ang_x, float ang_y,
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
#pragma unroll
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
