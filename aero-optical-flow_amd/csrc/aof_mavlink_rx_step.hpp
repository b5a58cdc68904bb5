// The stream bank's MAVLink receive (include/aof.h, "the stream bank's MAVLink receive"), the ONE place its state
// machine is written: k_bank_mavlink_rx.hip runs it per lane, aof_bank_mavlink_rx_host per stream.  A stream's state
// is worked on as a MavRx (plain 32-bit fields: registers on the device); rx_load / rx_store are the only place the
// 96 private bytes of aof_mavlink_rx_state are laid out, so both sides agree on them byte for byte.
#pragma once

#include "aof_mavlink.hpp"   // rx_crc: the checksum step, beside the packer's

namespace aof {

constexpr uint32_t kRxStartV2 = 0xFD, kRxStartV1 = 0xFE, kRxHighresImu = 105, kRxHighresImuExtra = 93;

// aof_mavlink_rx_state as it lies in memory.  Behind the public 32 bytes: the frame being received, all zero when idle.
struct MavRxBytes {
    uint64_t bytes;
    uint32_t frames, imu_samples, bad_check, overflowed, skipped, rejected_flags;
    uint64_t time_usec;       // payload bytes 0..7 taken so far, the others zero
    uint32_t gyro[3];         // payload bytes 20..31 likewise: xgyro, ygyro, zgyro as they lie on the wire
    uint32_t msgid;           // the message id bytes taken so far
    uint16_t pos;             // bytes of the frame taken behind its start byte
    uint16_t crc;             // the checksum so far (header; payload too where the message is wanted)
    uint8_t start;            // 0 = idle, else the frame's start byte
    uint8_t len, incompat;    // the header's, once taken
    uint8_t check;            // behind the first check byte: 1 = it matched; behind the second: 1 = both did
    uint8_t reserved[64];     // never written: zero since the reset
};
static_assert(sizeof(MavRxBytes) == 128 && sizeof(aof_mavlink_rx_state) == 128 && offsetof(MavRxBytes, time_usec) == 32 &&
              offsetof(MavRxBytes, reserved) == 64 && offsetof(aof_mavlink_rx_state, in_progress) == 32,
              "the state is 128 bytes: 32 public, 32 of the frame in progress, 64 reserved");
constexpr uint32_t kRxLiveBytes = 64;   // what a call reads and writes of a state

struct MavRx {
    uint64_t bytes;
    uint32_t frames, imu_samples, bad_check, overflowed, skipped, rejected_flags;
    uint64_t time_usec;
    uint32_t gx, gy, gz, msgid, pos, crc, start, len, incompat, check;
};

AOF_HD_INLINE void rx_load(MavRx &r, const MavRxBytes &m)
{
    r.bytes = m.bytes; r.frames = m.frames; r.imu_samples = m.imu_samples; r.bad_check = m.bad_check;
    r.overflowed = m.overflowed; r.skipped = m.skipped; r.rejected_flags = m.rejected_flags;
    r.time_usec = m.time_usec; r.gx = m.gyro[0]; r.gy = m.gyro[1]; r.gz = m.gyro[2]; r.msgid = m.msgid;
    r.pos = m.pos; r.crc = m.crc; r.start = m.start; r.len = m.len; r.incompat = m.incompat; r.check = m.check;
}

// (the first kRxLiveBytes of `m` only)
AOF_HD_INLINE void rx_store(MavRxBytes &m, const MavRx &r)
{
    m.bytes = r.bytes; m.frames = r.frames; m.imu_samples = r.imu_samples; m.bad_check = r.bad_check;
    m.overflowed = r.overflowed; m.skipped = r.skipped; m.rejected_flags = r.rejected_flags;
    m.time_usec = r.time_usec; m.gyro[0] = r.gx; m.gyro[1] = r.gy; m.gyro[2] = r.gz; m.msgid = r.msgid;
    m.pos = (uint16_t)r.pos; m.crc = (uint16_t)r.crc; m.start = (uint8_t)r.start; m.len = (uint8_t)r.len;
    m.incompat = (uint8_t)r.incompat; m.check = (uint8_t)r.check;
}

AOF_HD_INLINE void rx_idle(MavRx &r)
{
    r.time_usec = 0;
    r.gx = r.gy = r.gz = r.msgid = r.pos = r.crc = r.start = r.len = r.incompat = r.check = 0;
}

AOF_HD_INLINE uint32_t rx_header_bytes(const MavRx &r) { return r.start == kRxStartV2 ? 9u : 5u; }

// bytes of the frame behind its start byte; valid once the header is in (pos >= rx_header_bytes)
AOF_HD_INLINE uint32_t rx_frame_bytes(const MavRx &r)
{
    return rx_header_bytes(r) + r.len + 2u + (r.start == kRxStartV2 && (r.incompat & 1u) ? 13u : 0u);
}

// One byte.  True where it was the last byte of a HIGHRES_IMU frame whose checksum matched: (t, x, y, z) is the sample
// (the float bits as they lay on the wire) and the caller hands it to rx_take.
AOF_HD_INLINE bool rx_byte(MavRx &r, uint32_t b, uint64_t &t, uint32_t &x, uint32_t &y, uint32_t &z)
{
    r.bytes += 1u;
    if (!r.start) {
        if (b == kRxStartV2 || b == kRxStartV1) {
            r.start = b;
            r.crc = 0xFFFFu;
        } else {
            r.skipped += 1u;
        }
        return false;
    }
    const uint32_t hdr = rx_header_bytes(r), p = r.pos;
    r.pos = p + 1u;
    if (p < hdr) {
        r.crc = rx_crc(b, r.crc);
        if (p == 0u) {
            r.len = b;
        } else if (r.start == kRxStartV2) {
            if (p == 1u) {
                r.incompat = b;
                if (b & ~1u) {            // a frame this parser cannot size: idle at once, the byte is not rescanned
                    r.rejected_flags += 1u;
                    rx_idle(r);
                }
            } else if (p >= 6u) {
                r.msgid |= b << (8u * (p - 6u));
            }
        } else if (p == 4u) {
            r.msgid = b;
        }
        return false;
    }
    const uint32_t q = p - hdr;
    if (q < r.len) {
        if (r.msgid == kRxHighresImu) {
            r.crc = rx_crc(b, r.crc);
            if (q < 8u) {
                r.time_usec |= (uint64_t)b << (8u * q);
            } else if (q >= 20u && q < 32u) {
                const uint32_t v = b << (8u * (q & 3u)), w = (q - 20u) >> 2;
                r.gx |= w == 0u ? v : 0u;
                r.gy |= w == 1u ? v : 0u;
                r.gz |= w == 2u ? v : 0u;
            }
        }
        return false;
    }
    // (a frame of another message leaves the state as rx_skip does: whichever way its bytes are taken, the state agrees)
    if (r.msgid == kRxHighresImu) {
        if (q == r.len) {                 // the first check byte: the low one
            r.crc = rx_crc(kRxHighresImuExtra, r.crc);
            r.check = b == (r.crc & 0xFFu) ? 1u : 0u;
        } else if (q == r.len + 1u) {
            r.check = r.check && b == (r.crc >> 8) ? 1u : 0u;
        }
    }
    if (r.pos < rx_frame_bytes(r)) return false;
    r.frames += 1u;
    bool sample = false;
    if (r.msgid == kRxHighresImu) {
        if (r.check) {
            r.imu_samples += 1u;
            t = r.time_usec; x = r.gx; y = r.gy; z = r.gz;
            sample = true;
        } else {
            r.bad_check += 1u;
        }
    }
    rx_idle(r);
    return sample;
}

// A sample rx_byte delivered, in a round that holds `count` samples of at most M: true where the caller writes it to
// slot `count` and raises the count.
AOF_HD_INLINE bool rx_take(MavRx &r, uint32_t count, uint32_t M)
{
    if (count < M) return true;
    r.overflowed += 1u;
    return false;
}

// The bulk steps.  rx_skippable: how many of the next bytes can be taken without looking at them -- what is left of a
// frame that is not HIGHRES_IMU once its header is in (payload, check and signature: consumed by length, never
// checked).  rx_skip takes n <= rx_skippable(r) of them.
AOF_HD_INLINE uint32_t rx_skippable(const MavRx &r)
{
    if (!r.start || r.pos < rx_header_bytes(r) || r.msgid == kRxHighresImu) return 0u;
    return rx_frame_bytes(r) - r.pos;
}

AOF_HD_INLINE void rx_skip(MavRx &r, uint32_t n)
{
    r.bytes += n;
    r.pos += n;
    if (r.pos == rx_frame_bytes(r)) {
        r.frames += 1u;
        rx_idle(r);
    }
}

// n bytes in idle, none of them a start byte
AOF_HD_INLINE void rx_skip_idle(MavRx &r, uint32_t n)
{
    r.bytes += n;
    r.skipped += n;
}

// true where none of the eight bytes of `w` can be a start byte (a conservative test: 0xFC..0xFF are candidates)
AOF_HD_INLINE bool rx_no_start_in(uint64_t w)
{
    const uint64_t k = 0xFCFCFCFCFCFCFCFCull, v = (w & k) ^ k;   // a zero byte where a candidate was
    return ((v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull) == 0u;
}

}  // namespace aof
