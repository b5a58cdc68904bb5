// The calls around a push of the stream bank, each a kernel of its own with a lane or a tile per stream: the outbox,
// the auto-exposure controller, the IMU call and the MAVLink receive -- their arguments and launchers.
#pragma once

#include <cstdint>

#include "aof.h"

namespace aof {

// The outbox of a push (aof_bank_collect_device, aof_outbox.cpp, k_bank_outbox.hip): compaction of the published records
// and the due exposure records of n = K * S records into dense lists, and the tag behind them.
constexpr uint32_t kOutboxTile = 1024;   // consecutive records one workgroup owns
struct OutboxCounter {             // context-owned device memory, zero at rest (the kernel's last arriver zeroes it)
    uint32_t arrivals;             // workgroups that have finished their stores
    uint32_t pad;
    unsigned long long found;      // selected records of the workgroups that have arrived: messages | exposures << 32
};
struct OutboxArgs {
    uint32_t n, n_streams;         // records in all (K * S, < 2^31), records per round
    const uint8_t *records;        // aof_tick_record [n]
    const uint8_t *mavlink;        // [n][AOF_SEQ_FRAME_BYTES] or nullptr
    const uint8_t *mavlink_len;    // [n] or nullptr
    const uint8_t *exposure;       // aof_exposure_record [n] or nullptr
    const uint8_t *derotated;      // float [n][2] or nullptr
    uint32_t cap_messages, cap_exposures;
    uint8_t *outbox;               // header at 0
    uint8_t *messages, *exposures; // the two entry lists inside it
    unsigned long long tag;
    const unsigned long long *d_tag;   // or nullptr
    OutboxCounter *counter;
};
int launch_bank_outbox(const OutboxArgs &a, void *stream);
// The auto-exposure controller behind a camera push (aof_bank_exposure_control_device, aof_exposure.cpp,
// k_bank_exposure.hip): a lane per stream walks its K exposure records and steps the stream's state.
struct ExposureArgs {
    aof_exposure_control ec;
    uint32_t n_streams, n_rounds;      // S, K (1..AOF_BANK_BURST_MAX)
    const uint8_t *records;            // aof_exposure_record [K][S]
    aof_exposure_state *state;         // [S]
    aof_exposure_command *commands;    // [K][S]
};
int launch_bank_exposure(const ExposureArgs &a, void *stream);
int launch_bank_exposure_reset(aof_exposure_state *state, const uint8_t *mask, uint32_t n_streams, uint16_t exposure0,
                               uint8_t gain0, const uint16_t *d_exposure0, const uint8_t *d_gain0, void *stream);
// The IMU call behind a push (aof_bank_imu_device / aof_bank_imu_reset_device, aof_imu.cpp, k_bank_imu.hip): a lane per
// stream takes the stream's samples and completes its K records.
struct ImuArgs {
    uint32_t n_streams, n_rounds, max_samples;   // S, K (1..AOF_BANK_BURST_MAX), M (1..AOF_IMU_SLOTS_MAX)
    uint8_t system_id, component_id, first_seq;
    const aof_bank_stream *streams;    // [S] the identity of stream s in place of the triple above (aof_set_bank_streams), or nullptr
    const uint8_t *samples;            // aof_imu_sample [K][M][S]
    const uint8_t *sample_count;       // u8 [K][S] or nullptr (M everywhere)
    const uint64_t *time_us;           // [K][S]
    const uint8_t *records_in;         // aof_tick_record [K][S]
    uint8_t *records_out;              // [K][S]: records_in, or disjoint from it
    aof_imu_state *state;              // [S]
    uint8_t *mavlink, *mavlink_len;    // [K][S][AOF_SEQ_FRAME_BYTES], [K][S]; both nullptr, or neither
};
int launch_bank_imu(const ImuArgs &a, void *stream);
int launch_bank_imu_reset(aof_imu_state *state, const uint8_t *mask, uint32_t n_streams, uint64_t offset0, void *stream);
// The MAVLink receive in front of the IMU call (aof_bank_mavlink_rx_device / aof_bank_mavlink_rx_reset_device,
// aof_mavlink_rx.cpp, k_bank_mavlink_rx.hip): a lane per stream takes the stream's bytes and writes its samples.
struct MavlinkRxArgs {
    uint32_t n_streams, n_rounds, max_bytes, max_samples;   // S, K, B (16..4096, a multiple of 16), M
    const uint8_t *bytes;              // [K][S][B], 16-byte aligned
    const uint16_t *len;               // [K][S] or nullptr (B everywhere)
    aof_mavlink_rx_state *state;       // [S]
    uint8_t *samples;                  // aof_imu_sample [K][M][S]
    uint8_t *sample_count;             // [K][S]
};
int launch_bank_mavlink_rx(const MavlinkRxArgs &a, void *stream);
int launch_bank_mavlink_rx_reset(aof_mavlink_rx_state *state, const uint8_t *mask, uint32_t n_streams, void *stream);

}  // namespace aof
