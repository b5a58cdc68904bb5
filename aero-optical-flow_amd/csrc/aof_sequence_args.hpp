// The sequence pipeline's output kernel: its arguments and launcher (aof_sequence.cpp, k_sequence.hip).
#pragma once

#include <cstddef>
#include <cstdint>

#include "aof.h"

namespace aof {

// The output side of a frame sequence (k_sequence.hip): rate limiter, gyro sums, angles, OPTICAL_FLOW_RAD frames.
constexpr int64_t kLimitScanFrames = 4096;   // a publication must come within this many frames of the previous one
struct SequenceArgs {
    int64_t n_frames;
    const uint64_t *time_us;       // [n_frames] frame times relative to the first frame (mainloop.cpp:305-311)
    const aof_gyro *gyro;          // [n_frames] gyro integrated over the interval that ends at frame k, or nullptr
    const aof_flow *flows;         // [n_frames - 1]: pair k = frames k, k + 1
    int32_t output_rate;
    float period_us;               // limiter_period_us(output_rate)
    float focal_x, focal_y;
    uint64_t offset_timestamp_usec;
    uint8_t system_id, component_id, first_seq;
    uint32_t *jump[2], *hops[2];   // [n_frames + 1] each: pointer doubling, ping-pong
    uint8_t *reached;              // [n_frames + 1]: 0, or the round in which the node was marked + 1
    uint32_t *rank;                // [n_frames + 1]: position of a marked node on the chain = its message index
    uint32_t *count;               // [2]: records written, frames sent
    uint32_t *status;              // [1]: AOF_SEQ_STATUS_* flags (zeroed by the caller of the launcher)
    aof_seq_record *records;       // [n_frames]
    uint8_t *frames;               // [n_frames][AOF_SEQ_FRAME_BYTES], message m at + 56 m; or nullptr
    uint8_t *frame_len;            // [n_frames]
};
inline int sequence_rounds(int64_t n_frames)   // smallest R with 4^R > n_frames (the chain has at most that many hops)
{
    int r = 0;
    while ((1ll << (2 * r)) <= n_frames) r++;
    return r;
}
int launch_sequence_output(const SequenceArgs &a, void *stream);

// Where the limiter's four buffers lie inside aof_seq_layout.scratch: jump[0], jump[1], hops[0], hops[1], each (n_frames + 1)
// words in a slot of this many bytes, from offset 0.  (The sequence IMU call, aof_sequence_imu.cpp, keeps its scan there once
// k_sequence_emit has run.)
inline size_t limiter_slot_bytes(int64_t n_frames) { return (((size_t)n_frames + 1) * 4 + 255) / 256 * 256; }
// Behind them the limiter's rank ((n_frames + 1) words) and reached ((n_frames + 1) bytes), each rounded up to 256 bytes, then
// the flow engine's workspace for n_frames - 1 pairs (aof_workspace_layout), where a sequence call leaves every pair's level-0
// block records.  (The sequence field call, aof_sequence_field.cpp, reads them there.)
inline size_t limiter_rank_offset(int64_t n_frames) { return 4 * limiter_slot_bytes(n_frames); }
inline size_t limiter_reached_offset(int64_t n_frames) { return limiter_rank_offset(n_frames) + limiter_slot_bytes(n_frames); }
inline size_t sequence_flow_ws_offset(int64_t n_frames)
{
    return limiter_reached_offset(n_frames) + ((size_t)n_frames + 1 + 255) / 256 * 256;
}

}  // namespace aof
