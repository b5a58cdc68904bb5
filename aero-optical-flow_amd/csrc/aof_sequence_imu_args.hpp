// The sequence pipeline's IMU call: the arguments and the launcher of its kernels (aof_sequence_imu.cpp,
// k_sequence_imu.hip).
#pragma once

#include <cstdint>

#include "aof.h"

namespace aof {

constexpr uint32_t kSeqImuThreads = 256;   // lanes per workgroup of every kernel, and entries one workgroup scans

// Levels of the scan over the record pass's workgroup counts: level 0 has one count per workgroup of kSeqImuThreads
// records, level l + 1 one total per kSeqImuThreads entries of level l.  The top level is the first with at most
// kSeqImuThreads entries: one workgroup scans it.  Frame counts below 2^31 need at most three.
constexpr int kSeqImuLevels = 3;
inline int64_t seq_imu_groups(int64_t entries) { return (entries + kSeqImuThreads - 1) / kSeqImuThreads; }

struct SeqImuArgs {
    int64_t n_frames;              // n >= 1
    uint32_t n_samples;            // T
    uint64_t offset0;
    uint8_t system_id, component_id, first_seq;
    const uint64_t *time_us;       // [n]
    const uint8_t *samples;        // aof_imu_sample [T], or nullptr with T == 0
    const uint32_t *sample_end;    // [n]
    uint32_t *count;               // the workspace's count words: [0] records (read), [1] frames sent (written)
    aof_seq_record *records;       // [n]
    uint8_t *frames;               // [n][AOF_SEQ_FRAME_BYTES]
    uint8_t *frame_len;            // [n]
    aof_imu_state *state;          // one record, or nullptr
    // scratch (the limiter's jump / hops buffers, (n + 1) words each)
    uint32_t *sums[kSeqImuLevels]; // level l: seq_imu_groups^(l+1)(n + 1) words
    uint32_t *words;               // [kSeqImuWords]
};
// words[]: ~index of the first sample with a non-zero time (0: none; an atomic maximum), accepted and rejected samples
// of [0, E_last)
enum { kSeqImuFirst = 0, kSeqImuAccepted = 1, kSeqImuRejected = 2, kSeqImuWords = 4 };

int launch_sequence_imu(const SeqImuArgs &a, void *stream);

}  // namespace aof
