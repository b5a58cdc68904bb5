// The sequence pipeline's MAVLink receive: the arguments and the launcher of its kernels (aof_sequence_mavlink_rx.cpp,
// k_sequence_mavlink_rx.hip).  The shapes and the scratch offsets behind the pointers: aof_sequence_rx_plan.hpp.
#pragma once

#include <cstdint>

#include "aof.h"
#include "aof_sequence_rx_plan.hpp"

namespace aof {

struct SeqRxArgs {
    uint32_t n_bytes;              // N
    uint32_t max_samples;          // >= 1
    uint32_t n_frames;             // n >= 0
    uint32_t chunks;               // ceil(N / C)
    const uint8_t *bytes;          // [N], 16-byte aligned; nullptr with N == 0
    const uint32_t *byte_end;      // [n], or nullptr with n == 0
    uint8_t *samples;              // aof_imu_sample [max_samples]
    uint32_t *sample_end;          // [n], or nullptr with n == 0
    aof_mavlink_rx_state *state;   // one record, or nullptr
    // scratch
    uint32_t *words;               // [kSeqRxWords]
    uint16_t *entry;               // [chunks]
    uint32_t *count;               // [chunks]
    uint32_t *sums[kSeqRxScanLevels];
    uint16_t *tables[2];           // [chunks][kSeqRxTable] each
    uint16_t *list;                // [chunks][kSeqRxChunkSamples]: start offsets behind the frame pass, delivery offsets behind the pack
};

int launch_sequence_mavlink_rx(const SeqRxArgs &a, const SeqRxPlan &plan, void *stream);

}  // namespace aof
