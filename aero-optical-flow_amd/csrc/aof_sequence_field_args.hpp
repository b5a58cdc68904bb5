// The sequence pipeline's motion field: the arguments and the launcher of its window pass (aof_sequence_field.cpp,
// k_sequence_field.hip), and the tick both sides hand the bank's step (aof_bank_field_step.hpp) for a frame of a recording.
#pragma once

#include <cstdint>

#include "aof_bank_field_step.hpp"

namespace aof {

constexpr uint32_t kSeqFieldThreads = 256;   // lanes per workgroup: a lane per record, and one for the tail window
inline int64_t seq_field_groups(int64_t n_frames) { return (n_frames + 1 + kSeqFieldThreads - 1) / kSeqFieldThreads; }

// The tick of frame `frame` of a recording: a record of the list is a publication whatever its quality has become (rule 5 of
// include/aof_sequence_field.h), every other frame is held.  (The predictor belongs to the fit, not to the step.)
AOF_HD_INLINE BankFieldTick seq_field_tick(bool record, uint32_t frame, int32_t dt_us)
{
    return BankFieldTick{record ? 0 : AOF_TICK_HELD, record ? dt_us : 0, frame, 0, 0};
}

struct SeqFieldArgs {
    int64_t n_frames;                  // n >= 1
    const uint32_t *count;             // the workspace's count words: [0] records (read)
    const aof_seq_record *records;     // [n] (frame and dt_us read)
    const aof_field *fields;           // [n - 1] the per-pair fits, 8-byte aligned; nullptr with n == 1
    aof_bank_field_record *out;        // [n], the first count[0] written
    aof_bank_field_state *state;       // one record, or nullptr
    float focal_x, focal_y;
};
int launch_sequence_field(const SeqFieldArgs &a, void *stream);   // hipError_t as int

}  // namespace aof
