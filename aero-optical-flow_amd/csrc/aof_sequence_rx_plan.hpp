// The plan of the sequence pipeline's MAVLink receive (aof_sequence_mavlink_rx_device, include/aof_sequence_mavlink_rx.h):
// the chunk size, the chunk count, the launch shapes and the scratch layout of a log of N bytes.  Host only and plain C++:
// the entry point sizes the scratch with it, the launcher takes its shapes and offsets from it, the kernels its constants,
// and tests/sequence_rx_ref.py restates it in Python.
#pragma once

#include <cstddef>
#include <cstdint>

namespace aof {

constexpr uint32_t kSeqRxChunk = 4096;        // C: log bytes per workgroup of the chunk, frame and pack passes
constexpr uint32_t kSeqRxFrameMax = 280;      // the longest frame: a signed MAVLink 2 frame of len 255
constexpr uint32_t kSeqRxLookahead = 288;     // bytes behind a chunk that are staged with it: a frame that starts in the chunk
                                              // lies in what is staged (>= kSeqRxFrameMax, a multiple of 16)
constexpr uint32_t kSeqRxTable = 288;         // u16 per chunk and table: entry offset 0 .. 279 -> entry offset of the next chunk
constexpr uint32_t kSeqRxEnd = 0xFFFFu;       // the END node: the frame N cuts; nothing behind it is reached
constexpr uint32_t kSeqRxThreads = 256;       // lanes per workgroup of the chunk, frame, scan, pack and sample-end passes
constexpr uint32_t kSeqRxEntryThreads = 320;  // of an entry round: a lane per table entry, five waves
constexpr uint32_t kSeqRxDoublings = 12;      // 2^12 hops leave a chunk whatever it holds
constexpr uint32_t kSeqRxChunkSamples = 512;  // samples whose frames start in one chunk: a frame is at least 8 bytes
constexpr uint32_t kSeqRxChunkStarts = 1408;  // reachable start bytes of one chunk: at most one in 3 bytes (1 366)
constexpr uint32_t kSeqRxLdsMax = 20 * 1024;  // static LDS of a workgroup at most (the frame pass: staged bytes, 16-bit pointers,
                                              // three masks, the start list): eight workgroups per CU fit
constexpr int kSeqRxScanLevels = 3;          // 256^3 chunk counts: more than 2^31 bytes hold
constexpr int64_t kSeqRxBytesMax = 0x7FFFFFFFll;
static_assert(kSeqRxLookahead >= kSeqRxFrameMax && kSeqRxLookahead % 16 == 0 && kSeqRxTable >= kSeqRxFrameMax, "a frame fits");
static_assert(2 * kSeqRxTable * 2 >= kSeqRxChunkSamples * 2, "the sample list of a chunk fits the two tables it takes over");

// the counters the frame pass adds up over the workgroups (u32 words at SeqRxPlan::words)
enum { kSeqRxFrames = 0, kSeqRxSamples = 1, kSeqRxBadCheck = 2, kSeqRxSkipped = 3, kSeqRxRejected = 4, kSeqRxWords = 8 };

struct SeqRxPlan {
    int64_t n_bytes;
    uint32_t chunks;                      // ceil(N / C): workgroups of the chunk, frame and pack passes; 0 for N == 0
    uint32_t rounds;                      // entry rounds, a launch each: the smallest R with 2^R >= chunks (0 for one chunk)
    int scan_levels;                      // levels of the scan over the chunks' sample counts (0 for N == 0)
    uint32_t scan_entries[kSeqRxScanLevels];   // level 0: chunks; level l + 1: one total per kSeqRxThreads entries of level l
    // scratch, byte offsets (each a multiple of 256)
    size_t words;                         // u32 [kSeqRxWords]
    size_t entry;                         // u16 [chunks]: where the chain enters chunk c, or END
    size_t count;                         // u32 [chunks]: samples whose frames start in chunk c
    size_t sums[kSeqRxScanLevels];        // u32 [scan_entries[l]]: the scan, in place
    size_t tables[2];                     // u16 [chunks][kSeqRxTable] each: the exit tables and their doublings
    size_t list;                          // u16 [chunks][kSeqRxChunkSamples]: = tables[0], which are dead behind the entry rounds
    size_t total_bytes;
};

inline size_t seq_rx_round256(size_t v) { return (v + 255u) / 256u * 256u; }

// false for an N the call refuses
inline bool seq_rx_plan(int64_t n_bytes, SeqRxPlan *out)
{
    if (n_bytes < 0 || n_bytes > kSeqRxBytesMax) return false;
    SeqRxPlan P = {};
    P.n_bytes = n_bytes;
    P.chunks = (uint32_t)((n_bytes + kSeqRxChunk - 1) / kSeqRxChunk);
    while ((1ull << P.rounds) < P.chunks) P.rounds++;
    for (uint32_t e = P.chunks; e > 0; e = (e + kSeqRxThreads - 1) / kSeqRxThreads) {
        P.scan_entries[P.scan_levels++] = e;
        if (e <= kSeqRxThreads || P.scan_levels == kSeqRxScanLevels) break;
    }
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += seq_rx_round256(bytes); return o; };
    P.words = take(kSeqRxWords * 4);
    P.entry = take((size_t)P.chunks * 2);
    P.count = take((size_t)P.chunks * 4);
    for (int l = 0; l < kSeqRxScanLevels; l++) P.sums[l] = take((size_t)P.scan_entries[l] * 4);
    for (int t = 0; t < 2; t++) P.tables[t] = take((size_t)P.chunks * kSeqRxTable * 2);
    P.list = P.tables[0];
    P.total_bytes = at;
    *out = P;
    return true;
}

}  // namespace aof
