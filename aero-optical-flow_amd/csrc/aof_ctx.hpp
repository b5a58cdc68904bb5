// The context behind the C ABI, its state grouped by owner (forgetting a group is one assignment), and the host
// helpers aof_capi.hip, aof_batch.cpp and aof_percall.cpp share.
#pragma once

#include <hip/hip_runtime.h>
#include <chrono>
#include "aof_bank_calls.hpp"    // OutboxCounter
#include "aof_bank_tables.hpp"   // BankCtx
#include "aof_batch_plan.hpp"    // BatchConfig, AdaptiveSearch
#include "aof_engine_args.hpp"   // SmallArgs, Tile16Verdicts
#include "aof_resident.hpp"      // ResidentBox

namespace aof {

// Per-call host paths (aof_flow_pair_host, aof_stream_push_host): made on first use (ensure_host_state).
struct HostState {
    bool ready;                 // everything below exists
    hipStream_t stream;
    uint8_t *d_frames[2];       // ping-pong: previous / current frame (streaming entry point)
    uint8_t *d_pair[2];         // scratch of the stateless two-frame entry point
    int cur_slot;               // slot holding the newest frame
    bool have_prev;
    aof_block *d_blocks; uint8_t *d_subdirs; aof_flow *d_flow;   // one pair's records
    void *d_ws; size_t ws_bytes;
    // streaming entry point as two captured hipGraphs (one per ping-pong slot):
    // H2D of the pinned frame -> kernels -> D2H of the 16-byte result, one launch per call
    uint8_t *h_frame;           // pinned staging copy of the caller's frame
    uint8_t *h_frames[2];       // small frames: pinned ping-pong frames the kernels read in place
    bool zero_copy;             // (no H2D copy: a 64x64 frame is 4 KB over PCIe)
    aof_flow *h_flow;           // pinned result
    uint32_t *h_tag;            // pinned (same allocation, its own cache line): the tag the next tagged record carries
    hipGraphExec_t push_graph[2];
    bool push_tagged[2];        // the slot's graph publishes a tagged record: the host polls for it, no stream wait
};

// Resident form of the per-call path (aof_set_stream_resident): one workgroup stays on the device and serves
// aof_stream_push_host through a mailbox in pinned memory.
struct Resident {
    bool on;
    bool lost;                  // a resident kernel did not leave when asked: nothing it may touch is ever freed
    bool deaf;                  // fault injection (aof_debug_resident_fault): the next instances ignore the stop bit
    double stop_wait_s;         // how long resident_stop waits for the exit flag (1 s; the fault injection shortens it)
    uint32_t seq;               // number of the last request posted (the per-call graph's tagged records count on)
    uint32_t frame_req[2];      // request at which pinned frame b was posted as the newest frame, 0 = written otherwise
    struct Kernel {             // what a running instance holds: abandoned as a whole when it does not leave
        ResidentBox *box;       // pinned, device-visible
        hipStream_t stream;     // its own stream (highest priority: its own pool of hardware queues)
        uint32_t launches;      // instances started on `box`
    } k;
};

// Reduction inside the flat lane8 search (no K3 launch).  Vote records per context (launches of more pairs keep K3):
// 2 048 finaliser waves are at most 256 per XCD -- half of an XCD's wave slots at the search kernel's occupancy -- so
// the search workgroups of ANOTHER context's launch always find room beside them: two in-launch reductions in flight
// cannot wait for each other (they could from 4 096 pairs on, until the deadline).
constexpr int64_t kVotePairs = 2048;
constexpr uint32_t kVoteStride = 128;            // words per record: 1 + 2 * 55 bins at the most (R = 13)
constexpr uint32_t kVoteDeadlineTicks = 5000000; // 50 ms of the 100 MHz counter (aof_set_vote_deadline_us)
struct InLaunchReduce {
    uint32_t *mem;              // the pairs' vote records, zero at rest
    int64_t pairs;              // records allocated
    uint32_t deadline_ticks;    // finaliser waves give up after this (100 MHz ticks)
    bool separate;              // aof_set_reduce_fusion(ctx, 0): always launch K3
    hipEvent_t done;            // recorded behind every eager launch that uses `mem`
    hipStream_t stream;         // stream of that launch
    bool used;
    bool captured;              // a captured graph holds an in-launch reduction: eager launches keep to K3
};

struct Profiling {
    bool on;
    uint32_t mask;
    hipEvent_t (*ev)[AOF_PROFILE_RING][2];  // [AOF_K_COUNT][ring][start,stop], created on demand
    int64_t count[AOF_K_COUNT];             // launches timed since profiling was switched on
};

constexpr double kDrainS = 2.0;   // bounded waits for a stream of this library's kernels (each runs microseconds to milliseconds)

// The C ABI must not leave the calling thread on another HIP device than it found it on.
struct DeviceGuard {
    int prev;
    explicit DeviceGuard(int device) : prev(-1)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) (void)hipSetDevice(device);
        else prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

int fail(aof_ctx *ctx, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));   // sets aof_last_error
double seconds_since(std::chrono::steady_clock::time_point t0);
hipError_t drain_bounded(hipStream_t s, double seconds);   // hipErrorNotReady: `s` did not drain within `seconds`
int wedge(aof_ctx *ctx, const char *what, hipError_t e);
int sticky_error(aof_ctx *ctx);
int device_check(aof_ctx *ctx);
// The one-launch small-pair plan (k_flow_small and its tagged and resident forms) of one pair in the per-call
// buffers, or false where the batch plan takes separate passes (aof_batch.cpp).
bool plan_small_pair(const aof_ctx *ctx, const uint8_t *prev, const uint8_t *cur, aof_flow *flow, SmallArgs *sm);
bool resident_stop(aof_ctx *ctx);   // (aof_percall.cpp)
void drop_push_graphs(aof_ctx *ctx);
void free_host_state(aof_ctx *ctx);

#define HIP_TRY(ctx, expr)                                                              \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail(ctx, -EIO, "%s: %s", #expr, hipGetErrorString(e_));             \
    } while (0)

}  // namespace aof

struct aof_ctx {
    aof::BatchConfig cfg;       // params, grids, CUs of `device`, search mode and the kernel-choice switches: what the batch plan reads
    int device;
    char err[256];
    aof::BankCtx bank;          // the stream bank's section: the path switch and what the aof_set_bank_* calls have bound (bank_ctx, aof_bank_tables.hpp)
    bool graph_disabled;        // per-call graphs switched off, or a capture failed once: stay on the plain path
    bool capturing;             // a per-call graph is being captured (no event timing)
    bool wedged;                // a bounded wait for the device ran out: every later call fails, destroy frees nothing
    // device -> host fault word (pinned, its own allocation): a kernel that gave up on a device-side wait
    // stores a non-zero code here; every entry point that enqueues work looks at it first
    uint32_t *h_fault;
    aof::HostState host;
    aof::Resident res;
    aof::InLaunchReduce votes;
    aof::OutboxCounter *outbox_counter;   // device memory, zero at rest: arrivals of aof_bank_collect_device's workgroups
    aof::AdaptiveSearch adapt;
    aof::Tile16Verdicts tile16_verdicts;   // test hook (aof_debug_tile16_verdicts): count 0 = the probe decides
    aof::Profiling prof;
    aof_stream_stats stats;     // aof_stream_get_stats
};
