// Internal declarations shared by the host side of the C ABI and the kernel
// launchers.  Not installed; the public surface is include/aof.h.
#pragma once

#include <cstddef>
#include <cstdint>

#include "aof.h"

#if defined(__HIPCC__)
#define AOF_HD __host__ __device__
#else
#define AOF_HD
#endif

namespace aof {

// n / d for n < 2^31 as (umulhi(n, mul) + n) >> shift (round-up method of Granlund & Montgomery;
// with n < 2^31 the sum cannot overflow 32 bits).  Filled on the host, used by the lane-per-block
// kernels, where a run-time integer division costs ~20 VALU instructions per lane.
struct FastDiv {
    uint32_t mul, shift;
};
inline FastDiv fastdiv_make(uint32_t d)
{
    FastDiv f = {0u, 0u};
    if (d == 0) return f;
    uint32_t l = 0;
    while ((1ull << l) < d) l++;
    f.mul = (uint32_t)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
    f.shift = l;
    return f;
}

// Is p a multiple of n bytes (nullptr is)?  The host-side test of every entry point and launcher; kernels test their own.
inline bool aligned(const void *p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

// The rate limiter's period in microseconds, 0 without a limit: the facade's own division, in float.
inline float limiter_period_us(int output_rate) { return output_rate > 0 ? 1.0e6f / (float)output_rate : 0.0f; }

struct Grid {
    int32_t x0, y0, step_x, step_y, nx, ny;
    AOF_HD int32_t blocks() const { return nx * ny; }
};

// Host-only parameter logic (aof_params.cpp).
int grid_for_level(const aof_params &p, int level, Grid *g);
int level_range(const aof_params &p, int level);  // histogram half-range R
int value_threshold_u16(const aof_params &p);     // SAD gate clamped to the u16 record
int reduce_chunks(int nblocks);                   // 0: one reduction workgroup per pair reads all records
size_t hist_bytes_per_pair(const aof_params &p, int level);  // vote-histogram scratch of one pair

// What turns a pair's vote histograms into its aof_flow (K3).
struct FlowTail {
    int32_t nblocks;
    int32_t range;             // R
    int32_t hist_filter;
    int32_t min_valid;
    aof_flow *flows;           // [n_pairs]
    const aof_flow *pred;      // copy pred_x/pred_y + PRED_VALID from here (level 0 of two), or nullptr
    int32_t emit_predictor;    // level 1: write the integer predictor into pred_x/pred_y
};

// The context's vote memory (zero at rest): one record per pair of the running launch -- word 0 the
// number of blocks that have arrived, then the two vote histograms (aof_reduce.hpp).
struct VoteMem {
    uint32_t *base;     // [pairs][stride] words
    uint32_t stride;    // words per pair, a multiple of 64 (256 bytes: pairs never share a line)
    uint32_t *fault;    // pinned host word of the context: a finaliser that gives up stores pair + 1 here
    uint32_t deadline_ticks;   // finaliser waves give up after this many ticks of the 100 MHz counter
};

// What the pruned lane8 search tells the host about itself (the ADAPTIVE mode of 8x8 contexts, choose_lane8 in aof_batch_plan.hpp):
// one workgroup in `stride` stores how many of its first wave's chunks left with "pruning pays" into a word of
// pinned host memory: tag (low 16 bits of launch_no) << 16 | paying << 8 | chunks.  Plain stores, nobody waits
// for them: the host reads whatever has arrived when it enqueues the next launch.  Speed only, never results.
constexpr int kPruneSlots = 256;
struct PruneReport {
    uint32_t *slots;      // pinned, kPruneSlots words; nullptr = no report
    uint32_t launch_no;
    uint32_t stride;      // (filled by the launcher)
    uint32_t expected;    // slots this launch writes (filled by the launcher)
};

// Everything one search launch needs; passed to the kernels by value.
struct SearchArgs {
    const uint8_t *prev;       // level frames of the older image, pair i at +i*stride
    const uint8_t *cur;        // level frames of the newer image
    int64_t pair_stride;       // bytes between consecutive pairs (both arrays)
    int32_t w, h;              // level frame size, row stride == w
    int32_t tile, search;      // B, S
    Grid grid;
    int32_t feature_threshold;
    int32_t value_threshold;   // clamped to <= 0xFFFF
    int32_t subpixel;
    aof_block *blocks;         // [n_pairs][grid.blocks()]
    uint8_t *subdirs;          // [n_pairs][grid.blocks()] or nullptr
    const aof_flow *pred;      // [n_pairs] level-1 results carrying the predictor, or nullptr
    const uint32_t *sums;      // [n_pairs][2][2] pixel sums, or nullptr when not equalising
    int32_t level;             // which sums column to use
    int64_t n_pairs;
    int32_t hist_range;        // R
    int32_t prune;             // 0 exhaustive, 1 exact partial-distortion elimination (lane8, tile16), 2 adaptive (tile16: per pair, by hints; lane8: the first chunk of a wave runs exhaustively and judges)
    uint32_t *hints;           // tile16, adaptive: [n_pairs] written by its probe kernel (1 = pruning pays), workspace
    FastDiv div_nb, div_nx;    // lane8: filled by its launchers (item -> pair, block -> row)
};

struct ReduceArgs {
    const aof_block *blocks;
    const uint8_t *subdirs;    // nullptr when half-pixel refinement is off
    int32_t value_threshold;
    FlowTail tail;
    int64_t n_pairs;
    const uint32_t *parts;     // per-chunk histograms of the first step of a two-step reduction (then blocks are not read)
    int32_t nstrips;           // chunks per pair
    uint32_t *chunk_parts;     // large grids: scratch for per-chunk histograms ([n_pairs][chunks][2][bins]), or nullptr
};

// The fused coarse kernel (k_coarse): K1 + level-1 search + level-1 reduction of one pair per
// workgroup, level-1 frames in LDS.
struct CoarseArgs {
    const uint8_t *prev, *cur; // level-0 frames
    int64_t pair_stride;
    int32_t w, h;              // level-0 frame size
    int32_t tile, search, subpixel;
    Grid grid;                 // level-1 block grid
    int32_t feature_threshold;
    int32_t value_threshold;   // clamped to <= 0xFFFF
    uint32_t *sums;            // [n_pairs][2][2] written here (no memset, no atomics), or nullptr
    aof_block *blocks;         // level-1 records [n_pairs][grid.blocks()]
    FlowTail tail;             // level-1 flows: the predictor
    int64_t n_pairs;
    FastDiv div_nb, div_nx, div_chunks;   // filled by the launcher
    int32_t first_generation;  // workgroups of the first generation = CUs of the device (set by the caller)
    int32_t stagger_groups, stagger_ticks;   // start-up stagger; stagger_groups == 0: the launcher chooses
    int32_t rows_per_sweep;    // launcher: level-1 rows one sweep of the workgroup's lanes covers
};

// The one-workgroup kernel for small pairs (k_flow_small): one or two levels of a pair whose frames
// fit LDS and whose grids have at most 256 blocks each.  Reads l0.prev / l0.cur only; l1.prev,
// l1.cur, the pred and sums pointers inside l0 / l1 are not used (level-1 frames, predictor and
// deltas stay on chip).
struct SmallArgs {
    SearchArgs l0, l1;         // l1 only for levels == 2
    FlowTail t0, t1;
    uint32_t *sums;            // [n_pairs][2][2] written here, or nullptr when not equalising
    int32_t levels;
};

struct PyramidArgs {
    const uint8_t *prev, *cur;
    int64_t pair_stride;
    int32_t w, h;
    uint8_t *l1_prev, *l1_cur; // [n_pairs][h/2][w/2] or nullptr (sums only)
    uint32_t *sums;            // [n_pairs][2][2] or nullptr (pyramid only)
    int64_t n_pairs;
    // A frame SEQUENCE (cur = prev + one frame, pair_stride = one frame): every frame is summed and filtered ONCE.
    // n_pairs then counts the FRAMES (pairs + 1), `prev` is the first frame, `cur` / `l1_cur` are not used,
    // l1_prev receives one level-1 frame per frame, and frame f's sums go to pair f (prev) and pair f - 1 (cur).
    int32_t sequence;
};

// Kernel launchers (one per .hip file).  All enqueue on `stream` and return the
// hipError_t of the launch as int (0 = ok).
int launch_pyramid(const PyramidArgs &a, void *stream);   // zeroes a.sums first
int launch_zero_words(uint32_t *words, int64_t count, void *stream);   // (a kernel: replays correctly from a hipGraph)
int launch_coarse_fused(const CoarseArgs &a, void *stream);
int launch_search_generic(const SearchArgs &a, void *stream);
// K2b: half-pixel refinement of records written by an integer search (tile 8 or 16; today only
// the 16x16 kernel needs it); fills a.subdirs.
int launch_refine(const SearchArgs &a, void *stream);
// Lane-per-block kernel straight from global memory for B=8, S=4 on ANY grid / width /
// predictor (sparse PX4Flow grid, rows that are no multiple of 16 bytes), half-pixel refinement
// included (lane8_plan_supported, aof_small_plan.hpp).
// tail + votes: the reduction runs inside the same launch (votes through agent-scope atomics into the
// context's vote memory, the last wave of a pair writes its flow record); no K3 follows (lane8_votes_verdict,
// aof_lane8_plan.hpp).
int launch_search_lane8(const SearchArgs &a, void *stream, const FlowTail *tail = nullptr,
                        const VoteMem *votes = nullptr, PruneReport *report = nullptr);
// The pruned kernels carry their hints from block to block of a wave and need a launch large enough for walks of three
// blocks before that pays: at least kPruneMinChunks (below) 256-block chunks (lane8_flat_plan, aof_lane8_plan.hpp).
// The pruned search on dense grids as a column walk (k_search_cols8.hip; lane8_cols_supported, aof_cols8_plan.hpp).  Same
// modes (a.prune 1 / 2), same report.  tail + votes: the reduction in the same launch (lane8_cols_votes_supported).
int launch_search_lane8_cols(const SearchArgs &a, void *stream, PruneReport *report = nullptr, const FlowTail *tail = nullptr,
                             const VoteMem *votes = nullptr);
// Smallest launch (in 256-block chunks) the ADAPTIVE mode lets prune.  Round 5 sweep, bench.py --pairs N as it chooses
// itself (two batches in flight, graph replay), pruned column walk against the exhaustive kernel with the reduction in
// its launch, us per step (profiles/r05_small_launch_prune_sweep.txt): 32 pairs 14.7 / 11.0, 64: 18.6 / 14.8,
// 96: 22.2 / 20.4, 128: 23.0-24.5 / 26.0, 192: 26.6 / 38.0, 256: 33.8 / 49.7 -- a walk of two blocks pays for its vote
// and its second round of row loads with too little; from three blocks on (112 VGA pairs) it wins.
constexpr int64_t kPruneMinChunks = 2048;
// Grids of 8..256 blocks: a workgroup owns whole pairs and also writes their flow records (no K3; lane8_group_plan,
// aof_small_plan.hpp).
int launch_flow_lane8(const SearchArgs &a, const FlowTail &tail, void *stream);
// LDS-tiled (block, dy)-per-lane kernel for B=16, S=8 on a dense grid (any predictor; tile16_plan, aof_tile16_plan.hpp).
// Test hook of the adaptive 16x16 search (aof_debug_tile16_verdicts): pair i gets v[i % count] instead of the probe's
// verdict; count 0 = the probe decides.  Only launches with prune == 2 read it.
constexpr int kMaxForcedVerdicts = 8;
struct Tile16Verdicts {
    uint8_t v[kMaxForcedVerdicts];
    int32_t count;
};
int launch_search_tile16(const SearchArgs &a, void *stream, const Tile16Verdicts &forced);
// Small pairs (frames fit LDS, grids <= 256 blocks), one or two levels, in one launch: one workgroup per pair
// (small_plan_make, aof_small_plan.hpp).
int launch_flow_small(const SmallArgs &a, void *stream);
// One pair, the record published in pinned host memory by ONE tagged 16-byte store (top byte of `count` =
// low byte of *tag, which the host wrote before the launch): the per-call path polls for it.
int launch_flow_small_tagged(const SmallArgs &a, aof_flow *host_record, const uint32_t *tag, void *stream);
// The resident form of the same kernel for the per-call path: one workgroup that stays on the device and
// serves requests posted through a mailbox in pinned host memory (k_flow_small.hip).
struct ResidentBox {
    // host -> device, ONE 64-bit word (one PCIe read per poll): bits 0..31 the number of the newest request
    // (never 0), bit 32 which of the two pinned frames is the newest (the other is its predecessor), bits
    // 33..62 the low 30 bits of the request at which that OTHER frame was posted + 1 (0 = not through a
    // request), bit 63 = leave now
    unsigned long long word;
    uint32_t pad0[14];
    uint32_t done;      // device: number of the last request served (its record is in place)
    uint32_t running;   // host sets 1 before the launch, the device 0 when it leaves (the host never clears it)
    uint32_t exited;    // device: `done` at the moment it left
    uint32_t started;   // device: launch number of the instance that last reached its polling loop (diagnostics:
                        // tells "never got onto the device" from "on the device but not answering")
    uint32_t pad1[12];
};
static_assert(sizeof(ResidentBox) == 128, "two cache lines: host -> device, device -> host");
constexpr unsigned long long kResidentStopBit = 1ull << 63;
inline unsigned long long resident_word(uint32_t request, int slot, uint32_t prev_request)
{
    const unsigned long long prev = prev_request ? (unsigned long long)(prev_request & 0x3FFFFFFFu) + 1ull : 0ull;
    return (unsigned long long)request | ((unsigned long long)(slot & 1) << 32) | (prev << 33);
}
// host_record: the pinned 16-byte record the host polls (top byte of `count` = low byte of the request).
int launch_flow_resident(const SmallArgs &a, ResidentBox *box, aof_flow *host_record, const uint8_t *frame_a,
                         const uint8_t *frame_b, uint32_t served, uint32_t launch_no, uint64_t idle_ticks,
                         uint64_t life_ticks, bool deaf, void *stream);
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
// The stream bank (aof_bank.cpp, k_bank.hip; include/aof.h "a bank of live streams").  Layout of a bank:
//   frames   u8 [S][frame_stride]     the stored (previous) frame of every stream
//   state    BankState [S]            what one facade object keeps between calcFlow() calls, 64 bytes per stream
//   scratch  aof_workspace_layout(p, S) bytes (block records, sub-pixel directions, pixel sums and, on the composed
//            path, everything the batch plan needs), then aof_flow [S]: the tick's pixel records
//   staging  (aof_bank_camera_layout only) u8 [S][frame_stride]: the tick's cropped frames on the composed path of
//            aof_bank_push_camera_device, then u32 [S][10]: their raw exposure histograms
// every region at a multiple of 256 bytes.
struct BankState {
    uint32_t has_prev;         // 0 after a reset: the next frame is the stream's first
    uint32_t time_last_pub;    // OpticalFlow::time_last_pub
    float sum_flow_x, sum_flow_y;   // the limiter's sums (initLimitRate)
    int32_t sum_flow_quality, valid_frame_count;
    double gyro_x, gyro_y, gyro_z;  // summed since the last publication (mainloop.cpp:383-405)
    uint32_t messages;         // records published so far: the next MAVLink sequence number is first_seq + messages
    uint32_t frames;           // frames the stream has been given
    uint64_t next_exposure_us; // aof_bank_push_camera_device: the stream's exposure gate (mainloop.cpp:273-274); 0 after a
                               // reset.  The plain push passes it through.
};
static_assert(sizeof(BankState) == 64, "one bank state record is 64 bytes");
// The regions of a bank (aof_bank.cpp): aof_bank_layout's offsets and what the library keeps to itself.  -EINVAL for
// parameters a push refuses (n_streams, frame_stride, focal lengths), or what aof_params_check / aof_workspace_layout say.
struct BankLayout {
    struct aof_bank_layout pub;
    size_t flow_ws_bytes, flows;   // inside the bank: the engine's workspace is at pub.scratch, the pixel records at `flows`
    int64_t stride, frame;
    size_t staging, staging_hist;  // camera layout only: the tick's cropped frames and their raw histograms
};
int bank_layout(const aof_params *p, const aof_bank_params *bp, BankLayout *L);
// What aof_bank_push_camera_device adds to a tick (include/aof.h, "sensor frames").  camera == nullptr: a plain tick.
struct BankCamera {
    const uint8_t *camera;         // [S] sensor frames, stream s at + s * camera_stride; its crop starts `origin` bytes in
    int64_t camera_stride;
    int32_t pitch, origin;         // bytes between sensor rows; y0 * pitch + x0 of the crop rectangle
    int32_t crop_w, crop_h;
    int32_t mx0, my0, mx1, my1;    // the exposure mask inside the crop (mainloop.cpp:203-206, clipped)
    const uint32_t *hist;          // composed path: [S][10] raw histograms of the tick's crops (k_ingest)
    aof_exposure_record *exposure; // [S] or nullptr (no statistics, the gate does not move)
    uint32_t interval_us;
    float *derotated;              // [S][2] or nullptr
    aof_derotate_params derotate;
};
struct BankArgs {
    int32_t n_streams;
    int64_t frame_stride, frame_bytes;
    const uint8_t *frames;         // the tick's frames, stream s at + s * frame_stride
    const uint64_t *time_us;       // [S]
    const uint8_t *active;         // [S] or nullptr (= all)
    const aof_gyro *gyro;          // [S] or nullptr (zeros)
    uint8_t *bank_frames;          // [S][frame_stride]
    BankState *state;              // [S]
    const aof_flow *flows;         // [S] the tick's pixel records (composed path: written by the batch plan)
    int32_t output_rate;
    float period_us;               // limiter_period_us(output_rate)
    float focal_x, focal_y;
    uint64_t offset_timestamp_usec;
    uint8_t system_id, component_id, first_seq;
    // [S] per-stream values in place of output_rate .. first_seq (aof_set_bank_streams), or nullptr.  Here, beside the
    // scalars it replaces, and not behind `cam`: measured there, the UNBOUND tick lost 0.3 us (LAB_LOG.md, "Stream bank
    // per-stream cameras")
    const aof_bank_stream *streams;
    aof_tick_record *records;      // [S]
    uint8_t *mavlink;              // [S][AOF_SEQ_FRAME_BYTES] or nullptr
    uint8_t *mavlink_len;          // [S]
    BankCamera cam;                // (last: the plain kernels' argument offsets stay)
};
// Per-stream sensor records in place of cam.camera_stride, cam.pitch and cam.origin (aof_set_bank_sensors): a kernel
// argument of its own that only the instantiations for a bound array have -- with nothing bound the launched kernels
// and their BankArgs are the ones without it, argument for argument.  recs: [S]; camera_bytes: what the records are
// valid against; camera_base: bytes between the caller's d_camera and cam.camera (a burst's composed path: round k's
// launches see cam.camera = d_camera + k * round_stride).  recs == nullptr: nothing bound.
// formats: [S] the streams' pixel formats (aof_set_bank_pixel_formats), or nullptr: one grey byte per pixel.
// bins: [S] the streams' binning (aof_set_bank_binning), or nullptr: 1 everywhere.
struct BankSensors {
    const aof_bank_sensor *recs;
    uint64_t camera_bytes, camera_base;
    const uint8_t *formats;
    const uint8_t *bins;
};
// One launch per tick: a workgroup per stream computes the pair with flow_small_pair, runs the stream's tail and
// stores the new frame (sm: the small-pair plan of (bank frames, tick frames), small_plan_make).  With
// a.cam.camera the workgroup fetches the crop's rows from the stream's sensor frame itself (a.frames is not read).
int launch_bank_tick(const SmallArgs &sm, const BankArgs &a, void *stream, const BankSensors &sen = BankSensors{nullptr, 0, 0, nullptr, nullptr});
// Behind aof_flow_batch_device on (bank frames, tick frames): the tail of every stream and the masked copy of the
// active streams' frames into the bank.  With a.cam.camera: a.frames is the staging region, and the exposure gate,
// the exposure record and the de-rotated pair come from here as well.
// A burst's composed path runs it once per round: `a` carries the round's buffers, and stream s is active iff
// round < count[s] (count NULL: a.active decides, as in a tick).
int launch_bank_commit(const BankArgs &a, void *stream, const uint8_t *count = nullptr, int32_t round = 0,
                       const BankSensors &sen = BankSensors{nullptr, 0, 0, nullptr, nullptr});
// K frame rounds per stream (aof_bank_push_burst_device, k_bank_burst.hip).  Round k's frame of stream s sits
// round_stride bytes behind round k - 1's; time_us, gyro, records, mavlink_len, mavlink, cam.exposure and
// cam.derotated of a BankArgs are then dense [K][S] arrays, a.active is not read.
struct BankBurst {
    int32_t n_rounds;              // K, 1..AOF_BANK_BURST_MAX
    int64_t round_stride;          // bytes between the rounds of a.frames (a.cam.camera for the camera form)
    const uint8_t *count;          // [S] frames per stream (values above K count as K), or nullptr (= K)
};
// One launch per burst: a workgroup per stream walks its rounds with one frame resident in LDS (same configuration
// class and same `sm` as launch_bank_tick).
int launch_bank_burst(const SmallArgs &sm, const BankArgs &a, const BankBurst &b, void *stream,
                      const BankSensors &sen = BankSensors{nullptr, 0, 0, nullptr, nullptr});
int launch_bank_reset(BankState *state, const uint8_t *mask, int32_t n_streams, void *stream);
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
// The motion-field fit's host side (aof_field.cpp), for the stream bank's motion field (aof_bank_field.cpp): are the
// parameters outside their ranges; the geometry of a configuration's level-0 grid, or -EINVAL where the fit does not serve
// it; and the fit of one pair on host memory (flow: read for pred_x / pred_y).
struct FieldGeom;                             // (aof_field_step.hpp)
bool field_bad_params(const aof_field_params *fp);
int field_geom(const aof_params *p, const aof_field_params *fp, FieldGeom *out);
void field_pair(const FieldGeom &g, const aof_block *blocks, const uint8_t *subdirs, const aof_flow &flow, aof_field *out);
// (aof_batch.cpp) the small-pair plan of n pairs, whatever n: true where one workgroup per pair can serve the
// context's configuration and these buffers (flows: [n]; d_workspace: aof_workspace_layout(p, n))
bool plan_small_batch(const aof_ctx *ctx, const uint8_t *prev, const uint8_t *cur, int64_t stride, int64_t n, aof_flow *flows,
                      void *d_workspace, SmallArgs *sm);
// (aof_batch.cpp) the small-pair plan of a configuration alone (no context, no buffers: pointers that are only looked at
// for their alignment): true where one workgroup per pair can serve `p`
bool plan_small_params(const aof_params *p, SmallArgs *sm);
int bank_path(const aof_ctx *ctx);            // (aof_batch.cpp) aof_set_bank_path's value
int &bank_last_path(aof_ctx *ctx);            // (aof_batch.cpp) aof_bank_last_path's value: 0 no push yet, 1 one-launch kernel(s), 2 composed
void set_bank_path(aof_ctx *ctx, int path);
struct BankTables;                            // (aof_bank_tables.hpp) what the four aof_set_bank_* calls have bound
BankTables &bank_tables(aof_ctx *ctx);        // (aof_batch.cpp) the context's
struct BankWarps;                             // (aof_bank_tables.hpp) what aof_set_bank_warps has bound
BankWarps &bank_warps(aof_ctx *ctx);          // (aof_batch.cpp) the context's
// (aof_capi.hip) sticky fault / wedged state and current-device check of a context, before anything is enqueued; and
// aof_last_error's text for the callers outside aof_capi.hip
int precheck(aof_ctx *ctx);
int ctx_fail(aof_ctx *ctx, int code, const char *what);
// (aof_batch.cpp) the flow of a frame sequence for the pipeline: does the call run K1 as a pass of its own, and the
// call itself with K1's outputs already in the workspace
bool sequence_runs_k1(aof_ctx *ctx, const uint8_t *d_frames, int64_t n_pairs, void *d_workspace);
int flow_sequence(aof_ctx *ctx, const uint8_t *d_frames, int64_t n_pairs, aof_flow *d_flows, void *d_workspace,
                  size_t workspace_bytes, void *stream, bool k1_ready);
int launch_reduce(const ReduceArgs &a, void *stream);
int launch_derotate(const aof_derotate_params &p, const aof_flow *flows, const aof_gyro *gyro,
                    int64_t n, float *out, void *stream);
// sensors.recs (or nullptr: the kernel without the argument): frame i's place, pitch and crop origin come from record i, valid against camera_bytes with
// `camera` `base` bytes into the caller's buffer (bank_sensor, aof_bank_stream.hpp); p.camera_width / camera_height and
// camera_stride are then not used.  ok: u8 [n_frames] or nullptr, 1 where the record let the frame be read.
struct IngestSensors {
    const aof_bank_sensor *recs;
    uint64_t base, camera_bytes;
    uint8_t *ok;
    const uint8_t *formats;   // [n_frames] AOF_PIXEL_* of frame i, or nullptr: one grey byte per pixel
    const uint8_t *bins;      // [n_frames] binning of frame i (1, 2, 4), or nullptr: 1
};
int launch_ingest(const aof_ingest_params &p, const uint8_t *camera, int64_t camera_stride,
                  int64_t n_frames, uint8_t *cropped, int64_t cropped_stride, uint32_t *hist,
                  void *stream, const IngestSensors &sensors = IngestSensors{nullptr, 0, 0, nullptr, nullptr, nullptr});
// The sequence pipeline's ingest: the same pass also leaves every frame's level-1 image (l1: [n_frames] frames, or
// nullptr) and adds its byte sums to the pixel-sum records of the pairs it belongs to (sums: [n_frames - 1][2][2],
// zeroed here; or nullptr) -- what K1 would otherwise compute in a second pass over the cropped frames.
bool ingest_pyramid_supported(const aof_ingest_params &p, const uint8_t *cropped, int64_t cropped_stride);
int launch_ingest_pyramid(const aof_ingest_params &p, const uint8_t *camera, int64_t camera_stride, int64_t n_frames,
                          uint8_t *cropped, int64_t cropped_stride, uint32_t *hist, uint8_t *l1, uint32_t *sums, void *stream);

// The warp of n_frames crops through their meshes (k_bank_warp.hip; include/aof.h "the stream bank with a lens"): where
// launch_ingest stands in a camera push with aof_set_bank_warps bound, and behind aof_ingest_warped_device.  Frame i's
// plane is record i's (recs, formats, base, camera_bytes as IngestSensors), or with recs == nullptr the grey frame of
// plane_w x plane_h at camera + i * camera_stride (then the crop of an unwarped frame is the centred one).
struct WarpArgs {
    int32_t crop_w, crop_h;
    const uint8_t *camera;
    const aof_bank_sensor *recs;
    uint64_t base, camera_bytes;
    const uint8_t *formats;
    int64_t camera_stride;
    int32_t plane_w, plane_h;
    const aof_warp_point *points;  // [n_frames][ny][nx], 16-byte aligned
    uint8_t *cropped;              // [n_frames] crops cropped_stride apart, or nullptr
    int64_t cropped_stride;
    uint32_t *hist;                // [n_frames][10] raw masked histograms, or nullptr
    uint8_t *ok;                   // u8 [n_frames] or nullptr
    int32_t nstrips, strip_rows, vec, nx, ny;   // filled by the launcher
};
int launch_warp(const WarpArgs &a, int64_t n_frames, void *stream);   // hipErrorInvalidValue: a crop too wide for a strip's nodes
// The one-launch tick with the warp inside it (k_bank_tick_warp.hip): launch_bank_tick's camera form with stream s's mesh
// (points: [S][ny][nx]) in front of the new frame; sen.recs may be nullptr (the plane is then the call's grey frame of
// cam.pitch x plane_h), sen.bins must be.  (count, round): launch_bank_commit's -- a burst's round k is one launch with
// round_args' pointers.  Needs small_warp_plan_make(sm, nodes).ok (aof_small_plan.hpp); the staging region is not touched.
int launch_bank_tick_warped(const SmallArgs &sm, const BankArgs &a, const BankSensors &sen, const aof_warp_point *points, int32_t plane_h,
                            void *stream, const uint8_t *count = nullptr, int32_t round = 0);

}  // namespace aof
