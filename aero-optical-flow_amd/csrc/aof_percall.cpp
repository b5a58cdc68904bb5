// The per-call host paths of the C ABI (aof_flow_pair_host, aof_stream_push_host): the context's stream, device and
// pinned buffers, the two captured per-call graphs, the tagged 16-byte records, and the resident kernel.
#include <cerrno>
#include <cstdio>
#include <cstring>

#include "aof_ctx.hpp"
#include "aof_engine_args.hpp"
#include "aof_resident.hpp"

using namespace aof;

namespace {

constexpr uint64_t kResidentIdleTicks = 5000000;    // 50 ms of the 100 MHz counter without a request: the kernel leaves
constexpr uint64_t kResidentLifeTicks = 20000000;   // 200 ms in total: nothing that waits for the device waits longer
constexpr double kTaggedRecordWaitS = 0.002;         // per-call graph: polling for the tagged record this long, then the stream decides
constexpr double kResidentHostTimeoutS = 0.25;      // the host gives up on a request and falls back to the graph path

// Forgets the host-buffer state without freeing it (part of it belongs to a resident kernel that did not
// leave, or the device did not drain: a hipFree would wait for that without a time limit).
void forget_host_state(aof_ctx *ctx) { ctx->host = {}; }

int alloc_host_state(aof_ctx *ctx)
{
    const aof_params &p = ctx->cfg.params;
    HostState &h = ctx->host;
    const size_t frame = (size_t)p.width * p.height;
    aof_ws_layout L;
    aof_workspace_layout(&p, 1, &L);
    HIP_TRY(ctx, hipStreamCreateWithFlags(&h.stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) HIP_TRY(ctx, hipMalloc((void **)&h.d_frames[i], frame));
    for (int i = 0; i < 2; i++) HIP_TRY(ctx, hipMalloc((void **)&h.d_pair[i], frame));
    HIP_TRY(ctx, hipMalloc((void **)&h.d_blocks, sizeof(aof_block) * (size_t)ctx->cfg.g0.blocks()));
    HIP_TRY(ctx, hipMalloc((void **)&h.d_subdirs, (size_t)ctx->cfg.g0.blocks()));
    HIP_TRY(ctx, hipMalloc(&h.d_ws, L.total_bytes));
    h.ws_bytes = L.total_bytes;
    HIP_TRY(ctx, hipMalloc((void **)&h.d_flow, sizeof(aof_flow)));
    HIP_TRY(ctx, hipHostMalloc((void **)&h.h_frame, frame, hipHostMallocDefault));
    // Frames of up to 64 KB (the reference's 64x64 .. 128x128 images) are not copied to the device
    // at all: the kernels read the pinned host copies over PCIe, which takes less time than the
    // copy node it replaces.  Larger frames keep the H2D copy and the device-resident previous frame.
    h.zero_copy = frame <= 64 * 1024;
    if (h.zero_copy)
        for (int i = 0; i < 2; i++)
            HIP_TRY(ctx, hipHostMalloc((void **)&h.h_frames[i], frame, hipHostMallocMapped | hipHostMallocCoherent));
    // (record in the first cache line, the tag of the next tagged record in the second)
    HIP_TRY(ctx, hipHostMalloc((void **)&h.h_flow, 128, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(h.h_flow, 0, 128);
    h.h_tag = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(h.h_flow) + 64);
    return 0;
}

// Stream, device frames and pinned buffers of the host-buffer entry points, made on first use.
// A failure half-way frees what was made, so that a later call starts from scratch instead of
// overwriting (leaking) live handles.
int ensure_host_state(aof_ctx *ctx)
{
    if (ctx->host.ready) return 0;
    const int rc = alloc_host_state(ctx);
    if (rc) free_host_state(ctx);
    else ctx->host.ready = true;
    return rc;
}

// The tagged 16-byte record of the per-call paths (k_flow_small_tagged, k_flow_resident): the device
// publishes it with ONE 16-byte store to a 16-byte aligned address in pinned, coherent host memory -- one
// PCIe write, which the root complex commits to its cache line as a whole -- and the top byte of `count`
// (word 2) carries the tag.  The host reads it with ONE 16-byte load (an aligned SSE load is a single
// access), checks the tag IN THAT COPY, and reads once more to see the same bytes again.
typedef uint32_t RecordWords __attribute__((vector_size(16)));
inline bool read_tagged_record(const aof_flow *pinned, uint32_t tag, aof_flow *out)
{
    const volatile RecordWords *rec = reinterpret_cast<const volatile RecordWords *>(pinned);
    const RecordWords a = *rec;
    if ((a[2] & 0xFF000000u) != tag) return false;
    const RecordWords b = *rec;
    if (a[0] != b[0] || a[1] != b[1] || a[2] != b[2] || a[3] != b[3]) return false;
    std::memcpy(out, &a, sizeof(*out));
    out->count &= 0x00FFFFFFu;
    return true;
}

// Before a request is posted: whatever record is in place (first use, a record of the other path) must not
// carry the new request's tag.
inline void retag_stale_record(aof_flow *pinned, uint32_t tag)
{
    volatile uint32_t *word = &reinterpret_cast<volatile uint32_t *>(pinned)[2];
    if ((*word & 0xFF000000u) == tag) *word ^= 0x80000000u;
}

// Captures [H2D frame -> kernels (result written to pinned host memory)] for destination
// slot `slot` into a graph.
// Any failure leaves the context on the plain (un-captured) path; never an error.
void build_push_graph(aof_ctx *ctx, int slot)
{
    HostState &h = ctx->host;
    const aof_params &p = ctx->cfg.params;
    const size_t bytes = (size_t)p.width * p.height;
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(h.stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        ctx->graph_disabled = true;
        return;
    }
    ctx->capturing = true;
    uint8_t *const *frames = h.zero_copy ? h.h_frames : h.d_frames;
    bool ok = false, tagged = false;
    if (h.zero_copy) {
        // small frames served by the one-workgroup kernel: the record comes tagged (stream_push_graph polls
        // for it); the kernel's own copy goes to device memory
        SmallArgs sm;
        if (plan_small_pair(ctx, frames[1 - slot], frames[slot], h.d_flow, &sm)) {
            tagged = true;
            ok = launch_flow_small_tagged(sm, h.h_flow, h.h_tag, h.stream) == 0;
        }
    }
    if (!tagged) {
        ok = h.zero_copy || hipMemcpyAsync(h.d_frames[slot], h.h_frame, bytes, hipMemcpyHostToDevice, h.stream) == hipSuccess;
        // K3 writes the 16-byte result straight into the pinned (device-visible, coherent) host
        // record: no D2H copy node; it is visible to the host once the stream has drained.
        ok = ok && aof_flow_batch_device(ctx, frames[1 - slot], frames[slot], (int64_t)bytes, 1, h.d_blocks, h.d_subdirs,
                                         h.h_flow, h.d_ws, h.ws_bytes, h.stream) == 0;
    }
    ctx->capturing = false;
    const bool ended = hipStreamEndCapture(h.stream, &graph) == hipSuccess && graph;
    if (ok && ended && hipGraphInstantiate(&h.push_graph[slot], graph, nullptr, nullptr, 0) == hipSuccess) {
        (void)hipGraphDestroy(graph);
        h.push_tagged[slot] = tagged;
        return;
    }
    if (graph) (void)hipGraphDestroy(graph);
    h.push_graph[slot] = nullptr;
    ctx->graph_disabled = true;
    (void)hipGetLastError();
}

int run_one(aof_ctx *ctx, const uint8_t *d_prev, const uint8_t *d_cur, aof_block *blocks, uint8_t *subdirs, aof_flow *flow)
{
    HostState &h = ctx->host;
    const aof_params &p = ctx->cfg.params;
    int rc = aof_flow_batch_device(ctx, d_prev, d_cur, (int64_t)p.width * p.height, 1, h.d_blocks, h.d_subdirs, h.d_flow,
                                   h.d_ws, h.ws_bytes, h.stream);
    if (rc) return rc;
    const size_t nb = (size_t)ctx->cfg.g0.blocks();
    HIP_TRY(ctx, hipMemcpyAsync(flow, h.d_flow, sizeof(aof_flow), hipMemcpyDeviceToHost, h.stream));
    if (blocks)
        HIP_TRY(ctx, hipMemcpyAsync(blocks, h.d_blocks, nb * sizeof(aof_block), hipMemcpyDeviceToHost, h.stream));
    if (subdirs) {
        if (p.subpixel)
            HIP_TRY(ctx, hipMemcpyAsync(subdirs, h.d_subdirs, nb, hipMemcpyDeviceToHost, h.stream));
        else
            std::memset(subdirs, 8, nb);
    }
    if (const hipError_t e = drain_bounded(h.stream, kDrainS)) return wedge(ctx, "waiting for the pair's kernels and copies", e);
    return 0;
}

// Same contract as the plain path of aof_stream_push_host, one hipGraphLaunch per frame.
int stream_push_graph(aof_ctx *ctx, const uint8_t *frame, aof_flow *flow, int slot)
{
    HostState &h = ctx->host;
    ctx->res.frame_req[slot] = 0;   // (written outside a resident request)
    std::memcpy(h.zero_copy ? h.h_frames[slot] : h.h_frame, frame, (size_t)ctx->cfg.params.width * ctx->cfg.params.height);
    const bool tagged = h.push_tagged[slot];
    uint32_t tag = 0;
    if (tagged) {
        tag = ++ctx->res.seq << 24;
        retag_stale_record(h.h_flow, tag);
        __atomic_store_n(h.h_tag, ctx->res.seq, __ATOMIC_RELEASE);
    }
    hipError_t e = hipGraphLaunch(h.push_graph[slot], h.stream);
    if (e == hipSuccess && tagged) {
        // The record arrives tagged: the kernel is through with both frames when it is there, and the
        // runtime's own completion path (longer than the kernel) is not waited for.  A record that stays
        // away for 2 ms is left to the stream -- bounded: the stream drains (and the record is there), or it
        // reports the fault, or the time runs out and the context is disabled.
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spins = 1; !read_tagged_record(h.h_flow, tag, flow); spins++) {
            if ((spins & 0x3FFu) == 0 && seconds_since(t0) > kTaggedRecordWaitS) {
                ctx->stats.tagged_slow++;
                e = drain_bounded(h.stream, kDrainS);
                if (e == hipSuccess && !read_tagged_record(h.h_flow, tag, flow)) e = hipErrorUnknown;
                break;
            }
        }
    } else if (e == hipSuccess) {
        e = drain_bounded(h.stream, kDrainS);
        if (e == hipSuccess) *flow = *h.h_flow;
    }
    if (e != hipSuccess) {
        h.have_prev = false;
        if (e == hipErrorNotReady) return wedge(ctx, "per-call graph replay", e);
        return fail(ctx, -EIO, "graph replay: %s", hipGetErrorString(e));
    }
    h.cur_slot = slot;
    return 0;
}

// The resident path: post the request, make sure the kernel is there, wait for its tagged record.
// *served = false (and 0) when the one-workgroup kernel does not serve this configuration, or when it did
// not answer (the caller's frame then takes the launch-per-call path).
int stream_push_resident(aof_ctx *ctx, const uint8_t *frame, aof_flow *flow, int slot, bool *served)
{
    HostState &h = ctx->host;
    Resident &r = ctx->res;
    const size_t bytes = (size_t)ctx->cfg.params.width * ctx->cfg.params.height;
    *served = false;
    if (!r.k.box) {
        // The kernel's own stream at the HIGHEST priority: the runtime keeps a pool of hardware queues per priority,
        // so a parked resident kernel never shares one (every packet carrying the barrier bit) with normal-priority
        // streams.  Behind another context's resident kernel (from the fifth on, GPU_MAX_HW_QUEUES = 4) it starts
        // when that one leaves, at most 200 ms later: inside the 250 ms a request waits.
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (hipHostMalloc((void **)&r.k.box, sizeof(ResidentBox), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
            (hipStreamCreateWithPriority(&r.k.stream, hipStreamNonBlocking, greatest) != hipSuccess &&
             hipStreamCreateWithFlags(&r.k.stream, hipStreamNonBlocking) != hipSuccess)) {
            if (r.k.box) (void)hipHostFree(r.k.box);
            r.k = {};
            r.on = false;
            (void)hipGetLastError();
            return 0;
        }
        std::memset(r.k.box, 0, sizeof(ResidentBox));
        r.k.launches = 0;
    }
    // (the frame pointers of the view are placeholders: the kernel picks the two pinned frames by slot)
    // (the kernel's own copy of the record goes to device memory; the host's comes tagged, below)
    SmallArgs sm;
    if (!plan_small_pair(ctx, h.h_frames[0], h.h_frames[1], h.d_flow, &sm)) return 0;
    ResidentBox *box = r.k.box;
    std::memcpy(h.h_frames[slot], frame, bytes);
    uint32_t seq = ++r.seq;
    if (seq == 0) seq = ++r.seq;   // 0 means "no request" to the kernel
    const uint32_t tag = seq << 24;
    retag_stale_record(h.h_flow, tag);
    __atomic_store_n(&box->word, resident_word(seq, slot, r.frame_req[1 - slot]), __ATOMIC_RELEASE);   // the frame bytes first
    r.frame_req[slot] = seq;
    // The clock of the request: restarted whenever a launch returns -- the FIRST launch of the kernel in a
    // process loads its code object and creates the stream's hardware queue inside hipLaunchKernelGGL, which
    // takes longer than any answer (measured: aof_stream_stats.launch_call_us_max), and that is not the
    // kernel failing to answer.
    auto t0 = std::chrono::steady_clock::now();
    bool launched = false, start_seen = true;
    for (unsigned spins = 0;;) {
        if (read_tagged_record(h.h_flow, tag, flow)) break;
        if (!__atomic_load_n(&box->running, __ATOMIC_ACQUIRE)) {
            // not there (first call, or it left on its idle / lifetime deadline): start it behind its
            // predecessor, serving from the last request that one completed
            if (read_tagged_record(h.h_flow, tag, flow)) break;
            __atomic_store_n(&box->running, 1u, __ATOMIC_RELEASE);
            const auto l0 = std::chrono::steady_clock::now();
            const int lrc = launch_flow_resident(sm, box, h.h_flow, h.h_frames[0], h.h_frames[1],
                                                 __atomic_load_n(&box->done, __ATOMIC_ACQUIRE), ++r.k.launches,
                                                 kResidentIdleTicks, kResidentLifeTicks, r.deaf, r.k.stream);
            if (lrc) {
                // nothing was enqueued: the flag is the host's to take back
                __atomic_store_n(&box->running, 0u, __ATOMIC_RELEASE);
                r.on = false;
                h.have_prev = false;
                return fail(ctx, -EIO, "resident kernel launch: %s", hipGetErrorString((hipError_t)lrc));
            }
            t0 = std::chrono::steady_clock::now();
            const float us = (float)(std::chrono::duration<double>(t0 - l0).count() * 1e6);
            if (us > ctx->stats.launch_call_us_max) ctx->stats.launch_call_us_max = us;
            ctx->stats.resident_launches++;
            launched = true;
            start_seen = false;
            continue;
        }
        if (!start_seen && __atomic_load_n(&box->started, __ATOMIC_ACQUIRE) == r.k.launches) {
            // launch return -> the kernel's first instruction on the device, with no HIP call in between
            const float us = (float)(seconds_since(t0) * 1e6);
            if (us > ctx->stats.start_latency_us_max) ctx->stats.start_latency_us_max = us;
            start_seen = true;
        }
        if ((++spins & 0x3FFu) == 0 && seconds_since(t0) > kResidentHostTimeoutS) {
            // no answer: stop it, leave the resident mode and let the caller's frame take the graph path
            const hipError_t q = hipStreamQuery(r.k.stream);
            std::snprintf(ctx->stats.last_report, sizeof(ctx->stats.last_report),
                          "request %u unanswered for %.0f ms%s: record word %08x, launch %u, started %u, served %u, "
                          "exited at %u, on device %u, stream %s, longest launch call %.0f us",
                          seq, seconds_since(t0) * 1e3, launched ? " after this call's launch returned" : "",
                          (unsigned)reinterpret_cast<volatile uint32_t *>(h.h_flow)[2], r.k.launches,
                          (unsigned)box->started, (unsigned)box->done, (unsigned)box->exited, (unsigned)box->running,
                          q == hipSuccess ? "drained" : q == hipErrorNotReady ? "busy" : hipGetErrorString(q),
                          ctx->stats.launch_call_us_max);
            std::fprintf(stderr, "aof: the resident kernel did not answer (%s): falling back to one launch per call\n",
                         ctx->stats.last_report);
            ctx->stats.resident_fallbacks++;
            (void)resident_stop(ctx);   // (if it does not leave either, its buffers are abandoned with it)
            r.on = false;
            (void)hipGetLastError();
            return 0;
        }
    }
    ctx->stats.resident_served++;
    h.cur_slot = slot;
    *served = true;
    return 0;
}

}  // namespace

namespace aof {

// Runs before anything that frees what the resident kernel reads, and before a change of kernel choice.  The stop bit
// is only cleared after the DEVICE has cleared `running` (its last store), so an instance not started yet leaves at once.
// false: it did not leave within a second.  The box keeps its stop bit, the context forgets the kernel and the per-call
// host state (leaked, never reused; rebuilt on the next call), and aof_destroy frees no device memory at all.
bool resident_stop(aof_ctx *ctx)
{
    Resident &r = ctx->res;
    if (!r.k.box || !r.k.stream) return true;
    ResidentBox *box = r.k.box;
    if (!__atomic_load_n(&box->running, __ATOMIC_ACQUIRE)) return true;   // nothing launched since the last exit
    const unsigned long long word = __atomic_load_n(&box->word, __ATOMIC_ACQUIRE);
    __atomic_store_n(&box->word, word | kResidentStopBit, __ATOMIC_RELEASE);
    // The kernel clears `running` when it leaves -- at the latest on its 200 ms lifetime deadline: wait for THAT,
    // bounded.  (No HIP call is needed for the launch to reach the device: the launch has rung the doorbell.)
    const auto t0 = std::chrono::steady_clock::now();
    while (__atomic_load_n(&box->running, __ATOMIC_ACQUIRE) && seconds_since(t0) < r.stop_wait_s) {
    }
    hipError_t e = hipSuccess;
    if (!__atomic_load_n(&box->running, __ATOMIC_ACQUIRE)) {
        // it has left; the stream retires the launch within microseconds -- bounded all the same
        e = drain_bounded(r.k.stream, kDrainS);
        if (e == hipSuccess) {
            __atomic_store_n(&box->word, word & ~kResidentStopBit, __ATOMIC_RELEASE);
            return true;
        }
    }
    std::fprintf(stderr, "aof: the resident kernel did not leave within %.0f ms of being asked to (launch %u, started %u, "
                         "served %u, exited at %u, on device %u, stream: %s): its buffers are abandoned\n",
                 r.stop_wait_s * 1e3, r.k.launches, (unsigned)box->started, (unsigned)box->done, (unsigned)box->exited,
                 (unsigned)box->running, e == hipSuccess ? hipGetErrorString(hipStreamQuery(r.k.stream)) : hipGetErrorString(e));
    r.lost = true;
    r.on = false;
    ctx->stats.resident_lost++;
    r.k = {};
    forget_host_state(ctx);
    return false;
}

// Captured graphs hold the kernels chosen so far.  (The per-call path does not wait for the stream after a
// tagged record has arrived: drain it before a graph goes.)
void drop_push_graphs(aof_ctx *ctx)
{
    HostState &h = ctx->host;
    if (!h.push_graph[0] && !h.push_graph[1]) return;
    DeviceGuard guard(ctx->device);
    if (h.stream && !ctx->wedged) {
        const hipError_t e = drain_bounded(h.stream, kDrainS);
        if (e != hipSuccess) (void)wedge(ctx, "draining the per-call stream before its graphs are dropped", e);
    }
    for (int i = 0; i < 2; i++)   // (a wedged context leaks the executables: a replay may still be running)
        if (h.push_graph[i]) { if (!ctx->wedged) (void)hipGraphExecDestroy(h.push_graph[i]); h.push_graph[i] = nullptr; }
}

void free_host_state(aof_ctx *ctx)
{
    HostState &h = ctx->host;
    (void)resident_stop(ctx);
    if (ctx->res.lost || ctx->wedged) { forget_host_state(ctx); return; }
    if (h.stream) {
        const hipError_t e = drain_bounded(h.stream, kDrainS);
        if (e != hipSuccess) { (void)wedge(ctx, "draining the per-call stream", e); forget_host_state(ctx); return; }
        for (int i = 0; i < 2; i++) if (h.push_graph[i]) (void)hipGraphExecDestroy(h.push_graph[i]);
        (void)hipStreamDestroy(h.stream);
    }
    void *const dev[] = {h.d_frames[0], h.d_frames[1], h.d_pair[0], h.d_pair[1], h.d_blocks, h.d_subdirs, h.d_flow, h.d_ws};
    void *const pinned[] = {h.h_frame, h.h_frames[0], h.h_frames[1], h.h_flow};
    for (void *d : dev) if (d) (void)hipFree(d);
    for (void *m : pinned) if (m) (void)hipHostFree(m);
    forget_host_state(ctx);
}

}  // namespace aof

extern "C" {

int aof_flow_pair_host(aof_ctx *ctx, const uint8_t *prev, const uint8_t *cur, aof_block *blocks,
                       uint8_t *subdirs, aof_flow *flow)
{
    if (!ctx) return -EINVAL;
    if (!prev || !cur || !flow) return fail(ctx, -EINVAL, "null frame or flow pointer");
    if (int sticky = sticky_error(ctx)) return sticky;
    DeviceGuard guard(ctx->device);
    int rc = ensure_host_state(ctx);
    if (rc) return rc;
    HostState &h = ctx->host;
    const size_t frame = (size_t)ctx->cfg.params.width * ctx->cfg.params.height;
    // own scratch frames: the streaming state (aof_stream_push_host) is left untouched
    HIP_TRY(ctx, hipMemcpyAsync(h.d_pair[0], prev, frame, hipMemcpyHostToDevice, h.stream));
    HIP_TRY(ctx, hipMemcpyAsync(h.d_pair[1], cur, frame, hipMemcpyHostToDevice, h.stream));
    return run_one(ctx, h.d_pair[0], h.d_pair[1], blocks, subdirs, flow);
}

int aof_stream_push_host(aof_ctx *ctx, const uint8_t *frame, aof_flow *flow)
{
    if (!ctx) return -EINVAL;
    if (!frame || !flow) return fail(ctx, -EINVAL, "null frame or flow pointer");
    if (int sticky = sticky_error(ctx)) return sticky;
    DeviceGuard guard(ctx->device);
    int rc = ensure_host_state(ctx);
    if (rc) return rc;
    HostState &h = ctx->host;   // (the same object after a rebuild: ensure_host_state refills it in place)
    const size_t bytes = (size_t)ctx->cfg.params.width * ctx->cfg.params.height;
    int slot = h.have_prev ? 1 - h.cur_slot : 0;
    if (h.have_prev) ctx->stats.calls++;
    if (h.have_prev && ctx->res.on && h.zero_copy && !ctx->prof.on) {
        bool served = false;
        rc = stream_push_resident(ctx, frame, flow, slot, &served);
        if (served || rc) return rc;   // (not served and no error: this configuration takes the paths below)
        if (!h.ready) {
            // The kernel neither answered nor left: the pinned frames it may still read are abandoned, the
            // older frame with them.  This frame starts a new sequence on fresh buffers (return 1, as after
            // aof_stream_reset) -- one flow sample is lost, nothing wrong is ever reported.
            rc = ensure_host_state(ctx);
            if (rc) return rc;
            slot = 0;
        }
    }
    if (h.have_prev && !ctx->graph_disabled && !ctx->prof.on) {
        if (!h.push_graph[slot]) build_push_graph(ctx, slot);
        if (h.push_graph[slot]) return stream_push_graph(ctx, frame, flow, slot);
    }
    uint8_t *const *frames = h.zero_copy ? h.h_frames : h.d_frames;
    ctx->res.frame_req[slot] = 0;   // (written outside a resident request)
    if (h.zero_copy) std::memcpy(h.h_frames[slot], frame, bytes);
    else HIP_TRY(ctx, hipMemcpyAsync(h.d_frames[slot], frame, bytes, hipMemcpyHostToDevice, h.stream));
    if (!h.have_prev) {
        // caller may free `frame` on return
        if (const hipError_t e = drain_bounded(h.stream, kDrainS)) return wedge(ctx, "waiting for the first frame's copy", e);
        h.cur_slot = slot;
        h.have_prev = true;
        std::memset(flow, 0, sizeof(*flow));
        return 1;
    }
    rc = run_one(ctx, frames[h.cur_slot], frames[slot], nullptr, nullptr, flow);
    if (rc) {   // the new frame may be incomplete on the device: do not compare the next one with it
        h.have_prev = false;
        return rc;
    }
    h.cur_slot = slot;
    return 0;
}

int aof_set_stream_resident(aof_ctx *ctx, int on)
{
    if (!ctx) return -EINVAL;
    if (on < 0) return (ctx->res.k.box && __atomic_load_n(&ctx->res.k.box->running, __ATOMIC_ACQUIRE)) ? 1 : 0;
    if (!on) { DeviceGuard guard(ctx->device); (void)resident_stop(ctx); }
    ctx->res.on = on != 0;
    return 0;
}

int aof_debug_resident_fault(aof_ctx *ctx, int deaf, uint32_t stop_wait_us)
{
    if (!ctx) return -EINVAL;
    ctx->res.deaf = deaf != 0;
    ctx->res.stop_wait_s = stop_wait_us ? stop_wait_us * 1e-6 : 1.0;
    return 0;
}

int aof_stream_get_stats(const aof_ctx *ctx, aof_stream_stats *out)
{
    if (!ctx || !out) return -EINVAL;
    *out = ctx->stats;
    return 0;
}

int aof_set_stream_graph(aof_ctx *ctx, int on)
{
    if (!ctx) return -EINVAL;
    if (on < 0) return (ctx->host.push_graph[0] || ctx->host.push_graph[1]) ? 1 : 0;
    ctx->graph_disabled = on == 0;
    return 0;
}

int aof_stream_reset(aof_ctx *ctx)
{
    if (!ctx) return -EINVAL;
    ctx->host.have_prev = false;
    return 0;
}

}  // extern "C"
