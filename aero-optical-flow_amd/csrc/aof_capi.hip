// Host side of the C ABI (include/aof.h): context creation and destruction, the setters, event-based kernel
// timing, the ingest and de-rotation wrappers, and the error helpers the other host files share.
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <thread>

#include "aof_bank_calls.hpp"
#include "aof_bank_tables.hpp"
#include "aof_ctx.hpp"
#include "aof_engine_args.hpp"
#include "aof_host.hpp"
#include "aof_ingest_args.hpp"

using namespace aof;

namespace aof {

int fail(aof_ctx *ctx, int code, const char *fmt, ...)
{
    if (ctx) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
        va_end(ap);
    }
    return code;
}

double seconds_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// hipStreamQuery / hipEventQuery never block, hipStreamSynchronize / hipEventSynchronize have no time limit of their own.
template <class Query>
hipError_t wait_bounded(Query query, double seconds)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = query();
        if (e != hipErrorNotReady) return e;
        const double t = seconds_since(t0);
        if (t > seconds) return hipErrorNotReady;
        if (t > 200e-6) std::this_thread::sleep_for(std::chrono::microseconds(t > 5e-3 ? 500 : 20));
    }
}

hipError_t drain_bounded(hipStream_t s, double seconds) { return wait_bounded([s] { return hipStreamQuery(s); }, seconds); }

// (recovery = a new context; aof_destroy frees nothing a kernel might still touch)
int wedge(aof_ctx *ctx, const char *what, hipError_t e)
{
    const char *why = e == hipErrorNotReady ? "the device did not finish within the time limit" : hipGetErrorString(e);
    ctx->wedged = true;
    std::fprintf(stderr, "aof: %s: %s -- the context is disabled\n", what, why);
    return fail(ctx, e == hipErrorNotReady ? -ETIMEDOUT : -EIO, "%s: %s", what, why);
}

// Checked by every entry point that enqueues work: a bounded wait that ran out earlier, or the fault word a kernel
// raised (a finaliser wave of the in-launch reduction that gave up on its pair: that pair's record says quality 0,
// flags 0).  Like a sticky HIP error, it stays.
int sticky_error(aof_ctx *ctx)
{
    if (ctx->wedged) return -EIO;   // (ctx->err still holds the text of the first report)
    if (ctx->h_fault) {
        const uint32_t code = __atomic_load_n(ctx->h_fault, __ATOMIC_ACQUIRE);
        if (code)
            return fail(ctx, -EIO, "a reduction inside a search launch gave up waiting for the votes of pair %u of its "
                                   "launch (device-side deadline): that record carries quality 0 and no valid flag; "
                                   "the context's vote memory is no longer trusted -- create a new context", code - 1);
    }
    return 0;
}

int device_check(aof_ctx *ctx)
{
    int cur_dev = -1;
    if (hipGetDevice(&cur_dev) != hipSuccess || cur_dev != ctx->device)
        return fail(ctx, -EINVAL, "context was created for device %d but the calling thread's current "
                                  "device is %d", ctx->device, cur_dev);
    return 0;
}

// What every entry point that enqueues work on a context checks before its first launch: the sticky device-side
// condition, and that the calling thread's current device is the context's.  Sets aof_last_error.
int precheck(aof_ctx *ctx)
{
    if (int sticky = sticky_error(ctx)) return sticky;
    return device_check(ctx);
}

int ctx_fail(aof_ctx *ctx, int code, const char *what) { return fail(ctx, code, "%s", what); }

BankCtx &bank_ctx(aof_ctx *ctx) { return ctx->bank; }

}  // namespace aof

namespace {

// A setter that changes the kernel choice: the resident kernel and the captured per-call graphs run the kernels
// chosen so far.
void kernel_choice_changes(aof_ctx *ctx, bool changes)
{
    { DeviceGuard guard(ctx->device); (void)resident_stop(ctx); }
    if (changes) drop_push_graphs(ctx);
}

}  // namespace

extern "C" {

int aof_create(const aof_params *p, int device, aof_ctx **out)
{
    if (!out) return -EINVAL;
    *out = nullptr;
    int rc = aof_params_check(p);
    if (rc) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return -ENODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return -ENODEV;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return -ENODEV;  // kernels are gfx950 only

    aof_ctx *ctx = new (std::nothrow) aof_ctx();   // (zeroed)
    if (!ctx) return -ENOMEM;
    ctx->cfg.params = *p;
    ctx->device = device;
    ctx->cfg.cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    grid_for_level(*p, 0, &ctx->cfg.g0);
    if (p->pyramid_levels == 2) grid_for_level(*p, 1, &ctx->cfg.g1);
    std::snprintf(ctx->err, sizeof(ctx->err), "ok");
    if (p->tile == 8 && p->search == 4) {   // the flat lane8 search can reduce in its own launch
        DeviceGuard guard(device);
        const size_t bytes = (size_t)kVotePairs * kVoteStride * sizeof(uint32_t);
        if (hipMalloc((void **)&ctx->votes.mem, bytes) != hipSuccess || hipMemset(ctx->votes.mem, 0, bytes) != hipSuccess ||
            hipEventCreateWithFlags(&ctx->votes.done, hipEventDisableTiming) != hipSuccess ||
            hipHostMalloc((void **)&ctx->h_fault, 64 + kPruneSlots * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
            hipDeviceSynchronize() != hipSuccess) {
            aof_destroy(ctx);
            return -EIO;
        }
        std::memset(ctx->h_fault, 0, 64 + kPruneSlots * sizeof(uint32_t));
        ctx->adapt.slots = ctx->h_fault + 16;
        ctx->votes.pairs = kVotePairs;
    }
    {   // next to the vote records: the arrival counter of the outbox kernel (aof_bank_collect_device), zero at rest
        DeviceGuard guard(device);
        if (hipMalloc((void **)&ctx->outbox_counter, sizeof(OutboxCounter)) != hipSuccess ||
            hipMemset(ctx->outbox_counter, 0, sizeof(OutboxCounter)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
            aof_destroy(ctx);
            return -EIO;
        }
    }
    ctx->votes.deadline_ticks = kVoteDeadlineTicks;
    ctx->res.stop_wait_s = 1.0;
    ctx->votes.separate = true;   // the in-launch reduction is opt-in (aof_set_reduce_fusion)
    // exact pruning wherever it pays (include/aof.h): 16x16 tiles by a probe per pair, 8x8 tiles by what the
    // context's previous launches reported
    ctx->cfg.search_mode = AOF_SEARCH_ADAPTIVE;
    ctx->adapt.belief = -1;
    ctx->adapt.stats.belief = -1;

    *out = ctx;
    return 0;
}

void aof_destroy(aof_ctx *ctx)
{
    if (!ctx) return;
    DeviceGuard guard(ctx->device);
    (void)resident_stop(ctx);   // before anything it reads is freed
    // Every wait here is bounded: a hipFree / hipStreamDestroy / hipStreamSynchronize waits for the device
    // without a time limit, so they only run once the context's own work is known to have drained.  If it
    // has not (a lost resident kernel, a wedged device, a fault), the context's device and pinned memory and
    // its streams are leaked -- the caller (calcFlow's owner holds _mainloop_lock, mainloop.cpp:283) gets
    // control back either way.
    bool leak = ctx->res.lost || ctx->wedged;
    hipError_t e = hipSuccess;
    if (!leak && ctx->host.stream && (e = drain_bounded(ctx->host.stream, kDrainS)) != hipSuccess) leak = true;
    if (!leak && ctx->votes.done && ctx->votes.used && (e = wait_bounded([ctx] { return hipEventQuery(ctx->votes.done); }, kDrainS)) != hipSuccess)
        leak = true;
    if (ctx->prof.ev) {
        for (hipEvent_t *ev = *ctx->prof.ev[0], *end = ev + AOF_K_COUNT * AOF_PROFILE_RING * 2; ev != end; ev++)
            if (*ev) (void)hipEventDestroy(*ev);
        delete[] ctx->prof.ev;
    }
    if (leak) {
        std::fprintf(stderr, "aof: destroying a context whose device work has not drained (%s): its device memory, pinned "
                             "memory and streams are leaked, not freed\n",
                     ctx->res.lost ? "resident kernel lost" : ctx->wedged ? ctx->err : hipGetErrorString(e));
        delete ctx;
        return;
    }
    free_host_state(ctx);   // (drained above)
    if (ctx->res.k.stream) (void)hipStreamDestroy(ctx->res.k.stream);
    if (ctx->res.k.box) (void)hipHostFree(ctx->res.k.box);
    if (ctx->votes.done) (void)hipEventDestroy(ctx->votes.done);
    if (ctx->votes.mem) (void)hipFree(ctx->votes.mem);
    if (ctx->outbox_counter) (void)hipFree(ctx->outbox_counter);
    if (ctx->h_fault) (void)hipHostFree(ctx->h_fault);
    delete ctx;
}

const char *aof_last_error(const aof_ctx *ctx) { return ctx ? ctx->err : "null context"; }

int aof_get_search_mode(const aof_ctx *ctx) { return ctx ? ctx->cfg.search_mode : -EINVAL; }

int aof_get_search_stats(const aof_ctx *ctx, aof_search_stats *out)
{
    if (!ctx || !out) return -EINVAL;
    *out = ctx->adapt.stats;
    return 0;
}

int aof_set_search_belief(aof_ctx *ctx, int belief)
{
    if (!ctx || belief < -1 || belief > 1) return -EINVAL;
    ctx->adapt.belief = belief;
    ctx->adapt.stats.belief = belief;
    ctx->adapt.since_probe = 0;
    ctx->adapt.expected = 0;   // (reports of earlier launches no longer overrule the caller)
    return 0;
}

int aof_get_params(const aof_ctx *ctx, aof_params *out)
{
    if (!ctx || !out) return -EINVAL;
    *out = ctx->cfg.params;
    return 0;
}

int aof_set_force_generic(aof_ctx *ctx, int on)
{
    if (!ctx) return -EINVAL;
    kernel_choice_changes(ctx, (on != 0) != ctx->cfg.force_generic);
    ctx->cfg.force_generic = on != 0;
    return 0;
}

int aof_set_search_mode(aof_ctx *ctx, int mode)
{
    if (!ctx || mode < AOF_SEARCH_EXHAUSTIVE || mode > AOF_SEARCH_ADAPTIVE) return -EINVAL;
    kernel_choice_changes(ctx, mode != ctx->cfg.search_mode);
    ctx->cfg.search_mode = mode;
    return 0;
}

int aof_set_split_coarse(aof_ctx *ctx, int on)
{
    if (!ctx) return -EINVAL;
    kernel_choice_changes(ctx, (on != 0) != ctx->cfg.split_coarse);
    ctx->cfg.split_coarse = on != 0;
    return 0;
}

int aof_set_reduce_fusion(aof_ctx *ctx, int on)
{
    if (!ctx) return -EINVAL;
    ctx->votes.separate = on == 0;
    return 0;
}

int aof_set_vote_deadline_us(aof_ctx *ctx, uint32_t microseconds)
{
    if (!ctx) return -EINVAL;
    // below 100 us every finaliser wave would give up on its first polls, write a zero record and raise the sticky fault
    // word: one call would disable the context for good
    if (microseconds < 100u) return fail(ctx, -EINVAL, "vote deadline of %u us: at least 100 us", microseconds);
    ctx->votes.deadline_ticks = microseconds > 10000000u ? 1000000000u : microseconds * 100u;   // 100 MHz counter
    return 0;
}

int aof_debug_vote_deadline_ticks(aof_ctx *ctx, uint32_t ticks)
{
    if (!ctx) return -EINVAL;
    ctx->votes.deadline_ticks = ticks;   // (fault injection: 0 makes every finaliser wave give up at once)
    return 0;
}

int aof_debug_tile16_verdicts(aof_ctx *ctx, const uint8_t *verdicts, int count)
{
    if (!ctx) return -EINVAL;
    if (ctx->cfg.params.tile != 16) return fail(ctx, -EINVAL, "verdicts of the 16x16 search on a %dx%d context", ctx->cfg.params.tile, ctx->cfg.params.tile);
    if (count < 0 || count > kMaxForcedVerdicts) return fail(ctx, -EINVAL, "%d verdicts: 0 .. %d", count, kMaxForcedVerdicts);
    if (count > 0 && !verdicts) return fail(ctx, -EINVAL, "null verdicts");
    Tile16Verdicts f = {};
    for (int i = 0; i < count; i++) {
        if (verdicts[i] > 4) return fail(ctx, -EINVAL, "verdict %d of %u: 0 .. 4", i, verdicts[i]);
        f.v[i] = verdicts[i];
    }
    f.count = count;
    const bool changes = f.count != ctx->tile16_verdicts.count ||
                         std::memcmp(f.v, ctx->tile16_verdicts.v, sizeof f.v) != 0;
    kernel_choice_changes(ctx, changes);   // (captured per-call graphs hold the probe or the verdicts of their time)
    ctx->tile16_verdicts = f;
    return 0;
}

int aof_set_profiling(aof_ctx *ctx, int on)
{
    if (!ctx) return -EINVAL;
    DeviceGuard guard(ctx->device);
    Profiling &pr = ctx->prof;
    if (on && !pr.ev) {
        pr.ev = new (std::nothrow) hipEvent_t[AOF_K_COUNT][AOF_PROFILE_RING][2]();
        if (!pr.ev) return fail(ctx, -ENOMEM, "event ring");
        // timing only: without the system-scope fence a default event performs when it is
        // recorded (an L2 write-back and invalidation between the kernels it brackets)
        for (hipEvent_t *ev = *pr.ev[0], *end = ev + AOF_K_COUNT * AOF_PROFILE_RING * 2; ev != end; ev++)
            HIP_TRY(ctx, hipEventCreateWithFlags(ev, hipEventDisableSystemFence));
    }
    pr.on = on != 0;
    pr.mask = 0xFFFFFFFFu;
    if (on) for (int k = 0; k < AOF_K_COUNT; k++) pr.count[k] = 0;
    return 0;
}

int aof_set_profiling_mask(aof_ctx *ctx, uint32_t mask)
{
    int rc = aof_set_profiling(ctx, mask != 0);
    if (rc) return rc;
    ctx->prof.mask = mask;
    return 0;
}

int aof_profile_count(const aof_ctx *ctx, int kernel_id)
{
    if (!ctx || kernel_id < 0 || kernel_id >= AOF_K_COUNT) return -EINVAL;
    const int64_t n = ctx->prof.count[kernel_id];
    return (int)(n < AOF_PROFILE_RING ? n : AOF_PROFILE_RING);
}

int aof_profile_ms(aof_ctx *ctx, int kernel_id, int index, float *ms)
{
    if (!ctx || !ms) return -EINVAL;
    const int kept = aof_profile_count(ctx, kernel_id);
    if (kept < 0 || index < 0 || index >= kept)
        return fail(ctx, -EINVAL, "kernel %d has no timed launch %d", kernel_id, index);
    const int64_t n = ctx->prof.count[kernel_id];
    const int slot = (int)((n - kept + index) % AOF_PROFILE_RING);
    HIP_TRY(ctx, hipEventSynchronize(ctx->prof.ev[kernel_id][slot][1]));
    HIP_TRY(ctx, hipEventElapsedTime(ms, ctx->prof.ev[kernel_id][slot][0], ctx->prof.ev[kernel_id][slot][1]));
    return 0;
}

int aof_kernel_ms(aof_ctx *ctx, int kernel_id, float *ms)
{
    const int kept = ctx ? aof_profile_count(ctx, kernel_id) : -EINVAL;
    if (kept < 0) return -EINVAL;
    if (kept == 0) return fail(ctx, -EINVAL, "kernel %d was not timed", kernel_id);
    return aof_profile_ms(ctx, kernel_id, kept - 1, ms);
}

int aof_ingest_batch_device(const aof_ingest_params *p, const uint8_t *d_camera,
                            int64_t camera_stride, int64_t n_frames, uint8_t *d_cropped,
                            int64_t cropped_stride, uint32_t *d_hist, void *stream)
{
    if (!p || n_frames < 0) return -EINVAL;
    if (p->crop_width < 1 || p->crop_height < 1 || p->crop_width > p->camera_width ||
        p->crop_height > p->camera_height)
        return -EINVAL;
    if (n_frames == 0) return 0;
    if (!d_camera || (!d_cropped && !d_hist)) return -EINVAL;
    if (camera_stride < (int64_t)p->camera_width * p->camera_height && n_frames > 1) return -EINVAL;
    if (d_cropped && cropped_stride < (int64_t)p->crop_width * p->crop_height && n_frames > 1) return -EINVAL;
    if (n_frames * ((p->crop_height + 15) / 16) > 0x7FFFFFFF) return -EINVAL;
    return launch_ingest(*p, d_camera, camera_stride, n_frames, d_cropped, cropped_stride, d_hist, stream)
               ? -EIO : 0;
}

int aof_derotate_batch_device(const aof_derotate_params *p, const aof_flow *d_flows,
                              const aof_gyro *d_gyro, int64_t n, float *d_out, void *stream)
{
    if (!p || n < 0) return -EINVAL;
    if (n == 0) return 0;
    if (!d_flows || !d_gyro || !d_out || (n + 255) / 256 > 0x7FFFFFFF) return -EINVAL;
    return launch_derotate(*p, d_flows, d_gyro, n, d_out, stream) ? -EIO : 0;
}

}  // extern "C"
