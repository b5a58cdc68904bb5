// The stream bank's outbox (include/aof.h, "the stream bank's outbox"), host side: the layout, the argument checks and
// the one launch of k_bank_outbox.hip behind a push, and the pinned host memory an outbox may live in.  The call reads
// the push's output arrays only: it knows nothing about the bank.  Nothing here synchronises; only
// aof_outbox_alloc_host allocates.
#include <cerrno>
#include <cstring>

#include "aof_bank_calls.hpp"
#include "aof_ctx.hpp"
#include "aof_host.hpp"

using namespace aof;

namespace {

constexpr uint32_t kMaxCapacity = 0x7FFFFFFFu;

int outbox_layout(uint32_t capacity_messages, uint32_t capacity_exposures, struct aof_outbox_layout *L)
{
    if (capacity_messages > kMaxCapacity || capacity_exposures > kMaxCapacity) return -EINVAL;
    L->messages = sizeof(aof_outbox_header);
    L->exposures = L->messages + (size_t)capacity_messages * sizeof(aof_outbox_entry);
    L->total_bytes = L->exposures + (size_t)capacity_exposures * sizeof(aof_outbox_exposure);
    return 0;
}

}  // namespace

extern "C" {

int aof_outbox_layout(uint32_t capacity_messages, uint32_t capacity_exposures, struct aof_outbox_layout *out)
{
    if (!out) return -EINVAL;
    return outbox_layout(capacity_messages, capacity_exposures, out);
}

int aof_bank_collect_device(aof_ctx *ctx, int32_t n_streams, int32_t n_rounds, const aof_tick_record *d_records,
                            const uint8_t *d_mavlink, const uint8_t *d_mavlink_len, const aof_exposure_record *d_exposure,
                            const float *d_derotated, uint32_t capacity_messages, uint32_t capacity_exposures, void *outbox,
                            size_t outbox_bytes, uint64_t tag, const uint64_t *d_tag, void *stream)
{
    if (!ctx) return -EINVAL;
    if (!d_records || !outbox) return ctx_fail(ctx, -EINVAL, "bank collect: null record or outbox pointer");
    if (n_streams < 1) return ctx_fail(ctx, -EINVAL, "bank collect: n_streams < 1");
    if (n_rounds < 1 || n_rounds > AOF_BANK_BURST_MAX)
        return ctx_fail(ctx, -EINVAL, "bank collect: n_rounds outside 1..AOF_BANK_BURST_MAX");
    const int64_t n = (int64_t)n_streams * n_rounds;
    if (n > 0x7FFFFFFF) return ctx_fail(ctx, -EINVAL, "bank collect: more than 2^31 - 1 records");
    if (!aligned(outbox, 64)) return ctx_fail(ctx, -EINVAL, "bank collect: the outbox must be 64-byte aligned");
    if (d_mavlink && !d_mavlink_len) return ctx_fail(ctx, -EINVAL, "bank collect: MAVLink frames need their length array");
    if (!tag && !d_tag) return ctx_fail(ctx, -EINVAL, "bank collect: the tag must be non-zero");
    if (!aligned(d_records, 4) || !aligned(d_exposure, 4) || !aligned(d_derotated, 4) || !aligned(d_tag, 8))
        return ctx_fail(ctx, -EINVAL, "bank collect: records, exposure records and de-rotated pairs must be 4-byte aligned, the tag word 8-byte aligned");
    struct aof_outbox_layout L;
    if (outbox_layout(capacity_messages, capacity_exposures, &L))
        return ctx_fail(ctx, -EINVAL, "bank collect: a capacity above 2^31 - 1");
    if (outbox_bytes < L.total_bytes) return ctx_fail(ctx, -ENOSPC, "outbox smaller than aof_outbox_layout().total_bytes");
    if (const int rc = precheck(ctx)) return rc;

    OutboxArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n = (uint32_t)n;
    a.n_streams = (uint32_t)n_streams;
    a.records = reinterpret_cast<const uint8_t *>(d_records);
    a.mavlink = d_mavlink;
    a.mavlink_len = d_mavlink_len;
    a.exposure = reinterpret_cast<const uint8_t *>(d_exposure);
    a.derotated = reinterpret_cast<const uint8_t *>(d_derotated);
    a.cap_messages = capacity_messages;
    a.cap_exposures = capacity_exposures;
    a.outbox = static_cast<uint8_t *>(outbox);
    a.messages = a.outbox + L.messages;
    a.exposures = a.outbox + L.exposures;
    a.tag = tag;
    a.d_tag = reinterpret_cast<const unsigned long long *>(d_tag);
    a.counter = ctx->outbox_counter;
    if (launch_bank_outbox(a, stream)) return ctx_fail(ctx, -EIO, "bank outbox launch failed");
    return 0;
}

int aof_outbox_alloc_host(size_t bytes, void **out)
{
    if (!out) return -EINVAL;
    *out = nullptr;
    if (!bytes) return -EINVAL;
    void *p = nullptr, *d = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
        (void)hipGetLastError();
        return -ENOMEM;
    }
    // one pointer for both sides: what the kernels store to is what the host polls
    if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess || d != p) {
        (void)hipGetLastError();
        (void)hipHostFree(p);
        return -ENOMEM;
    }
    *out = p;
    return 0;
}

int aof_outbox_free_host(void *p)
{
    if (!p) return 0;
    return hipHostFree(p) == hipSuccess ? 0 : -EINVAL;
}

}  // extern "C"
