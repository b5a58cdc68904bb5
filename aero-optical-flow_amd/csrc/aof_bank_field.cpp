// The stream bank's motion field (include/aof.h, "the stream bank's motion field"), host side: the argument checks, where
// a bank keeps the tick's block records (the bank's own bank_layout and the engine's aof_workspace_layout: nothing about
// either is restated here), the geometry of the fit (field_geom, aof_field.cpp), the launch of k_bank_field.hip behind a
// push, and the same function as a plain loop on host memory over field_pair and the step.  The step itself is
// aof_bank_field_step.hpp, which the kernel compiles too.  Nothing here synchronises or allocates, and nothing includes the
// HIP runtime: the file also builds for a host-only test program.  Compiled with floating-point contraction off:
// aof_bank_field_host rounds every operation on its own, as the kernel does.
#include <cerrno>
#include <cstring>

#include "aof_bank_args.hpp"
#include "aof_bank_calls.hpp"
#include "aof_bank_field_step.hpp"
#include "aof_bank_tables.hpp"
#include "aof_host.hpp"

using namespace aof;

namespace {

BankFieldTick tick_of(const aof_tick_record &r)
{
    return BankFieldTick{r.quality, r.dt_us, r.frame, r.pixel.pred_x, r.pixel.pred_y};
}

}  // namespace

extern "C" {

int aof_bank_field_reset_device(aof_ctx *ctx, int32_t n_streams, const uint8_t *d_mask, aof_bank_field_state *d_state, void *stream)
{
    if (!ctx) return -EINVAL;
    if (!d_state) return ctx_fail(ctx, -EINVAL, "bank field reset: null state pointer");
    if (n_streams < 1) return ctx_fail(ctx, -EINVAL, "bank field reset: n_streams < 1");
    if (!aligned(d_state, 8)) return ctx_fail(ctx, -EINVAL, "bank field reset: the state must be 8-byte aligned");
    if (const int rc = precheck(ctx)) return rc;
    // a reset record is 64 zero bytes under the mask: what the IMU's reset kernel stores for a time offset of 0
    static_assert(sizeof(aof_bank_field_state) == sizeof(aof_imu_state) && alignof(aof_bank_field_state) == alignof(aof_imu_state),
                  "the two per-stream records are reset by one kernel");
    if (launch_bank_imu_reset(reinterpret_cast<aof_imu_state *>(d_state), d_mask, (uint32_t)n_streams, 0, stream))
        return ctx_fail(ctx, -EIO, "bank field reset launch failed");
    return 0;
}

int aof_bank_field_device(aof_ctx *ctx, const aof_bank_params *bp, const aof_field_params *fp, const void *d_bank, size_t bank_bytes,
                          const aof_tick_record *d_records, aof_bank_field_state *d_state, aof_field *d_fields,
                          aof_bank_field_record *d_out, void *stream)
{
    if (!ctx) return -EINVAL;
    if (!bp || !fp || !d_bank || !d_records || !d_state || !d_out)
        return ctx_fail(ctx, -EINVAL, "bank field: null bank params, field params, bank, record, state or output pointer");
    if (bp->n_streams < 1) return ctx_fail(ctx, -EINVAL, "bank field: n_streams < 1");
    if (field_bad_params(fp))
        return ctx_fail(ctx, -EINVAL, "bank field: min_blocks < 3, passes outside 1..2, exclude_reach outside 0..1 or a gate that is not > 0 and finite");
    aof_params p;
    if (aof_get_params(ctx, &p)) return -EINVAL;
    BankFieldArgs a;
    std::memset(&a, 0, sizeof(a));
    if (field_geom(&p, fp, &a.g)) return ctx_fail(ctx, -EINVAL, "bank field: the grid is beyond the fit's integer range (aof_field_supported)");
    BankLayout L;
    aof_ws_layout W;
    int rc = bank_layout(&p, bp, &L);
    if (!rc) rc = aof_workspace_layout(&p, bp->n_streams, &W);
    if (rc) return ctx_fail(ctx, rc, "bank field: bad bank parameters (n_streams, frame_stride, focal length)");
    if (!aligned(d_bank, 256)) return ctx_fail(ctx, -EINVAL, "bank field: the bank must be 256-byte aligned");
    if (!aligned(d_records, 4) || !aligned(d_out, 4)) return ctx_fail(ctx, -EINVAL, "bank field: tick and output records must be 4-byte aligned");
    if (!aligned(d_state, 8) || !aligned(d_fields, 8)) return ctx_fail(ctx, -EINVAL, "bank field: state and fields must be 8-byte aligned");
    // a bound per-stream array (aof_set_bank_streams) gives every stream its own focal lengths; it is for one stream count
    const BankTables &tables = bank_ctx(ctx).tables;
    if (bank_table_differs(tables, kBankStreams, bp->n_streams))
        return ctx_fail(ctx, -EINVAL, "bank field: n_streams differs from the array bound with aof_set_bank_streams");
    if (bank_bytes < L.pub.total_bytes) return ctx_fail(ctx, -ENOSPC, "bank field: bank smaller than aof_bank_layout().total_bytes");
    if ((rc = precheck(ctx))) return rc;

    const uint8_t *scratch = static_cast<const uint8_t *>(d_bank) + L.pub.scratch;
    a.blocks = reinterpret_cast<const uint32_t *>(scratch + W.l0_blocks);
    a.subdirs = p.subpixel ? scratch + W.l0_subdirs : nullptr;
    a.records = reinterpret_cast<const uint32_t *>(d_records);
    a.state = d_state;
    a.fields = d_fields;
    a.out = d_out;
    a.streams = static_cast<const aof_bank_stream *>(tables.table[kBankStreams].array);
    a.focal_x = bp->focal_x;
    a.focal_y = bp->focal_y;
    a.n_streams = bp->n_streams;
    if (launch_bank_field(a, stream)) return ctx_fail(ctx, -EIO, "bank field launch failed");
    return 0;
}

int aof_bank_field_host(const aof_params *p, const aof_bank_params *bp, const aof_bank_stream *streams, const aof_field_params *fp,
                        const aof_block *blocks, const uint8_t *subdirs, const aof_tick_record *records, aof_bank_field_state *state,
                        aof_field *fields, aof_bank_field_record *out)
{
    if (!p || !bp || !blocks || !records || !state || !out || bp->n_streams < 1 || field_bad_params(fp)) return -EINVAL;
    FieldGeom g;
    if (field_geom(p, fp, &g)) return -EINVAL;
    if (!p->subpixel) subdirs = nullptr;   // sub-directions belong to a sub-pixel context
    for (int32_t s = 0; s < bp->n_streams; s++) {
        const BankFieldTick r = tick_of(records[s]);
        const bool pair = bank_field_pair(r);
        aof_field f;
        std::memset(&f, 0, sizeof(f));
        if (pair) field_pair(g, blocks + (size_t)s * g.nb, subdirs ? subdirs + (size_t)s * g.nb : nullptr, records[s].pixel, &f);
        if (fields) fields[s] = f;
        if (bank_field_no_frame(r.quality)) { out[s] = bank_field_record_zero(r.quality); continue; }
        out[s] = bank_field_step(r, pair, f, streams ? streams[s].focal_x : bp->focal_x, streams ? streams[s].focal_y : bp->focal_y, state[s]);
    }
    return 0;
}

}  // extern "C"
