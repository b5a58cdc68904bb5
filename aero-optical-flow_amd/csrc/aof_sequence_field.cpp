// The sequence pipeline's motion field (include/aof_sequence_field.h), host side: the argument checks, where a sequence call
// leaves every pair's block records (aof_sequence_layout, the limiter's buffers of aof_sequence_args.hpp and the engine's
// aof_workspace_layout: nothing about them is restated here), the launch of the fit (k_field.hip's own launcher, so that a
// pair's record is aof_field_batch_device's by construction) and of the window pass (k_sequence_field.hip) behind it, and the
// same function as a plain SEQUENTIAL loop on host memory: one aof_bank_field_state walked frame by frame with the bank's step
// (aof_bank_field_step.hpp), as a one-stream bank is pushed.  The kernel restates that loop in parallel (DESIGN.md section 2,
// "Sequence motion field"); this file does not.  Nothing here synchronises or allocates, and nothing includes the HIP runtime:
// the file also builds for a host-only test program.  Compiled with floating-point contraction off: every operation is
// rounded on its own, as in the kernel.
#include <cerrno>
#include <cstring>

#include "aof_host.hpp"
#include "aof_sequence_args.hpp"
#include "aof_sequence_field_args.hpp"

using namespace aof;

extern "C" {

int aof_sequence_field_device(aof_ctx *ctx, const aof_sequence_params *sp, const aof_field_params *fp, int64_t n_frames,
                              void *d_workspace, size_t workspace_bytes, aof_field *d_fields, aof_bank_field_record *d_out,
                              aof_bank_field_state *d_state_out, void *stream)
{
    if (!ctx) return -EINVAL;
    if (!sp || !fp || !d_workspace || !d_out)
        return ctx_fail(ctx, -EINVAL, "sequence field: null sequence params, field params, workspace or output pointer");
    if (field_bad_params(fp))
        return ctx_fail(ctx, -EINVAL, "sequence field: min_blocks < 3, passes outside 1..2, exclude_reach outside 0..1 or a gate that is not > 0 and finite");
    aof_params p;
    int rc = aof_get_params(ctx, &p);
    if (rc) return rc;
    FieldArgs fit;
    std::memset(&fit, 0, sizeof(fit));
    if (field_geom(&p, fp, &fit.g)) return ctx_fail(ctx, -EINVAL, "sequence field: the grid is beyond the fit's integer range (aof_field_supported)");
    aof_seq_layout L;
    rc = aof_sequence_layout(&p, sp, n_frames, &L);
    if (rc) return ctx_fail(ctx, rc, "sequence field: sequence parameters do not match the context (crop size, frame count)");
    if (!d_fields && n_frames > 1) return ctx_fail(ctx, -EINVAL, "sequence field: null field records with more than one frame");
    if (!aligned(d_workspace, 256)) return ctx_fail(ctx, -EINVAL, "sequence field: the workspace must be 256-byte aligned");
    if (!aligned(d_fields, 8) || !aligned(d_state_out, 8) || !aligned(d_out, 4))
        return ctx_fail(ctx, -EINVAL, "sequence field: fields and state must be 8-byte aligned, the output records 4-byte aligned");
    if (workspace_bytes < L.total_bytes) return ctx_fail(ctx, -ENOSPC, "sequence field: workspace smaller than aof_sequence_layout().total_bytes");
    if ((rc = precheck(ctx))) return rc;
    if (n_frames == 0) return 0;

    const uint8_t *ws = static_cast<const uint8_t *>(d_workspace);
    if (n_frames > 1) {
        // the flow engine's workspace of the n - 1 pairs, behind the limiter's buffers
        aof_ws_layout W;
        rc = aof_workspace_layout(&p, n_frames - 1, &W);
        if (rc) return ctx_fail(ctx, rc, "sequence field: no workspace layout for the recording's pairs");
        const uint8_t *flow_ws = ws + L.scratch + sequence_flow_ws_offset(n_frames);
        fit.blocks = reinterpret_cast<const uint32_t *>(flow_ws + W.l0_blocks);
        fit.subdirs = p.subpixel ? flow_ws + W.l0_subdirs : nullptr;
        fit.flows = reinterpret_cast<const uint32_t *>(ws + L.flows);
        fit.fields = d_fields;
        fit.n_pairs = n_frames - 1;
        if (launch_field(fit, stream)) return ctx_fail(ctx, -EIO, "sequence field: fit launch failed");
    }
    SeqFieldArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n_frames = n_frames;
    a.count = reinterpret_cast<const uint32_t *>(ws + L.count);
    a.records = reinterpret_cast<const aof_seq_record *>(ws + L.records);
    a.fields = n_frames > 1 ? d_fields : nullptr;
    a.out = d_out;
    a.state = d_state_out;
    a.focal_x = sp->focal_x; a.focal_y = sp->focal_y;
    if (launch_sequence_field(a, stream)) return ctx_fail(ctx, -EIO, "sequence field: window launch failed");
    return 0;
}

int aof_sequence_field_host(const aof_params *p, const aof_sequence_params *sp, const aof_field_params *fp, int64_t n_frames,
                            const aof_block *blocks, const uint8_t *subdirs, const aof_flow *flows, const aof_seq_record *records,
                            uint32_t n_records, aof_field *fields, aof_bank_field_record *out, aof_bank_field_state *state_out)
{
    if (!p || !sp || !out || field_bad_params(fp)) return -EINVAL;
    if (n_frames < 0 || n_frames >= 0x7FFFFFF0ll || (int64_t)n_records > n_frames) return -EINVAL;
    if (n_frames > 1 && (!blocks || !flows || !fields)) return -EINVAL;
    if (!records && n_records > 0) return -EINVAL;
    if (!(sp->focal_x > 0.0f) || !(sp->focal_y > 0.0f)) return -EINVAL;
    FieldGeom g;
    if (field_geom(p, fp, &g)) return -EINVAL;
    for (uint32_t m = 0; m < n_records; m++)
        if ((int64_t)records[m].frame >= n_frames || (m > 0 && records[m].frame <= records[m - 1].frame)) return -EINVAL;
    if (n_frames == 0) return 0;
    if (!p->subpixel) subdirs = nullptr;   // sub-directions belong to a sub-pixel context

    aof_bank_field_state st;
    std::memset(&st, 0, sizeof(st));
    uint32_t m = 0;   // the first record not yet met
    for (int64_t j = 0; j < n_frames; j++) {
        const bool pair = j >= 1;
        aof_field f;
        std::memset(&f, 0, sizeof(f));
        if (pair) {
            const size_t k = (size_t)(j - 1);
            field_pair(g, blocks + k * g.nb, subdirs ? subdirs + k * g.nb : nullptr, flows[k], &f);
            fields[k] = f;
        }
        const bool record = m < n_records && (int64_t)records[m].frame == j;
        const aof_bank_field_record o = bank_field_step(seq_field_tick(record, (uint32_t)j, record ? records[m].dt_us : 0), pair, f,
                                                        sp->focal_x, sp->focal_y, st);
        if (record) out[m++] = o;
    }
    if (state_out) *state_out = st;
    return 0;
}

}  // extern "C"
