// The motion field of a batch (include/aof.h, "the motion FIELD of a batch"), host side: the parameter and geometry checks,
// the launch of k_field.hip behind a batch, and the same function as a plain loop on host memory.  The rule itself is
// aof_field_step.hpp, which the kernel compiles too.  Nothing here synchronises or allocates, and nothing includes the HIP
// runtime: the file also builds for a host-only test program.  Compiled with floating-point contraction off:
// aof_field_host rounds every operation on its own, as the kernel does.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstring>

#include "aof_engine_args.hpp"
#include "aof_field_step.hpp"
#include "aof_host.hpp"

using namespace aof;

// (the three below are declared in aof_host.hpp: the stream bank's motion field, aof_bank_field.cpp, runs them too)
namespace aof {

bool field_bad_params(const aof_field_params *fp)
{
    return !fp || fp->min_blocks < 3 || (fp->passes != 1 && fp->passes != 2) || (fp->exclude_reach != 0 && fp->exclude_reach != 1) ||
           !(fp->gate_px > 0.0f) || !std::isfinite(fp->gate_px);
}

// The geometry of a configuration's level-0 grid, or -EINVAL where the fit does not serve it.
//
// The bound: nb^2 * R^2 < 2^62 with R^2 = Xmax^2 + Ymax^2, Xmax / Ymax the largest |X| / |Y| of the grid.  Why every integer
// the rule forms then fits int64 (n <= nb blocks in a set; |X| <= Xmax, |Y| <= Ymax; |U|, |V| <= 2*128 + 1 = 257, so
// U^2 + V^2 < 364^2):
//   * per block, by Cauchy-Schwarz: X^2 + Y^2 <= R^2, |X*U + Y*V| <= 364 R, |X*V - Y*U| <= 364 R; hence Q <= n R^2 and
//     |A|, |C| <= 364 n R, and |SX| <= n Xmax, |SY| <= n Ymax, |SU|, |SV| <= 257 n;
//   * D = n*Q - SX^2 - SY^2: n*Q <= nb^2 R^2 < 2^62; n*sum(X^2) >= SX^2 and n*sum(Y^2) >= SY^2 (Cauchy-Schwarz again), so
//     both partial differences stay in [0, 2^62);
//   * Na = n*A - SX*SU - SY*SV and Nb = n*C - SX*SV + SY*SU: every partial result is at most
//     n^2 (364 R + 257 Xmax + 257 Ymax) <= 728 n^2 R in magnitude (Xmax + Ymax <= sqrt(2) R).  If R >= 728 that is at most
//     nb^2 R^2 < 2^62.  If R < 728: the X of a row's blocks are distinct integers of one parity within +-Xmax, so
//     nx <= Xmax + 1 <= 728 and likewise ny <= 728, nb <= 728^2, and 728 nb^2 R < 728^6 < 2^58.
// nb >= 1 also gives R < 2^31: X and Y fit int32.
int field_geom(const aof_params *p, const aof_field_params *fp, FieldGeom *out)
{
    if (!p || aof_params_check(p)) return -EINVAL;
    Grid g;
    if (grid_for_level(*p, 0, &g)) return -EINVAL;
    const int64_t cx = 2 * (int64_t)g.x0 + p->tile - p->width, cy = 2 * (int64_t)g.y0 + p->tile - p->height;
    const int64_t ex = cx + 2 * (int64_t)g.step_x * (g.nx - 1), ey = cy + 2 * (int64_t)g.step_y * (g.ny - 1);
    const int64_t xmax = std::max(cx < 0 ? -cx : cx, ex < 0 ? -ex : ex), ymax = std::max(cy < 0 ? -cy : cy, ey < 0 ? -ey : ey);
    const unsigned __int128 nb = (unsigned __int128)((int64_t)g.nx * g.ny);
    const unsigned __int128 r2 = (unsigned __int128)xmax * (unsigned __int128)xmax + (unsigned __int128)ymax * (unsigned __int128)ymax;
    if (nb * nb * r2 >= ((unsigned __int128)1 << 62)) return -EINVAL;
    if (out) {
        std::memset(out, 0, sizeof(*out));
        out->cx = (int32_t)cx; out->cy = (int32_t)cy;
        out->sx2 = 2 * g.step_x; out->sy2 = 2 * g.step_y;
        out->nx = g.nx; out->nb = g.nx * g.ny;
        out->vthr = value_threshold_u16(*p);
        out->reach = p->search;
        if (fp) {
            out->min_blocks = fp->min_blocks; out->passes = fp->passes; out->exclude_reach = fp->exclude_reach;
            out->gate = 2.0 * (double)fp->gate_px;
        }
    }
    return 0;
}

void field_pair(const FieldGeom &g, const aof_block *blocks, const uint8_t *subdirs, const aof_flow &flow, aof_field *out)
{
    const int32_t px = flow.pred_x, py = flow.pred_y;
    auto word = [&](int32_t k) { return (uint32_t)(uint8_t)blocks[k].dx | (uint32_t)(uint8_t)blocks[k].dy << 8 | (uint32_t)blocks[k].sad << 16; };
    FieldSums s1 = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t accepted = 0, at_reach = 0;
    for (int32_t k = 0; k < g.nb; k++) {
        const FieldRecord r = field_record(g, word(k), subdirs ? subdirs[k] : 8u, px, py);
        accepted += r.accepted; at_reach += r.at_reach;
        if (field_member(g, r)) field_add(s1, field_x(g, k % g.nx), field_y(g, k / g.nx), r.U, r.V);
    }
    const FieldModel m1 = field_solve(s1, g.min_blocks);
    if (!m1.fits) { *out = field_publish(accepted, at_reach, 0, nullptr, 0, false); return; }
    if (g.passes == 2) {
        FieldSums s2 = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int32_t k = 0; k < g.nb; k++) {
            const FieldRecord r = field_record(g, word(k), subdirs ? subdirs[k] : 8u, px, py);
            const int32_t X = field_x(g, k % g.nx), Y = field_y(g, k / g.nx);
            if (field_member(g, r) && field_inlier(m1.a, m1.b, m1.tU, m1.tV, g.gate, X, Y, r.U, r.V)) field_add(s2, X, Y, r.U, r.V);
        }
        const FieldModel m2 = field_solve(s2, g.min_blocks);
        if (m2.fits) { *out = field_publish(accepted, at_reach, (uint32_t)s1.n, &m2, (uint32_t)s2.n, true); return; }
    }
    *out = field_publish(accepted, at_reach, (uint32_t)s1.n, &m1, (uint32_t)s1.n, false);
}

}  // namespace aof

extern "C" {

int aof_field_params_default(aof_field_params *fp)
{
    if (!fp) return -EINVAL;
    fp->min_blocks = 8;
    fp->passes = 2;
    fp->exclude_reach = 1;
    fp->gate_px = 1.0f;
    return 0;
}

int aof_field_supported(const aof_params *p) { return field_geom(p, nullptr, nullptr); }

int aof_field_batch_device(aof_ctx *ctx, const aof_field_params *fp, const aof_block *d_blocks, const uint8_t *d_subdirs,
                           const aof_flow *d_flows, int64_t n_pairs, aof_field *d_fields, void *stream)
{
    if (!ctx) return -EINVAL;
    if (!fp || !d_blocks || !d_flows || !d_fields) return ctx_fail(ctx, -EINVAL, "field: null params, block, flow or field pointer");
    if (field_bad_params(fp)) return ctx_fail(ctx, -EINVAL, "field: min_blocks < 3, passes outside 1..2, exclude_reach outside 0..1 or a gate that is not > 0 and finite");
    if (n_pairs < 0 || n_pairs > 0x7FFFFFFF) return ctx_fail(ctx, -EINVAL, "field: n_pairs outside 0..2^31-1");
    if (!aligned(d_blocks, 4) || !aligned(d_flows, 4)) return ctx_fail(ctx, -EINVAL, "field: blocks and flows must be 4-byte aligned");
    if (!aligned(d_fields, 8)) return ctx_fail(ctx, -EINVAL, "field: the field records must be 8-byte aligned");
    aof_params p;
    if (aof_get_params(ctx, &p)) return -EINVAL;
    FieldArgs a;
    std::memset(&a, 0, sizeof(a));
    if (field_geom(&p, fp, &a.g)) return ctx_fail(ctx, -EINVAL, "field: the grid is beyond the fit's integer range (aof_field_supported)");
    if (const int rc = precheck(ctx)) return rc;
    a.blocks = reinterpret_cast<const uint32_t *>(d_blocks);
    a.subdirs = d_subdirs;
    a.flows = reinterpret_cast<const uint32_t *>(d_flows);
    a.fields = d_fields;
    a.n_pairs = n_pairs;
    if (launch_field(a, stream)) return ctx_fail(ctx, -EIO, "field launch failed");
    return 0;
}

int aof_field_host(const aof_params *p, const aof_field_params *fp, const aof_block *blocks, const uint8_t *subdirs,
                   const aof_flow *flows, int64_t n_pairs, aof_field *out)
{
    if (!p || !blocks || !flows || !out || n_pairs < 0 || field_bad_params(fp)) return -EINVAL;
    FieldGeom g;
    if (field_geom(p, fp, &g)) return -EINVAL;
    for (int64_t i = 0; i < n_pairs; i++)
        field_pair(g, blocks + i * g.nb, subdirs ? subdirs + i * g.nb : nullptr, flows[i], out + i);
    return 0;
}

}  // extern "C"
