// The motion-field fit (include/aof.h, "the motion FIELD of a batch"; DESIGN.md "The motion field"), the rule both sides
// run: which records count, where a block sits and how far it moved, the integer sums of a set of blocks, the model in
// double and the gate of the second pass.  The kernel (k_field.hip) and the host loop (aof_field.cpp) compile this text;
// both are built with floating-point contraction off, and the functions that round say so themselves.
//
// Ranges.  aof_field_supported admits a geometry iff nb^2 * (Xmax^2 + Ymax^2) < 2^62 (field_geom, aof_field.cpp, where the
// proof that every sum and product below then fits int64 stands).  With R^2 = Xmax^2 + Ymax^2 that also gives nb * R < 2^31:
// a sum of X, Y, U or V over ANY subset of a pair's blocks fits int32 (|U|, |V| <= 257 and nb <= 2^24), which is what lets
// the kernel's lanes keep n, SX, SY, SU and SV in 32-bit registers.
#pragma once

#include <cstdint>

#include "aof_hd.hpp"

namespace aof {

static_assert(sizeof(aof_field) == 64 && alignof(aof_field) == 8, "one field record is 64 bytes, 8-byte aligned");

struct FieldGeom {
    int32_t cx, cy;        // X of column 0 and Y of row 0: 2*x0 + B - W, 2*y0 + B - H
    int32_t sx2, sy2;      // 2*step_x, 2*step_y
    int32_t nx, nb;        // columns, blocks
    int32_t vthr, reach;   // min(value_threshold, 0xFFFF), S
    int32_t min_blocks, passes, exclude_reach;
    double gate;           // g = 2.0 * (double)gate_px, half-pixels
};

// One record as the rule sees it.  word: the aof_block as one little-endian word (dx | dy << 8 | sad << 16); sd: its
// sub-direction, 8 (or anything above 7) = none; (px, py): the pair's predictor.
struct FieldRecord {
    int32_t U, V;          // 2*dx + hx, 2*dy + hy
    bool accepted, at_reach;
};

AOF_HD_INLINE FieldRecord field_record(const FieldGeom &g, uint32_t word, uint32_t sd, int32_t px, int32_t py)
{
    const int32_t dx = (int8_t)(word & 0xFFu), dy = (int8_t)((word >> 8) & 0xFFu);
    const uint32_t sad = word >> 16;
    // Reduce's table (k_reduce.hip): direction k points at angle k * 45 degrees, 8 = the integer match itself
    const int32_t hx = (sd == 0 || sd == 1 || sd == 7) ? 1 : ((sd == 3 || sd == 4 || sd == 5) ? -1 : 0);
    const int32_t hy = (sd == 1 || sd == 2 || sd == 3) ? 1 : ((sd == 5 || sd == 6 || sd == 7) ? -1 : 0);
    FieldRecord r;
    r.U = 2 * dx + hx;
    r.V = 2 * dy + hy;
    r.accepted = sad != AOF_SAD_SKIPPED && (int32_t)sad < g.vthr;
    const int32_t ex = dx - px, ey = dy - py;
    r.at_reach = r.accepted && (ex == g.reach || ex == -g.reach || ey == g.reach || ey == -g.reach);
    return r;
}

// Is an accepted record a member of M1?
AOF_HD_INLINE bool field_member(const FieldGeom &g, const FieldRecord &r) { return r.accepted && !(g.exclude_reach && r.at_reach); }

AOF_HD_INLINE int32_t field_x(const FieldGeom &g, int32_t bx) { return g.cx + bx * g.sx2; }
AOF_HD_INLINE int32_t field_y(const FieldGeom &g, int32_t by) { return g.cy + by * g.sy2; }

// The three 64-bit terms of one block.
AOF_HD_INLINE int64_t field_q(int32_t X, int32_t Y) { return (int64_t)X * X + (int64_t)Y * Y; }
AOF_HD_INLINE int64_t field_a(int32_t X, int32_t Y, int32_t U, int32_t V) { return (int64_t)X * U + (int64_t)Y * V; }
AOF_HD_INLINE int64_t field_c(int32_t X, int32_t Y, int32_t U, int32_t V) { return (int64_t)X * V - (int64_t)Y * U; }

struct FieldSums {
    int64_t n, SX, SY, SU, SV, Q, A, C;
};

AOF_HD_INLINE void field_add(FieldSums &s, int32_t X, int32_t Y, int32_t U, int32_t V)
{
    s.n += 1; s.SX += X; s.SY += Y; s.SU += U; s.SV += V;
    s.Q += field_q(X, Y); s.A += field_a(X, Y, U, V); s.C += field_c(X, Y, U, V);
}

struct FieldModel {
    int64_t D, Na, Nb;
    double a, b, tU, tV;
    bool fits;
};

// The double finaliser: one rounding per operation, integers converted first.
AOF_HD_INLINE FieldModel field_solve(const FieldSums &s, int32_t min_blocks)
{
#pragma clang fp contract(off)
    FieldModel m;
    m.D = s.n * s.Q - s.SX * s.SX - s.SY * s.SY;
    m.Na = s.n * s.A - s.SX * s.SU - s.SY * s.SV;
    m.Nb = s.n * s.C - s.SX * s.SV + s.SY * s.SU;
    m.fits = s.n >= (int64_t)min_blocks && m.D > 0;
    m.a = m.b = m.tU = m.tV = 0.0;
    if (m.fits) {
        const double n = (double)s.n, SX = (double)s.SX, SY = (double)s.SY, SU = (double)s.SU, SV = (double)s.SV;
        const double D = (double)m.D;
        m.a = (double)m.Na / D;
        m.b = (double)m.Nb / D;
        const double aSX = m.a * SX, bSY = m.b * SY, bSX = m.b * SX, aSY = m.a * SY;
        m.tU = ((SU - aSX) + bSY) / n;
        m.tV = ((SV - bSX) - aSY) / n;
    }
    return m;
}

// The second pass's gate: both residuals within g.  (a, b, tU, tV) come as plain doubles: the kernel's lanes take them
// from LDS, bit for bit what the solving lane stored.
AOF_HD_INLINE bool field_inlier(double a, double b, double tU, double tV, double gate, int32_t X, int32_t Y, int32_t U, int32_t V)
{
#pragma clang fp contract(off)
    const double x = (double)X, y = (double)Y;
    const double aX = a * x, bY = b * y, bX = b * x, aY = a * y;
    const double ru = (double)U - ((tU + aX) - bY);
    const double rv = (double)V - ((tV + bX) + aY);
    return __builtin_fabs(ru) <= gate && __builtin_fabs(rv) <= gate;
}

// The published record.  m == nullptr: M1 did not fit -- all zero except accepted and at_reach.
AOF_HD_INLINE aof_field field_publish(uint32_t accepted, uint32_t at_reach, uint32_t fitted, const FieldModel *m, uint32_t used, bool refit)
{
#pragma clang fp contract(off)
    aof_field f;
    f.det = f.num_zoom = f.num_rot = 0;
    f.accepted = accepted; f.at_reach = at_reach; f.fitted = 0; f.used = 0;
    f.zoom = f.rotation = f.centre_x = f.centre_y = 0.0f;
    f.flags = 0; f.reserved = 0;
    if (m) {
        f.det = m->D; f.num_zoom = m->Na; f.num_rot = m->Nb;
        f.fitted = fitted; f.used = used;
        f.zoom = (float)m->a; f.rotation = (float)m->b;
        f.centre_x = (float)(m->tU * 0.5); f.centre_y = (float)(m->tV * 0.5);
        f.flags = AOF_FIELD_VALID | (refit ? AOF_FIELD_REFIT : 0u);
    }
    return f;
}

// What one launch needs (k_field.hip); by value.
struct FieldArgs {
    FieldGeom g;
    const uint32_t *blocks;    // [n_pairs][nb] records as words, 4-byte aligned
    const uint8_t *subdirs;    // [n_pairs][nb] or nullptr
    const uint32_t *flows;     // [n_pairs] aof_flow as four words (word 3: quality | flags << 8 | pred_x << 16 | pred_y << 24)
    aof_field *fields;         // [n_pairs], 8-byte aligned
    int64_t n_pairs;
    uint32_t div_nx_mul, div_nx_shift;   // fastdiv_make(nx), filled by the launcher
};
int launch_field(const FieldArgs &a, void *stream);   // hipError_t as int

}  // namespace aof
