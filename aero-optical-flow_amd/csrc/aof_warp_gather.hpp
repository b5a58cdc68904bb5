// The warp's gather on the device, the ONE home of it: the value of a stream's plane at a coordinate of the rule
// (aof_warp_step.hpp), for the warp launch (k_bank_warp.hip) and the one-launch tick with the warp inside it
// (k_bank_tick_warp.hip).  Grey planes fetch a tap row's horizontal pair as ONE 2-byte load (any alignment), every other
// format a byte at a time through warp_pixel.  The bounds proof is the rule's: behind warp_clamp only pixels xi,
// min(xi + 1, xmax) of rows yi, min(yi + 1, ymax) of the plane are read.
#pragma once

#include "aof_warp_step.hpp"

namespace aof {

namespace {

// warp_sample for a grey plane (gb 1): the same four taps, a row's two in one 2-byte load where they are two pixels
// (xi < xmax; at xi == xmax the rule's second tap IS the first).
__device__ __forceinline__ uint32_t sample_grey(const WarpPlane &pl, int32_t X, int32_t Y)
{
    const int32_t xi = X >> AOF_WARP_FRAC_BITS, fx = X & (kWarpOne - 1);
    const int32_t yi = Y >> AOF_WARP_FRAC_BITS, fy = Y & (kWarpOne - 1), y1 = yi + 1 < pl.ymax ? yi + 1 : pl.ymax;
    const uint8_t *r0 = pl.base + (int64_t)yi * pl.pitch + xi, *r1 = pl.base + (int64_t)y1 * pl.pitch + xi;
    uint32_t a, b;
    if (xi < pl.xmax) {
        uint16_t t0, t1;
        __builtin_memcpy(&t0, r0, 2);
        __builtin_memcpy(&t1, r1, 2);
        a = t0; b = t1;
    } else {
        a = r0[0] * 0x101u; b = r1[0] * 0x101u;
    }
    return warp_blend(a & 0xFFu, a >> 8, b & 0xFFu, b >> 8, fx, fy);
}

__device__ __forceinline__ uint32_t sample(const WarpPlane &pl, int32_t X, int32_t Y)
{
    return pl.gb == 1 ? sample_grey(pl, X, Y) : warp_sample(pl, X, Y);   // (gb is uniform)
}

}  // namespace

}  // namespace aof
