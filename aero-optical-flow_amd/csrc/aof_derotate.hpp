// The published PX4Flow gyro compensation of ONE flow record (include/aof.h, "gyro de-rotation"), shared by
// k_derotate.hip (aof_derotate_batch_device) and the stream bank's tail lane (k_bank.hip), so that a pair's de-rotated
// flow cannot depend on the entry point that computed it.  Three float operations per axis with FMA contraction
// switched off for the block: every operation rounds once and the device result is bit-identical to the host
// arithmetic.  (Plain operators on purpose: __fmul_rn/__fadd_rn are inline functions whose bodies keep the
// translation unit's default contraction and fuse after inlining.)
#pragma once

#include "aof.h"
#include "aof_device.hpp"

namespace aof {

__device__ __forceinline__ void derotate_flow(const aof_derotate_params &p, const aof_flow &f, const aof_gyro &g, float *out_x,
                                              float *out_y)
{
#pragma clang fp contract(off)
    const float lim = p.rate_threshold * g.dt_s;
    float x = f.flow_x, y = f.flow_y;
    if (fabsf(g.integ_y) > lim) {
        const float pix = g.integ_y * p.focal_x;
        x = f.flow_x + pix;
        x = x < -p.max_flow ? -p.max_flow : (x > p.max_flow ? p.max_flow : x);
    }
    if (fabsf(g.integ_x) > lim) {
        const float pix = g.integ_x * p.focal_y;
        y = f.flow_y - pix;
        y = y < -p.max_flow ? -p.max_flow : (y > p.max_flow ? p.max_flow : y);
    }
    *out_x = x;
    *out_y = y;
}

}  // namespace aof
