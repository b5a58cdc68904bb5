// Division by a run-time constant without a divide: the host makes the magic number, the kernels use it
// (fast_div, aof_device.hpp).
#pragma once

#include <cstdint>

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

}  // namespace aof
