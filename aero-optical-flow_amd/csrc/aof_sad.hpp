// The packed-SAD vocabulary of the search kernels (v_qsad_pk_u16_u8 and what goes round it), the 4x4 gradient gate
// and the minimum of a row of packed sums: one definition for the lane-per-block 8x8 search (aof_lane8.hpp), the
// column walk (aof_cols8_kernels.hpp), the coarse level (k_coarse.hip), the one-workgroup kernels (k_flow_small.hip)
// and the 16x16 search (k_search_tile16.hip).  Device-only; internal linkage, like the kernels that use it.
#pragma once

#include "aof_device.hpp"

namespace aof {

namespace {

// Four 4-byte SADs of `ref` against the window's byte offsets 0..3, added to the four u16 lanes of acc.
__device__ __forceinline__ u64 qsad(u64 window, uint32_t ref, u64 acc)
{
    return __builtin_amdgcn_qsad_pk_u16_u8(window, ref, acc);
}
__device__ __forceinline__ u64 pack64(uint32_t lo, uint32_t hi) { return ((u64)hi << 32) | lo; }
// Dwords 1 and 2 of a window row whose dwords (0, 1) and (2, 3) sit in two aligned register pairs: ONE v_pk_mov_b32
// (pack64(w.y, w.z) compiles to it in the exhaustive kernels, but to two v_mov_b32 in the pruned rows).
__device__ __forceinline__ u64 middle64(u64 p01, u64 p23)
{
    u64 r;
    asm("v_pk_mov_b32 %0, %1, %2 op_sel:[1,0]" : "=v"(r) : "v"(p01), "v"(p23));
    return r;
}

__device__ __forceinline__ uint32_t pk_min_u16(uint32_t x, uint32_t y)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(ushort2_t, x),
                                                                  __builtin_bit_cast(ushort2_t, y)));
}

// The smallest of a dy row's 17 partial sums of the 16x16 search (acc: offsets 4g .. 4g+3 as packed u16; acc16: offset
// 16 in the high half) alone -- the lower bounds of the pruned search need no candidate index: packed minima instead of
// 17 keys, 11 instructions against row_key's 25, on every (dy, block) item of every block row.
__device__ __forceinline__ uint32_t row_min17(const u64 (&acc)[4], uint32_t acc16)
{
    const uint32_t m01 = pk_min_u16(pk_min_u16((uint32_t)acc[0], (uint32_t)(acc[0] >> 32)), pk_min_u16((uint32_t)acc[1], (uint32_t)(acc[1] >> 32)));
    const uint32_t m23 = pk_min_u16(pk_min_u16((uint32_t)acc[2], (uint32_t)(acc[2] >> 32)), pk_min_u16((uint32_t)acc[3], (uint32_t)(acc[3] >> 32)));
    const uint32_t m = pk_min_u16(pk_min_u16(m01, m23), acc16 | 0xFFFFu);
    return min(m & 0xFFFFu, m >> 16);
}

// 4x4 gradient gate: the absolute differences between vertical and between horizontal neighbours of a tile's middle
// 4x4 pixels, summed; mid[r] = the four middle bytes of middle row r.
__device__ __forceinline__ uint32_t gradient_gate(const uint32_t (&mid)[4])
{
    uint32_t diff = 0;
#pragma unroll
    for (int r = 0; r < 3; r++) diff = __builtin_amdgcn_sad_u8(mid[r], mid[r + 1], diff);
#pragma unroll
    for (int r = 0; r < 4; r++)  // bytes (3,4,5,5) against (2,3,4,5): the doubled byte adds 0
        diff = __builtin_amdgcn_sad_u8(mid[r], __builtin_amdgcn_perm(0u, mid[r], 0x03030201u), diff);
    return diff;
}
// ... of an 8x8 tile in registers, two dwords per row: tile bytes [2..5] x rows [2..5]
__device__ __forceinline__ uint32_t gradient_gate(const uint32_t (&ref)[8][2])
{
    uint32_t mid[4];
#pragma unroll
    for (int r = 0; r < 4; r++) mid[r] = __builtin_amdgcn_alignbyte(ref[r + 2][1], ref[r + 2][0], 2);
    return gradient_gate(mid);
}

}  // namespace

}  // namespace aof
