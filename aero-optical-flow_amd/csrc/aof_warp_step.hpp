// The warp of a stream's crop through its mesh (include/aof.h, "the stream bank with a lens"), the ONE place its
// arithmetic is written: k_bank_warp.hip runs it per lane, aof_warp_host (aof_warp.cpp) per pixel, and
// tests/native/warp_selftest.cpp holds it to a 64-bit restatement.  32-bit integers throughout; the clamp in front makes
// every later step small: a clamped node is at most 32767 * 32 < 2^20, a cell's weights sum to 64 (N < 2^26), a tap's
// weights to 1024 (the sum below 2^18).
#pragma once

#include "aof_bank_sensor_rule.hpp"
#include "aof_exposure_step.hpp"

namespace aof {

constexpr int32_t kWarpCell = AOF_WARP_CELL;            // crop pixels between two nodes
constexpr int32_t kWarpOne = 1 << AOF_WARP_FRAC_BITS;   // a sensor pixel in node units
constexpr int32_t kWarpLastMax = 32767;                 // the largest pixel index a node can name

// Nodes along an axis of `size` >= 1 crop pixels: (size + 7) / 8 + 1, written so that no size wraps.
AOF_HD_INLINE int32_t warp_nodes(int32_t size) { return (size - 1) / kWarpCell + 2; }

// xmax / ymax of a plane axis of `size` >= 1 pixels.
AOF_HD_INLINE int32_t warp_last(int32_t size) { return size - 1 < kWarpLastMax ? size - 1 : kWarpLastMax; }

// A node coordinate into [0, last * 32]: never invalid, the border replicates.
AOF_HD_INLINE int32_t warp_clamp(int32_t v, int32_t last)
{
    const int32_t hi = last * kWarpOne;
    return v < 0 ? 0 : (v > hi ? hi : v);
}

// A cell on one axis, for row j of it: the left and the right edge's coordinate, times 8.  Pixel i of the row is
// N = (8 - i) * left + i * right = 8 * left + i * (right - left): the rule's N, and a row advances by one addition.
struct WarpEdge { int32_t left, right; };
AOF_HD_INLINE WarpEdge warp_edge(int32_t a, int32_t b, int32_t c, int32_t d, int32_t j)
{
    return WarpEdge{(kWarpCell - j) * a + j * c, (kWarpCell - j) * b + j * d};
}
AOF_HD_INLINE int32_t warp_round(int32_t n) { return (n + 32) >> 6; }
// X of pixel (i, j) of the cell with the clamped corners a, b (upper) and c, d (lower).
AOF_HD_INLINE int32_t warp_coord(int32_t a, int32_t b, int32_t c, int32_t d, int32_t i, int32_t j)
{
    const WarpEdge e = warp_edge(a, b, c, d, j);
    return warp_round((kWarpCell - i) * e.left + i * e.right);
}

// The grey value of pixel x of the row whose first group starts at `row`: crop_pixel of aof_crop.hpp (which is the
// kernels' alone: it sits behind the HIP runtime's qualifiers), for every AOF_PIXEL_* by its group bytes and shift.
AOF_HD_INLINE uint32_t warp_pixel(const uint8_t *row, int32_t x, int32_t gb, int32_t shift)
{
    if (gb == 1) return row[x];
    if (gb == 2) return (((uint32_t)row[2 * (int64_t)x] | (uint32_t)row[2 * (int64_t)x + 1] << 8) >> shift) & 0xFFu;
    if (gb == 5) return row[(int64_t)(x >> 2) * 5 + (x & 3)];
    return row[(int64_t)(x >> 1) * 3 + (x & 1)];
}

// A stream's grey plane: pixel (0, 0)'s group at `base`, rows `pitch` bytes apart, the format's group bytes and shift.
struct WarpPlane {
    const uint8_t *base;
    int32_t pitch, gb, shift;
    int32_t xmax, ymax;   // warp_last of its width and height
};

// The four taps' weighted mean.
AOF_HD_INLINE uint32_t warp_blend(uint32_t p00, uint32_t p10, uint32_t p01, uint32_t p11, int32_t fx, int32_t fy)
{
    const uint32_t ux = (uint32_t)fx, uy = (uint32_t)fy, gx = (uint32_t)kWarpOne - ux, gy = (uint32_t)kWarpOne - uy;
    return (p00 * gx * gy + p10 * ux * gy + p01 * gx * uy + p11 * ux * uy + 512u) >> 10;
}

// The plane's value at (X, Y), both inside [0, last * 32]: reads pixels xi, min(xi + 1, xmax) of rows yi, min(yi + 1, ymax)
// and nothing else.
AOF_HD_INLINE uint32_t warp_sample(const WarpPlane &pl, int32_t X, int32_t Y)
{
    const int32_t xi = X >> AOF_WARP_FRAC_BITS, fx = X & (kWarpOne - 1), x1 = xi + 1 < pl.xmax ? xi + 1 : pl.xmax;
    const int32_t yi = Y >> AOF_WARP_FRAC_BITS, fy = Y & (kWarpOne - 1), y1 = yi + 1 < pl.ymax ? yi + 1 : pl.ymax;
    const uint8_t *r0 = pl.base + (int64_t)yi * pl.pitch, *r1 = pl.base + (int64_t)y1 * pl.pitch;
    return warp_blend(warp_pixel(r0, xi, pl.gb, pl.shift), warp_pixel(r0, x1, pl.gb, pl.shift), warp_pixel(r1, xi, pl.gb, pl.shift),
                      warp_pixel(r1, x1, pl.gb, pl.shift), fx, fy);
}

// Crop pixel (x, y) through the mesh `nodes` ([..][nx], UNclamped, row 0 = node row 0): the whole rule for one pixel.
AOF_HD_INLINE uint32_t warp_pixel_through(const WarpPlane &pl, const aof_warp_point *nodes, int32_t nx, int32_t x, int32_t y)
{
    const int32_t cx = x >> 3, cy = y >> 3, i = x & 7, j = y & 7;
    const aof_warp_point *n0 = nodes + (int64_t)cy * nx + cx, *n1 = n0 + nx;
    const int32_t X = warp_coord(warp_clamp(n0[0].x, pl.xmax), warp_clamp(n0[1].x, pl.xmax), warp_clamp(n1[0].x, pl.xmax),
                                 warp_clamp(n1[1].x, pl.xmax), i, j);
    const int32_t Y = warp_coord(warp_clamp(n0[0].y, pl.ymax), warp_clamp(n0[1].y, pl.ymax), warp_clamp(n1[0].y, pl.ymax),
                                 warp_clamp(n1[1].y, pl.ymax), i, j);
    return warp_sample(pl, X, Y);
}

// The exposure mask of a crop (mainloop.cpp:203-206, clipped): the centred 128 x 128 region.
struct WarpMask { int32_t x0, y0, x1, y1; };
AOF_HD_INLINE WarpMask warp_mask(int32_t w, int32_t h)
{
    int32_t x0 = w / 2 - AOF_EXPOSURE_MASK_SIZE / 2, y0 = h / 2 - AOF_EXPOSURE_MASK_SIZE / 2;
    int32_t x1 = x0 + AOF_EXPOSURE_MASK_SIZE, y1 = y0 + AOF_EXPOSURE_MASK_SIZE;
    return WarpMask{x0 < 0 ? 0 : x0, y0 < 0 ? 0 : y0, x1 > w ? w : x1, y1 > h ? h : y1};
}

}  // namespace aof
