// The warp rule (csrc/aof_warp_step.hpp -- include/aof.h "the stream bank with a lens") and the mesh builders and the
// one-frame host form around it (csrc/aof_warp.cpp), compiled for the host under UBSan and ASan and held to ONE
// restatement in 64-bit integers: extreme nodes (INT32_MIN + 1, INT32_MAX and everything next to the clamp's edges),
// planes of 1 x 1, planes wider and taller than the 32 768 pixels a node can name, crops of 1 x 1 and 9 x 17, every pixel
// format.  The planes are allocated at their exact size: a tap outside a plane ends the run, as does a step that
// wrapped or a conversion that left its type.  The builders: identity meshes next to the ends of int32 against 64-bit
// arithmetic, the lens helper on coefficients that are huge, infinite or no number.
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "aof_bank_tables.hpp"
#include "aof_host.hpp"
#include "aof_ingest_args.hpp"
#include "aof_warp_step.hpp"

// what aof_warp.cpp's device-side entry points link against: not called here
namespace aof {
static BankCtx g_bank;
BankCtx &bank_ctx(aof_ctx *) { return g_bank; }
int ctx_fail(aof_ctx *, int code, const char *) { return code; }
int launch_warp(const WarpArgs &, int64_t, void *) { return 1; }
}  // namespace aof

static long checked = 0;
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the header's table of formats: the grey value of pixel x of a row
static int64_t grey64(const uint8_t *row, int64_t x, int format)
{
    switch (format) {
    case 0: return row[x];
    case 1: case 2: case 4: case 5: case 6: {
        const int shift = format == 1 ? 0 : format == 2 ? 8 : format == 4 ? 2 : format == 5 ? 4 : 6;
        return (((int64_t)row[2 * x] | (int64_t)row[2 * x + 1] << 8) >> shift) & 0xFF;
    }
    case 7: return row[(x / 4) * 5 + x % 4];
    default: return row[(x / 2) * 3 + x % 2];
    }
}

// The rule of include/aof.h for crop pixel (x, y), all in 64 bits.
static int64_t wide(const uint8_t *plane, int64_t pitch, int format, int64_t width, int64_t height, const aof_warp_point *nodes, int64_t nx,
                    int64_t x, int64_t y)
{
    const int64_t xmax = width - 1 < 32767 ? width - 1 : 32767, ymax = height - 1 < 32767 ? height - 1 : 32767;
    const int64_t cx = x >> 3, cy = y >> 3, i = x & 7, j = y & 7;
    int64_t P[2];
    for (int axis = 0; axis < 2; axis++) {
        const int64_t hi = (axis ? ymax : xmax) * 32;
        auto node = [&](int64_t c, int64_t r) {
            const aof_warp_point &p = nodes[r * nx + c];
            return clamp64(axis ? p.y : p.x, 0, hi);
        };
        const int64_t N = (8 - i) * (8 - j) * node(cx, cy) + i * (8 - j) * node(cx + 1, cy) + (8 - i) * j * node(cx, cy + 1) + i * j * node(cx + 1, cy + 1);
        P[axis] = (N + 32) >> 6;
    }
    const int64_t xi = P[0] >> 5, fx = P[0] & 31, x1 = xi + 1 < xmax ? xi + 1 : xmax;
    const int64_t yi = P[1] >> 5, fy = P[1] & 31, y1 = yi + 1 < ymax ? yi + 1 : ymax;
    const uint8_t *r0 = plane + yi * pitch, *r1 = plane + y1 * pitch;
    return (grey64(r0, xi, format) * (32 - fx) * (32 - fy) + grey64(r0, x1, format) * fx * (32 - fy) + grey64(r1, xi, format) * (32 - fx) * fy +
            grey64(r1, x1, format) * fx * fy + 512) >> 10;
}

// A node coordinate for an axis whose last pixel is `last`: the ends of int32 and both sides of both edges of the clamp.
static int32_t edge_value(int64_t last)
{
    const int64_t hi = last * 32;
    const int64_t v[] = {INT32_MIN + 1ll, INT32_MIN + 2ll, -1000000, -33, -1, 0, 1, 15, 16, 31, 32, 33, hi / 2, hi - 33, hi - 32, hi - 1, hi, hi + 1, hi + 31,
                         hi + 32, 2 * hi + 5, 1ll << 30, INT32_MAX - 1ll, INT32_MAX};
    int64_t pick = v[rnd() % (sizeof(v) / sizeof(v[0]))];
    if (rnd() % 4 == 0) pick = (int64_t)(rnd() % (uint64_t)(hi + 64)) - 32;
    return (int32_t)clamp64(pick, INT32_MIN + 1ll, INT32_MAX);
}

// One plane of `format`, width x height, rows `pitch` apart at `offset` in a buffer of exactly its extent; crops of w x h
// through `rounds` meshes of edge values: every pixel by warp_pixel_through and the whole frame by aof_warp_host against
// the restatement.  Returns the number of differences.
static long plane_case(int format, int32_t width, int32_t height, int32_t pad, int32_t w, int32_t h, int rounds)
{
    const aof::BankPixelLayout l = aof::bank_pixel_layout((uint32_t)format);
    const int64_t row_bytes = (int64_t)(width / l.group_px) * l.group_bytes, pitch = row_bytes + pad, offset = 3;
    const size_t bytes = (size_t)(offset + (int64_t)(height - 1) * pitch + row_bytes);
    std::vector<uint8_t> heap(bytes);
    for (size_t k = 0; k < bytes; k++) heap[k] = (uint8_t)(rnd() >> 32);
    for (size_t k = 0; k < bytes; k += 5) heap[k] = 255;
    const int32_t nx = aof::warp_nodes(w), ny = aof::warp_nodes(h);
    if (nx != (w + 7) / 8 + 1 || ny != (h + 7) / 8 + 1) return 1;
    aof_bank_sensor rec;
    std::memset(&rec, 0, sizeof(rec));
    rec.offset = (uint64_t)offset; rec.pitch = (int32_t)pitch; rec.width = width; rec.height = height;
    const bool crop_fits = w <= width && h <= height;   // (the record's own rule: the plain crop at (0, 0))
    std::vector<aof_warp_point> mesh((size_t)nx * ny);
    std::vector<uint8_t> out((size_t)w * h), guard((size_t)w * h + 64, 0xEE);
    long bad = 0;
    for (int r = 0; r < rounds; r++) {
        for (auto &p : mesh) { p.x = edge_value(aof::warp_last(width)); p.y = edge_value(aof::warp_last(height)); }
        const aof::WarpPlane pl = {heap.data() + offset, (int32_t)pitch, l.group_bytes, l.shift, aof::warp_last(width), aof::warp_last(height)};
        uint32_t want_hist[AOF_EXPOSURE_BINS] = {0};
        const aof::WarpMask m = aof::warp_mask(w, h);
        for (int32_t y = 0; y < h; y++) {
            for (int32_t x = 0; x < w; x++, checked++) {
                const int64_t want = wide(heap.data() + offset, pitch, format, width, height, mesh.data(), nx, x, y);
                if (want < 0 || want > 255 || (int64_t)aof::warp_pixel_through(pl, mesh.data(), nx, x, y) != want) bad++;
                out[(size_t)y * w + x] = (uint8_t)want;
                if (y >= m.y0 && y < m.y1 && x >= m.x0 && x < m.x1 && want * 10 / 255 < 10) want_hist[want * 10 / 255]++;
            }
        }
        uint32_t hist[AOF_EXPOSURE_BINS];
        const int rc = aof_warp_host(w, h, heap.data(), bytes, &rec, (uint8_t)format, mesh.data(), guard.data(), hist);
        if (rc != (crop_fits ? 1 : 0)) bad++;
        if (rc == 1 && (std::memcmp(guard.data(), out.data(), out.size()) != 0 || std::memcmp(hist, want_hist, sizeof(hist)) != 0)) bad++;
        for (size_t k = out.size(); k < guard.size(); k++) bad += guard[k] != 0xEE;
        if (rc == 1 && aof_warp_host(w, h, heap.data(), bytes - 1, &rec, (uint8_t)format, mesh.data(), guard.data(), hist) != 0) bad++;   // one byte short: refused
    }
    return bad;
}

static long builders()
{
    long bad = 0;
    aof_params p;
    std::memset(&p, 0, sizeof(p));
    const int32_t sizes[][2] = {{1, 1}, {9, 17}, {64, 64}, {INT32_MAX, 1}};
    for (const auto &s : sizes) {
        p.width = s[0]; p.height = s[1];
        int32_t nx = 0, ny = 0;
        if (aof_warp_mesh_size(&p, &nx, &ny) || nx != (int32_t)(((int64_t)s[0] + 7) / 8 + 1) || ny != (int32_t)(((int64_t)s[1] + 7) / 8 + 1)) bad++;
        checked++;
    }
    p.width = 0;
    int32_t nx, ny;
    if (aof_warp_mesh_size(&p, &nx, &ny) != -EINVAL) bad++;
    p.width = 9; p.height = 17;
    aof_warp_mesh_size(&p, &nx, &ny);
    std::vector<aof_warp_point> mesh((size_t)nx * ny), kept;
    const int32_t origins[] = {INT32_MIN, INT32_MIN / 32 - 1, INT32_MIN / 32, INT32_MIN / 32 + 1, -1, 0, 7, INT32_MAX / 32 - 32, INT32_MAX / 32 - 17, INT32_MAX / 32 - 16,
                               INT32_MAX / 32 - 15, INT32_MAX / 32, INT32_MAX};
    for (int32_t x0 : origins) {
        for (int32_t y0 : origins) {
            for (auto &q : mesh) q = aof_warp_point{77, 77};
            const int rc = aof_warp_mesh_identity(&p, x0, y0, mesh.data());
            bool fits = true;
            for (int32_t cy = 0; cy < ny; cy++)
                for (int32_t cx = 0; cx < nx; cx++) {
                    const int64_t X = ((int64_t)x0 + 8 * cx) * 32, Y = ((int64_t)y0 + 8 * cy) * 32;
                    fits = fits && X > INT32_MIN && X <= INT32_MAX && Y >= INT32_MIN && Y <= INT32_MAX;
                }
            if (rc != (fits ? 0 : -EINVAL)) bad++;
            for (int32_t cy = 0; cy < ny; cy++)
                for (int32_t cx = 0; cx < nx; cx++, checked++) {
                    const aof_warp_point q = mesh[(size_t)cy * nx + cx];
                    if (fits ? (q.x != ((int64_t)x0 + 8 * cx) * 32 || q.y != ((int64_t)y0 + 8 * cy) * 32) : (q.x != 77 || q.y != 77)) bad++;
                }
        }
    }
    // the lens helper: whatever the coefficients, every node is an int32 made by a conversion that stays in range
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double values[] = {0.0, -0.3, 1.0, 1e300, -1e300, 1e-300, inf, -inf, nan};
    for (double a : values) {
        for (double b : values) {
            aof_lens l = {70.0, 70.0, 4.5, 8.5, a, b, a, b, a, 70.0, 70.0, 4.5, 8.5};
            if (aof_warp_mesh_from_lens(&p, &l, mesh.data())) bad++;
            if (mesh[0].x == AOF_WARP_NONE) bad++;
            l.fx = a; l.cy = b;
            if (aof_warp_mesh_from_lens(&p, &l, mesh.data())) bad++;
            l.out_fx = a;
            const bool usable = std::isfinite(a) && a != 0.0;
            if (aof_warp_mesh_from_lens(&p, &l, mesh.data()) != (usable ? 0 : -EINVAL)) bad++;
            checked += 3;
        }
    }
    // without coefficients and with equal cameras: the identity mesh at the principal points' difference
    aof_lens l = {70.0, 71.0, 4.5 + 12, 8.5 + 5, 0, 0, 0, 0, 0, 70.0, 71.0, 4.5, 8.5};
    kept.resize(mesh.size());
    if (aof_warp_mesh_from_lens(&p, &l, mesh.data()) || aof_warp_mesh_identity(&p, 12, 5, kept.data()) ||
        std::memcmp(mesh.data(), kept.data(), mesh.size() * sizeof(aof_warp_point)) != 0)
        bad++;
    return bad;
}

int main()
{
    long bad = 0;
    const int formats[] = {0, 1, 2, 4, 5, 6, 7, 8};
    for (int f : formats) {
        bad += plane_case(f, 4, 1, 0, 1, 1, 40);      // (four pixels: one group of every format)
        bad += plane_case(f, 12, 7, 3, 9, 17, 12);    // the crop larger than the plane: warp_pixel_through still, aof_warp_host refuses
        bad += plane_case(f, 24, 20, 1, 9, 17, 12);
    }
    bad += plane_case(0, 1, 1, 0, 1, 1, 60);          // a plane of one pixel: every tap is that pixel
    bad += plane_case(0, 1, 1, 5, 9, 17, 10);
    bad += plane_case(0, 32771, 2, 0, 9, 17, 20);     // wider than a node can name: pixel 32767 replicates
    bad += plane_case(0, 2, 32771, 1, 9, 17, 20);     // and taller
    bad += plane_case(1, 32770, 1, 0, 1, 1, 40);
    bad += plane_case(7, 32772, 3, 2, 9, 17, 10);
    bad += builders();
    if (bad) {
        std::printf("warp_selftest: %ld differences in %ld checks\n", bad, checked);
        return 1;
    }
    std::printf("warp_selftest: the rule, the host form and the builders agree with the 64-bit restatement in %ld checks\n", checked);
    return 0;
}
