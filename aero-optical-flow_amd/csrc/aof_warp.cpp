// The warp meshes of the stream bank (include/aof.h, "the stream bank with a lens"), host side: the mesh builders, the
// one-frame host form of the rule (aof_warp_step.hpp, the header the kernel compiles), the binding call and the
// stateless device entry point.  Nothing here allocates or synchronises; the camera pushes' use of the binding is
// bank_push's (aof_bank.cpp).
#include <cerrno>
#include <cmath>
#include <cstdint>

#include "aof_bank_tables.hpp"
#include "aof_host.hpp"
#include "aof_ingest_args.hpp"
#include "aof_warp_step.hpp"

using namespace aof;

namespace {

// floor(v * 32 + 0.5) saturated to int32 (a NaN: 0).
int32_t node_unit(double v)
{
    const double r = std::floor(v * 32.0 + 0.5);
    if (!(r == r)) return 0;
    if (r <= (double)INT32_MIN) return INT32_MIN;
    if (r >= (double)INT32_MAX) return INT32_MAX;
    return (int32_t)r;
}

bool mesh_size(const aof_params *p, int32_t *nx, int32_t *ny)
{
    if (!p || p->width < 1 || p->height < 1) return false;
    *nx = warp_nodes(p->width);
    *ny = warp_nodes(p->height);
    return true;
}

}  // namespace

extern "C" {

int aof_warp_mesh_size(const aof_params *p, int32_t *nx, int32_t *ny)
{
    if (!nx || !ny) return -EINVAL;
    return mesh_size(p, nx, ny) ? 0 : -EINVAL;
}

int aof_warp_mesh_identity(const aof_params *p, int32_t x0, int32_t y0, aof_warp_point *out)
{
    int32_t nx, ny;
    if (!out || !mesh_size(p, &nx, &ny)) return -EINVAL;
    // (64 bits: the last node of either axis decides whether every node is an int32)
    const int64_t last_x = ((int64_t)x0 + (int64_t)kWarpCell * (nx - 1)) * kWarpOne, last_y = ((int64_t)y0 + (int64_t)kWarpCell * (ny - 1)) * kWarpOne;
    const int64_t first_x = (int64_t)x0 * kWarpOne, first_y = (int64_t)y0 * kWarpOne;
    if (first_x <= INT32_MIN || first_y < INT32_MIN || last_x > INT32_MAX || last_y > INT32_MAX) return -EINVAL;   // (x: AOF_WARP_NONE is no coordinate)
    for (int32_t cy = 0; cy < ny; cy++)
        for (int32_t cx = 0; cx < nx; cx++)
            out[(int64_t)cy * nx + cx] = aof_warp_point{(int32_t)(first_x + (int64_t)kWarpCell * kWarpOne * cx), (int32_t)(first_y + (int64_t)kWarpCell * kWarpOne * cy)};
    return 0;
}

int aof_warp_mesh_from_lens(const aof_params *p, const aof_lens *lens, aof_warp_point *out)
{
    int32_t nx, ny;
    if (!out || !lens || !mesh_size(p, &nx, &ny)) return -EINVAL;
    const aof_lens &l = *lens;
    if (!std::isfinite(l.out_fx) || !std::isfinite(l.out_fy) || l.out_fx == 0.0 || l.out_fy == 0.0) return -EINVAL;
    for (int32_t cy = 0; cy < ny; cy++) {
        for (int32_t cx = 0; cx < nx; cx++) {
            const double u = (double)(kWarpCell * (int64_t)cx), v = (double)(kWarpCell * (int64_t)cy);
            const double xn = (u - l.out_cx) / l.out_fx, yn = (v - l.out_cy) / l.out_fy;
            const double r2 = xn * xn + yn * yn;
            const double rad = 1.0 + r2 * (l.k1 + r2 * (l.k2 + r2 * l.k3));
            const double xd = xn * rad + 2.0 * l.p1 * xn * yn + l.p2 * (r2 + 2.0 * xn * xn);
            const double yd = yn * rad + l.p1 * (r2 + 2.0 * yn * yn) + 2.0 * l.p2 * xn * yn;
            out[(int64_t)cy * nx + cx] = aof_warp_point{node_unit(l.fx * xd + l.cx), node_unit(l.fy * yd + l.cy)};
        }
    }
    if (out[0].x == AOF_WARP_NONE) out[0].x = AOF_WARP_NONE + 1;   // (a coordinate, not the mark: both clamp to 0)
    return 0;
}

int aof_set_bank_warps(aof_ctx *ctx, const aof_warp_point *d_points, int32_t n_streams)
{
    if (!ctx) return -EINVAL;
    if (const char *what = bank_warps_bind(&bank_ctx(ctx).warps, d_points, n_streams)) return ctx_fail(ctx, -EINVAL, what);
    return 0;
}

int aof_ingest_warped_device(int32_t crop_width, int32_t crop_height, const uint8_t *d_camera, uint64_t camera_bytes,
                             const aof_bank_sensor *d_sensors, const uint8_t *d_formats, const aof_warp_point *d_points,
                             int64_t n_frames, uint8_t *d_cropped, int64_t cropped_stride, uint32_t *d_hist, uint8_t *d_ok,
                             void *stream)
{
    if (crop_width < 1 || crop_height < 1 || n_frames < 0) return -EINVAL;
    if (n_frames == 0) return 0;
    if (!d_camera || !d_sensors || !aligned(d_sensors, 16) || camera_bytes == 0 || (!d_cropped && !d_hist)) return -EINVAL;
    if (!d_points || !aligned(d_points, 16)) return -EINVAL;
    if (d_cropped && cropped_stride < (int64_t)crop_width * crop_height && n_frames > 1) return -EINVAL;
    if (n_frames * ((crop_height + 7) / 8) > 0x7FFFFFFF) return -EINVAL;
    WarpArgs a = {};
    a.crop_w = crop_width; a.crop_h = crop_height;
    a.camera = d_camera;
    a.recs = d_sensors; a.base = 0; a.camera_bytes = camera_bytes; a.formats = d_formats;
    a.points = d_points;
    a.cropped = d_cropped; a.cropped_stride = cropped_stride;
    a.hist = d_hist; a.ok = d_ok;
    const int rc = launch_warp(a, n_frames, stream);
    return rc == 1 /* hipErrorInvalidValue: a crop too wide */ ? -EINVAL : (rc ? -EIO : 0);
}

int aof_warp_host(int32_t crop_width, int32_t crop_height, const uint8_t *camera, uint64_t camera_bytes,
                  const aof_bank_sensor *sensor, uint8_t format, const aof_warp_point *points, uint8_t *cropped, uint32_t *hist)
{
    if (crop_width < 1 || crop_height < 1 || !camera || !sensor || !points || (!cropped && !hist)) return -EINVAL;
    const aof_bank_sensor &r = *sensor;
    if (!bank_sensor_valid_format(r.offset, r.pitch, r.width, r.height, r.x0, r.y0, crop_width, crop_height, 0, camera_bytes, format, 1))
        return 0;
    const BankPixelLayout l = bank_pixel_layout(format);
    const WarpPlane pl = {camera + r.offset, r.pitch, l.group_bytes, l.shift, warp_last(r.width), warp_last(r.height)};
    const int32_t nx = warp_nodes(crop_width);
    const bool none = points[0].x == AOF_WARP_NONE;
    const WarpMask m = warp_mask(crop_width, crop_height);
    if (hist)
        for (int b = 0; b < AOF_EXPOSURE_BINS; b++) hist[b] = 0;
    for (int32_t y = 0; y < crop_height; y++) {
        for (int32_t x = 0; x < crop_width; x++) {
            const uint32_t v = none ? warp_pixel(camera + r.offset + (int64_t)(r.y0 + y) * r.pitch, r.x0 + x, l.group_bytes, l.shift)
                                    : warp_pixel_through(pl, points, nx, x, y);
            if (cropped) cropped[(int64_t)y * crop_width + x] = (uint8_t)v;
            if (hist && y >= m.y0 && y < m.y1 && x >= m.x0 && x < m.x1) {
                const int b = exposure_bin(v);
                if (b < AOF_EXPOSURE_BINS) hist[b]++;
            }
        }
    }
    return 1;
}

}  // extern "C"
