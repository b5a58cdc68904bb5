// The warp launch (include/aof.h, "the stream bank with a lens"): a stream's crop resampled through its mesh, and the
// crop's masked exposure histogram, where k_ingest copies a window -- in a camera push with aof_set_bank_warps bound and
// behind aof_ingest_warped_device.  The rule is aof_warp_step.hpp's, which aof_warp_host compiles for the host.
//
// Shaped like k_ingest: 256 lanes, a workgroup per (frame, strip of up to 128 rows); the frame's record comes through the
// scalar path (bank_sensor, aof_bank_stream.hpp) and a workgroup whose record forbids the read leaves before its first
// load.  The strip's nodes are clamped into LDS once (two node rows more than a strip has cells: 17 rows of nx for 128
// rows; the strip, its halving for wide crops and the launch's LDS are warp_plan_make's, aof_warp_plan.hpp).  A lane produces 16 consecutive pixels of a row -- two cells, along which a coordinate advances by one addition
// per pixel -- and stores them as one 16-byte value; crops whose width is no multiple of 16 (or whose destination is
// not aligned) take a lane per pixel.  A gather, not a copy: a pixel is four taps at a place only the mesh knows.  Grey
// planes fetch a tap's horizontal pair as ONE 2-byte load (any alignment), every other format a byte at a time through
// warp_pixel (sample, aof_warp_gather.hpp: shared with the one-launch tick that has the warp inside it); what that costs,
// and what wider fetches were not tried, is in LAB_LOG.md ("Stream bank warp").
// The histogram is exposure_bin's: a lane counts in 12-bit fields of two 64-bit registers (bank_histogram's layout), the
// waves add theirs to the workgroup's ten words, and a workgroup that owns its frame stores them; several strips add
// with integer atomics to words the launcher zeroed.
#include "aof_bank_stream.hpp"   // (bank_sensor, kThreads)
#include "aof_engine_args.hpp"   // (launch_zero_words)
#include "aof_ingest_args.hpp"   // (WarpArgs, launch_warp)
#include "aof_warp_gather.hpp"   // (aof_warp_step.hpp; sample)
#include "aof_warp_plan.hpp"     // (the launch plan and its constants: kLaneItems)

namespace aof {

namespace {

struct LaneBins { unsigned long long lo, hi; };   // bins 0..4, 5..9, 12 bits each

__device__ __forceinline__ void count_bin(LaneBins &n, uint32_t v)
{
    const uint32_t b = (uint32_t)exposure_bin(v);   // 10 for v = 255: counted nowhere
    if (b < 5) n.lo += 1ull << (12 * b);
    else if (b < 10) n.hi += 1ull << (12 * (b - 5));
}

// Every lane of the wave: the wave's ten sums into the workgroup's histogram.
__device__ __forceinline__ void flush_bins(uint32_t *s_hist, LaneBins &n)
{
#pragma unroll
    for (int b = 0; b < AOF_EXPOSURE_BINS; b++) {
        const uint32_t c = wave_sum_u32((uint32_t)((b < 5 ? n.lo >> (12 * b) : n.hi >> (12 * (b - 5))) & 0xFFFu));
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_hist[b], c);
    }
    n.lo = n.hi = 0;
}

__global__ __launch_bounds__(kThreads) void k_bank_warp(WarpArgs a)
{
    extern __shared__ int2 s_nodes[];   // the strip's clamped nodes, [node rows][nx]
    __shared__ uint32_t s_hist[AOF_EXPOSURE_BINS];
    const int strip = blockIdx.x % a.nstrips;
    const int64_t frame = blockIdx.x / a.nstrips;
    const int tid = threadIdx.x;
    const int W = a.crop_w, H = a.crop_h;

    // the frame's plane and its plain crop's origin (x0, y0): the record's, or the call's grey frame with the centred crop
    WarpPlane pl;
    int32_t x0, y0;
    if (a.recs) {   // (uniform: one frame per workgroup; the record's words arrive in scalar registers)
        const BankSensor r = bank_sensor(a.recs, (size_t)frame, W, H, a.base, a.camera_bytes, a.formats);
        if (a.ok && strip == 0 && tid == 0) a.ok[frame] = r.ok ? 1 : 0;
        if (!r.ok) return;
        typedef const u32x4 __attribute__((address_space(4))) *const_words;
        const const_words rec = reinterpret_cast<const_words>(reinterpret_cast<uintptr_t>(a.recs + frame));
        const u32x4 lo = rec[0], hi = rec[1];
        pl.base = a.camera + (int64_t)((uint64_t)lo.x | (uint64_t)lo.y << 32);
        pl.pitch = r.crop.pitch; pl.gb = r.crop.gb; pl.shift = r.crop.shift;
        pl.xmax = warp_last((int32_t)lo.w); pl.ymax = warp_last((int32_t)hi.x);
        x0 = (int32_t)hi.y; y0 = (int32_t)hi.z;
    } else {
        if (a.ok && strip == 0 && tid == 0) a.ok[frame] = 1;
        pl.base = a.camera + frame * a.camera_stride;
        pl.pitch = a.plane_w; pl.gb = 1; pl.shift = 0;
        pl.xmax = warp_last(a.plane_w); pl.ymax = warp_last(a.plane_h);
        x0 = a.plane_w / 2 - W / 2; y0 = a.plane_h / 2 - H / 2;
    }
    if (tid < AOF_EXPOSURE_BINS) s_hist[tid] = 0;

    const int row_begin = strip * a.strip_rows, row_end = min(H, row_begin + a.strip_rows);
    const int cy0 = row_begin >> 3, node_rows = ((row_end - 1) >> 3) + 2 - cy0;
    const int2 *mesh = reinterpret_cast<const int2 *>(a.points + frame * (int64_t)a.nx * a.ny);
    // not warped: the plain crop of the record, pixel by pixel through the same stores and the same histogram
    const bool none = __builtin_amdgcn_readfirstlane(mesh[0].x) == AOF_WARP_NONE;
    if (!none) {
        for (int i = tid; i < node_rows * a.nx; i += kThreads) {
            const int2 p = mesh[(int64_t)cy0 * a.nx + i];
            s_nodes[i] = make_int2(warp_clamp(p.x, pl.xmax), warp_clamp(p.y, pl.ymax));
        }
    }
    __syncthreads();

    const WarpMask m = warp_mask(W, H);
    uint8_t *dst = a.cropped ? a.cropped + frame * a.cropped_stride : nullptr;
    // crop pixel (x, y) of an unwarped frame
    auto plain = [&](int x, int y) __attribute__((always_inline)) {
        return warp_pixel(pl.base + (int64_t)(y0 + y) * pl.pitch, x0 + x, pl.gb, pl.shift);
    };

    if (a.vec) {   // W % 16 == 0 and an aligned destination: 16 pixels, two cells, per lane and trip
        const int pieces = W / 16, items = (row_end - row_begin) * pieces;
        LaneBins bins = {0, 0};
        int trips = 0;
        for (int base = 0; base < items; base += kThreads, trips++) {   // (uniform trip count: the flushes are wave-wide)
            const int it = base + tid;
            if (it < items) {
                const int y = row_begin + it / pieces, x = (it % pieces) * 16;
                const int j = y & 7;
                const int2 *n0 = s_nodes + ((y >> 3) - cy0) * a.nx + (x >> 3), *n1 = n0 + a.nx;
                uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    const int2 A = n0[c], B = n0[c + 1], C = n1[c], D = n1[c + 1];
                    const WarpEdge ex = warp_edge(A.x, B.x, C.x, D.x, j), ey = warp_edge(A.y, B.y, C.y, D.y, j);
                    int32_t nxv = kWarpCell * ex.left, nyv = kWarpCell * ey.left;
                    const int32_t sx = ex.right - ex.left, sy = ey.right - ey.left;
#pragma unroll
                    for (int i = 0; i < 8; i++, nxv += sx, nyv += sy) {
                        const int k = 8 * c + i;
                        const uint32_t v = none ? plain(x + k, y) : sample(pl, warp_round(nxv), warp_round(nyv));
                        w[k >> 2] |= v << (8 * (k & 3));
                    }
                }
                if (dst) *reinterpret_cast<uint4 *>(dst + (int64_t)y * W + x) = make_uint4(w[0], w[1], w[2], w[3]);
                if (a.hist && y >= m.y0 && y < m.y1 && x + 16 > m.x0 && x < m.x1) {
#pragma unroll
                    for (int k = 0; k < 16; k++)
                        if (x + k >= m.x0 && x + k < m.x1) count_bin(bins, (w[k >> 2] >> (8 * (k & 3))) & 0xFFu);
                }
            }
            if (a.hist && trips % kLaneItems == kLaneItems - 1) flush_bins(s_hist, bins);
        }
        if (a.hist) flush_bins(s_hist, bins);
    } else {
        const int items = (row_end - row_begin) * W;
        for (int it = tid; it < items; it += kThreads) {
            const int y = row_begin + it / W, x = it % W;
            uint32_t v;
            if (none) {
                v = plain(x, y);
            } else {
                const int i = x & 7, j = y & 7;
                const int2 *n0 = s_nodes + ((y >> 3) - cy0) * a.nx + (x >> 3), *n1 = n0 + a.nx;
                v = sample(pl, warp_coord(n0[0].x, n0[1].x, n1[0].x, n1[1].x, i, j), warp_coord(n0[0].y, n0[1].y, n1[0].y, n1[1].y, i, j));
            }
            if (dst) dst[(int64_t)y * W + x] = (uint8_t)v;
            if (a.hist && y >= m.y0 && y < m.y1 && x >= m.x0 && x < m.x1) {
                const int b = exposure_bin(v);
                if (b < AOF_EXPOSURE_BINS) atomicAdd(&s_hist[b], 1u);
            }
        }
    }
    if (!a.hist) return;
    __syncthreads();
    if (tid < AOF_EXPOSURE_BINS) {
        if (a.nstrips == 1) a.hist[frame * AOF_EXPOSURE_BINS + tid] = s_hist[tid];   // the workgroup owns the frame
        else if (s_hist[tid]) atomicAdd(&a.hist[frame * AOF_EXPOSURE_BINS + tid], s_hist[tid]);
    }
}

}  // namespace

int launch_warp(const WarpArgs &args, int64_t n_frames, void *stream)
{
    if (n_frames == 0) return 0;
    const WarpPlan plan = warp_plan_make(args.crop_w, args.crop_h, n_frames, reinterpret_cast<uintptr_t>(args.cropped), args.cropped_stride,
                                         args.hist != nullptr);
    if (plan.verdict != WARP_OK) return (int)hipErrorInvalidValue;
    WarpArgs a = args;
    a.nx = plan.nx; a.ny = plan.ny;
    a.strip_rows = plan.strip_rows; a.nstrips = plan.nstrips;
    a.vec = plan.vec;
    if (plan.zero_hist) {   // several workgroups add to a frame's histogram
        const int rc = launch_zero_words(a.hist, n_frames * AOF_EXPOSURE_BINS, stream);
        if (rc) return rc;
    }
    if (plan.attr) {   // (aof_small_plan.hpp: dynamic LDS beyond 48 KiB needs the function attribute)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_bank_warp), hipFuncAttributeMaxDynamicSharedMemorySize, kNodeBytesMax);
        if (e != hipSuccess) return e == hipErrorInvalidValue ? (int)hipErrorLaunchFailure : (int)e;   // (invalid value is the plan's refusal)
    }
    hipLaunchKernelGGL(k_bank_warp, dim3((uint32_t)plan.wgs), dim3(kThreads), plan.lds, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

}  // namespace aof
