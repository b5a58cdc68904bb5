// The one-launch tick with the lens inside it (include/aof.h, "the stream bank with a lens"): the camera form of
// k_bank_tick (k_bank.hip) with the stream's warp mesh in front of the new frame -- a camera push with aof_set_bank_warps
// bound stays ONE launch per round, and the staging region is neither read nor written.
//   k_bank_tick_warped   one workgroup of 256 lanes per stream.  The idle exit and the bad-sensor exit come before any
//                  frame load, by the tick's own bank_source / bank_gate / bank_idle; the sensor rule alone decides
//                  AOF_TICK_BAD_SENSOR, whatever the mesh says.  The stream's plane is its record's (the records pointer
//                  may be null: then the grey camera_width x camera_height frame at camera + s * camera_stride, whose
//                  unwarped crop is the centred one), as k_bank_warp has it.
//                  A stream whose first node has x == AOF_WARP_NONE (uniform) takes the plain crop of its record through
//                  flow_small_pair's pitched / packed fetch, exactly as k_bank_tick<..., BankSensors> does.
//                  A warped stream: the mesh's nx * ny nodes are clamped (warp_clamp) into LDS once, behind the plan's
//                  dynamic LDS; a lane produces 16 consecutive pixels of a crop row -- two cells: warp_edge, then one
//                  addition per pixel, warp_round, four taps (sample, aof_warp_gather.hpp), warp_blend --, adds their
//                  byte sum to its share of the frame's pixel sum and stores one 16-byte value into LDS buffer 1 of
//                  flow_small_pair's layout.  The pair then runs with that buffer "filled by the caller" (the FILLED
//                  seam of flow_small_pair): its sums and its level-1 image are made as ever, both searches, the
//                  histogram from the LDS copy on a due frame, bank_tail<true> by one lane, store_slot out of LDS.  A
//                  first frame: gather -> LDS -> slot, histogram, tail.
//                  The bounds proof is k_bank_warp's: behind the clamp only pixels xi, min(xi + 1, xmax) of rows yi,
//                  min(yi + 1, ymax) of a valid record's plane are read; the nodes read are node (y >> 3, x >> 3) and its
//                  three neighbours for x <= w - 16 + 15, y <= h - 1, all inside (w / 8 + 1) x ((h - 1) / 8 + 2).
// (count, round) are k_bank_commit's: a stream is active iff round < count[s]; with a null count the `active` mask
// decides.  A warped camera burst of K rounds on this path is K launches with round_args' pointers (aof_bank.cpp): one
// launch per round, byte-identical to K ticks by construction.
#include "aof_bank_args.hpp"
#include "aof_bank_stream.hpp"
#include "aof_engine_args.hpp"
#include "aof_warp_gather.hpp"

namespace aof {

namespace {

// What the kernel takes beside the tick's arguments.
struct WarpTick {
    const aof_warp_point *points;   // [S][ny][nx], 16-byte aligned
    int32_t nx, ny;
    int32_t plane_h;                // no records bound: the rows of the call's grey frame (its width is cam.pitch)
    uint32_t nodes_at;              // byte offset of the clamped nodes in the dynamic LDS (small_warp_plan_make)
    const uint8_t *count;           // a burst's round: [S] frames per stream, or nullptr: a.active decides
    int32_t round;
};

template <bool SUBPIXEL>
__global__ __launch_bounds__(kThreads) void k_bank_tick_warped(SmallArgs sm, BankArgs a, BankSensors sen, WarpTick wt)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_mem[];
    __shared__ aof_flow s_record;
    __shared__ uint8_t s_payload[kMavlinkPayloadBytes];
    __shared__ uint32_t s_hist[AOF_EXPOSURE_BINS];
    const uint32_t s = blockIdx.x;   // (the launcher: one workgroup per stream)
    const int tid = threadIdx.x;
    if (wt.count ? wt.round >= (int32_t)wt.count[s] : (a.active && a.active[s] == 0)) {   // (uniform)
        if (tid == 0) bank_idle<true>(a, s);
        return;
    }
    // (uniform: with a sensor array bound, the stream's record)
    const BankSource from = sen.recs ? bank_source<true>(a, s, 0, sen) : bank_source<true>(a, s, 0);
    const uint8_t *src = from.src;
    uint8_t *slot = a.bank_frames + (int64_t)s * a.frame_stride;
    uint8_t *lds_new = s_mem + a.frame_bytes + kPad;
    const uint32_t gate = bank_gate(a, s, from.ok);   // (uniform)
    if (gate & kGateBadSensor) {             // as early as the idle exit, and like it in front of any frame load
        if (tid == 0) bank_idle<true>(a, s, AOF_TICK_BAD_SENSOR);
        return;
    }

    const int W = a.cam.crop_w, H = a.cam.crop_h;
    const int2 *mesh = reinterpret_cast<const int2 *>(wt.points + (int64_t)s * wt.nx * wt.ny);
    const bool none = __builtin_amdgcn_readfirstlane(mesh[0].x) == AOF_WARP_NONE;   // not warped: the tick as it is
    uint32_t filled = 0, lane_sum = 0;
    if (!none) {
        // the stream's plane: the record's, or the call's grey frame
        WarpPlane pl;
        if (sen.recs) {   // (uniform; the record's words arrive in scalar registers)
            typedef const u32x4 __attribute__((address_space(4))) *const_words;
            const const_words rec = reinterpret_cast<const_words>(reinterpret_cast<uintptr_t>(sen.recs + s));
            const u32x4 lo = rec[0], hi = rec[1];
            pl.base = a.cam.camera + (int64_t)((uint64_t)lo.x | (uint64_t)lo.y << 32);
            pl.pitch = from.crop.pitch; pl.gb = from.crop.gb; pl.shift = from.crop.shift;
            pl.xmax = warp_last((int32_t)lo.w); pl.ymax = warp_last((int32_t)hi.x);
        } else {
            pl.base = a.cam.camera + (int64_t)s * a.cam.camera_stride;
            pl.pitch = a.cam.pitch; pl.gb = 1; pl.shift = 0;
            pl.xmax = warp_last(a.cam.pitch); pl.ymax = warp_last(wt.plane_h);
        }
        int2 *s_nodes = reinterpret_cast<int2 *>(s_mem + wt.nodes_at);
        for (int i = tid; i < wt.nx * wt.ny; i += kThreads) {
            const int2 p = mesh[i];
            s_nodes[i] = make_int2(warp_clamp(p.x, pl.xmax), warp_clamp(p.y, pl.ymax));
        }
        __syncthreads();
        const int pieces = W / 16, items = H * pieces;   // (the one-workgroup class: W is a multiple of 16)
        for (int it = tid; it < items; it += kThreads) {
            const int y = it / pieces, x = (it - y * pieces) * 16;
            const int j = y & 7;
            const int2 *n0 = s_nodes + (y >> 3) * wt.nx + (x >> 3), *n1 = n0 + wt.nx;
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
                    w[k >> 2] |= sample(pl, warp_round(nxv), warp_round(nyv)) << (8 * (k & 3));
                }
            }
            lane_sum = byte_sum(w[0], lane_sum); lane_sum = byte_sum(w[1], lane_sum);
            lane_sum = byte_sum(w[2], lane_sum); lane_sum = byte_sum(w[3], lane_sum);
            *reinterpret_cast<uint4 *>(lds_new + y * W + x) = make_uint4(w[0], w[1], w[2], w[3]);
        }
        filled = 2u;
    }

    if (gate & kGateFirst) {
        if (none) {
            crop_first_frame(a.cam, src, from.crop, lds_new, slot);
        } else {
            __syncthreads();
            store_slot(a, slot, lds_new);
        }
        if (gate & kGateDue) bank_histogram(a.cam, lds_new, s_hist);
        if (tid == 0) bank_tail<true>(a, s, aof_flow{}, true, s_payload, s_hist);
        return;
    }
    // (a warped stream: buffer 1 is in LDS already, pass A fetches the stored frame alone)
    flow_small_pair<SUBPIXEL, true, true, true>(sm, s, slot, src, 1, 3u, &s_record, from.crop, 2u, true, filled, lane_sum);
    // (run_level's last barrier is behind every read of the frames; s_hist is nobody else's)
    if (gate & kGateDue) bank_histogram(a.cam, lds_new, s_hist);
    __syncthreads();
    if (tid == 0) bank_tail<true>(a, s, s_record, false, s_payload, s_hist);
    store_slot(a, slot, lds_new);
}

}  // namespace

int launch_bank_tick_warped(const SmallArgs &sm, const BankArgs &a, const BankSensors &sen, const aof_warp_point *points, int32_t plane_h,
                            void *stream, const uint8_t *count, int32_t round)
{
    if (!bank_plan_fits(sm, a) || !a.cam.camera || !points || sen.bins) return (int)hipErrorInvalidValue;
    const int32_t nx = warp_nodes(a.cam.crop_w), ny = warp_nodes(a.cam.crop_h);
    const SmallWarpPlan plan = small_warp_plan_make(sm, (int64_t)nx * ny);
    if (!plan.ok) return (int)hipErrorInvalidValue;
    const WarpTick wt = {points, nx, ny, plane_h, (uint32_t)plan.nodes_at, count, round};
    void (*fn)(SmallArgs, BankArgs, BankSensors, WarpTick) = sm.l0.subpixel ? k_bank_tick_warped<true> : k_bank_tick_warped<false>;
    if (plan.attr) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)(kSmallLdsLimit - kSmallStaticLds));
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(fn, dim3((uint32_t)a.n_streams), dim3(kThreads), plan.lds, static_cast<hipStream_t>(stream), sm, a, sen, wt);
    return (int)hipGetLastError();
}

}  // namespace aof
