// The one-workgroup small pair shared by the kernels of k_flow_small.hip (batch, tagged per-call and resident forms)
// and by the stream bank's tick kernel (k_bank.hip): one or two levels of a pair whose frames fit LDS and whose grids
// have at most 256 blocks, passes A..D (DESIGN.md "Kernels": KS).  One function for all of them, so that the pixel
// record of a pair cannot depend on the entry point that computed it.
#pragma once

#include "aof_crop.hpp"
#include "aof_device.hpp"
#include "aof_engine_args.hpp"
#include "aof_reduce.hpp"
#include "aof_refine.hpp"
#include "aof_sad.hpp"
#include "aof_small_plan.hpp"   // kThreads, kMaxBins, kLoads, kPad; the launch plan

namespace aof {

namespace {

// Unaligned reads from an LDS frame: aligned dwords, funnel-shifted by the byte offset's low bits.
__device__ __forceinline__ uint4 lds_bytes16(const uint8_t *frame, int off)
{
    const uint32_t *q = reinterpret_cast<const uint32_t *>(frame) + (off >> 2);
    const uint32_t sh = (uint32_t)off & 3u;
    const uint32_t q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4];
    return make_uint4(__builtin_amdgcn_alignbyte(q1, q0, sh), __builtin_amdgcn_alignbyte(q2, q1, sh),
                      __builtin_amdgcn_alignbyte(q3, q2, sh), __builtin_amdgcn_alignbyte(q4, q3, sh));
}
__device__ __forceinline__ void lds_bytes8(const uint8_t *frame, int off, uint32_t (&out)[2])
{
    const uint32_t *q = reinterpret_cast<const uint32_t *>(frame) + (off >> 2);
    const uint32_t sh = (uint32_t)off & 3u;
    const uint32_t q0 = q[0], q1 = q[1], q2 = q[2];
    out[0] = __builtin_amdgcn_alignbyte(q1, q0, sh);
    out[1] = __builtin_amdgcn_alignbyte(q2, q1, sh);
}
__device__ __forceinline__ void lds_bytes12(const uint8_t *frame, int off, uint32_t (&out)[3])
{
    const uint32_t *q = reinterpret_cast<const uint32_t *>(frame) + (off >> 2);
    const uint32_t sh = (uint32_t)off & 3u;
    const uint32_t q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    out[0] = __builtin_amdgcn_alignbyte(q1, q0, sh);
    out[1] = __builtin_amdgcn_alignbyte(q2, q1, sh);
    out[2] = __builtin_amdgcn_alignbyte(q3, q2, sh);
}

struct LevelMeta { int px, py, delta; };

// One level of one pair out of LDS: search, records, refinement, votes, flow record.
// `keys`: one packed key per block; `record_out`: LDS copy of the flow record (level 1: it carries the
// predictor); `pred_rec`: the level-1 record whose predictor fields level 0 copies into its own.
template <bool SUBPIXEL>
__device__ __forceinline__ void run_level(const SearchArgs &a, const FlowTail &tail, uint32_t pair, const uint8_t *fp,
                                          const uint8_t *fc, const LevelMeta &m, uint32_t *keys,
                                          uint32_t (*votes)[kMaxBins], int *tot, aof_flow *record_out,
                                          const aof_flow *pred_rec)
{
    const int tid = threadIdx.x, W = a.w;
    const int nb = a.grid.blocks(), nx = a.grid.nx;
    const int centre = 2 * tail.range + 1;
    constexpr int ring = SUBPIXEL ? 1 : 0;
    for (int k = tid; k < nb; k += kThreads) keys[k] = 0xFFFFFFFFu;
    if (tid < kMaxBins) { votes[0][tid] = 0; votes[1][tid] = 0; }
    if (tid < 3) tot[tid] = 0;
    __syncthreads();

    // ---- C: one lane per (block, dy) ----
    for (int it = tid; it < nb * 9; it += kThreads) {
        const int blk = it / 9, d = it - blk * 9;
        const int by = blk / nx, bx = blk - by * nx;
        const int i = a.grid.x0 + bx * a.grid.step_x, j = a.grid.y0 + by * a.grid.step_y;
        const int wx0 = i + m.px - 4, wy0 = j + m.py - 4;
        // the search window (plus the half-pixel ring) must lie inside the frame
        if (wx0 - ring < 0 || wy0 - ring < 0 || wx0 + 16 + ring > a.w || wy0 + 16 + ring > a.h) continue;
        uint32_t ref[8][2];
#pragma unroll
        for (int r = 0; r < 8; r++) lds_bytes8(fp, (j + r) * W + i, ref[r]);
        if (gradient_gate(ref) < (uint32_t)a.feature_threshold) continue;
        u64 lo = 0, hi = 0;
        uint32_t k8 = (uint32_t)(d * 9 + 8);
#pragma unroll
        for (int r = 0; r < 8; r++) {
            uint4 w = lds_bytes16(fc, (wy0 + d + r) * W + wx0);
            if (m.delta != 0) w = sat_add_u8x16(w, m.delta);
            const u64 p01 = pack64(w.x, w.y), p12 = pack64(w.y, w.z), p23 = pack64(w.z, w.w);
            lo = qsad(p01, ref[r][0], lo);
            lo = qsad(p12, ref[r][1], lo);
            hi = qsad(p12, ref[r][0], hi);
            hi = qsad(p23, ref[r][1], hi);
            k8 = __builtin_amdgcn_sad_hi_u8(w.z, ref[r][0], k8);
            k8 = __builtin_amdgcn_sad_hi_u8(w.w, ref[r][1], k8);
        }
        const uint32_t base = (uint32_t)(d * 9);
        const uint32_t l0 = (uint32_t)lo, l1 = (uint32_t)(lo >> 32), h0 = (uint32_t)hi, h1 = (uint32_t)(hi >> 32);
        uint32_t best = min(min((l0 << 16) | (base + 0), (l0 & 0xFFFF0000u) | (base + 1)),
                            min((l1 << 16) | (base + 2), (l1 & 0xFFFF0000u) | (base + 3)));
        best = min(best, min(min((h0 << 16) | (base + 4), (h0 & 0xFFFF0000u) | (base + 5)),
                             min((h1 << 16) | (base + 6), (h1 & 0xFFFF0000u) | (base + 7))));
        best = min(best, k8);
        atomicMin(&keys[blk], best);
    }
    __syncthreads();

    // ---- D1 (half-pixel refinement): four lanes per accepted block, two tile rows each with their window
    // rows -1 .. 2 relative to the best match (aof_refine.hpp); the eight direction sums of the four slices
    // add up across the quad (integer sums: any order) and the direction rides back in bits 8..11 of the
    // block's key (idx < 81 needs seven).  A quarter of the dependent row steps of one lane per block: this
    // is the latency path.  Whole waves: shuffles.
    if constexpr (SUBPIXEL) {
        constexpr int kParts = 4, kRows = 8 / kParts;
        for (int q = tid; q < (kParts * nb + 63) / 64 * 64; q += kThreads) {
            const int blk = q / kParts, part = q % kParts;
            const uint32_t key = blk < nb ? keys[blk] : 0xFFFFFFFFu;
            const bool refine = key != 0xFFFFFFFFu && (key >> 16) < (uint32_t)a.value_threshold;
            RefineState<2, kRows> st;
            st.init();
            if (refine && (key >> 16) != 0) {   // (nothing is below a SAD of zero: such a match keeps "none" from the empty sums)
                const int idx = (int)(key & 0xFFFFu);
                const int by = blk / nx, bx = blk - by * nx;
                const int i = a.grid.x0 + bx * a.grid.step_x, j = a.grid.y0 + by * a.grid.step_y + kRows * part;
                const int rx = i + m.px - 4 + idx % 9 - 1, ry = j + m.py - 4 + idx / 9 - 1;
                uint32_t ref[kRows][2];
#pragma unroll
                for (int r = 0; r < kRows; r++) lds_bytes8(fp, (j + r) * W + i, ref[r]);
                for_rows<-1, kRows>([&](auto yc) {
                    constexpr int Y = decltype(yc)::value;
                    uint32_t dd[3];
                    lds_bytes12(fc, (ry + Y + 1) * W + rx, dd);
                    if (m.delta != 0) {
#pragma unroll
                        for (int k = 0; k < 3; k++) dd[k] = sat_add_u8x4(dd[k], m.delta);
                    }
                    st.template row<Y>(dd, ref);
                });
            }
#pragma unroll
            for (int o = 1; o < kParts; o <<= 1) {
#pragma unroll
                for (int k = 0; k < 8; k++) st.acc[k] += (uint32_t)__shfl_xor((int)st.acc[k], o, 64);
            }
            // (the quad's four lanes read the key above, in the same wave, before this write)
            if (refine && part == 0) keys[blk] = key | ((uint32_t)st.direction(key >> 16) << 8);
        }
        __syncthreads();
    }

    // ---- D: one lane per block ----
    const bool live = tid < nb;   // nb <= kThreads
    aof_block rec;
    rec.dx = 0; rec.dy = 0; rec.sad = AOF_SAD_SKIPPED;
    int subdir = 8;
    if (live) {
        const uint32_t key = keys[tid];
        const size_t item = (size_t)pair * (size_t)nb + (size_t)tid;
        if (key != 0xFFFFFFFFu) {
            const int idx = (int)(key & 0xFFu);
            rec.dx = (int8_t)(m.px + idx % 9 - 4);
            rec.dy = (int8_t)(m.py + idx / 9 - 4);
            rec.sad = (uint16_t)(key >> 16);
            if constexpr (SUBPIXEL) {
                if ((uint32_t)rec.sad < (uint32_t)a.value_threshold) subdir = (int)((key >> 8) & 0xFu);
            }
        }
        reinterpret_cast<uint32_t *>(a.blocks)[item] = __builtin_bit_cast(uint32_t, rec);
        if (SUBPIXEL) a.subdirs[item] = (uint8_t)subdir;
    }
    const bool ok = live && (uint32_t)rec.sad < (uint32_t)a.value_threshold;  // skipped = 0xFFFF
    const int hx = (subdir == 0 || subdir == 1 || subdir == 7) ? 1 : ((subdir == 3 || subdir == 4 || subdir == 5) ? -1 : 0);
    const int hy = (subdir == 1 || subdir == 2 || subdir == 3) ? 1 : ((subdir == 5 || subdir == 6 || subdir == 7) ? -1 : 0);
    const int vx = 2 * rec.dx + hx, vy = 2 * rec.dy + hy;
    wave_vote2(votes[0], votes[1], vx + centre, vy + centre, ok);
    const int s2x = (int)wave_sum_u32((uint32_t)(ok ? vx : 0)), s2y = (int)wave_sum_u32((uint32_t)(ok ? vy : 0));
    const int cnt = (int)wave_sum_u32(ok ? 1u : 0u);
    if ((tid & 63) == 0 && cnt) {
        atomicAdd(&tot[0], s2x);
        atomicAdd(&tot[1], s2y);
        atomicAdd(&tot[2], cnt);
    }
    __syncthreads();
    if (tid < 64) finalise_flow_wave(tail, pair, votes[0], votes[1], tot, record_out, pred_rec);   // bins <= 64 (launcher)
}

// One pair: passes A..D.  The workgroup keeps two frame buffers in LDS (each with its level-1 image and
// its pixel sums); `src[b]` is the frame that belongs in buffer b (device or pinned host memory),
// `cur_buf` says which buffer holds the newer frame of the pair, and bit b of `load` says whether buffer
// b has to be fetched (and its level-1 image and sums made) -- the resident kernel keeps the frame of its
// previous call in LDS and fetches only the new one.
// PITCHED (the stream bank's camera forms): bit b of `pitched` says that src[b] is a window of a larger image -- its
// rows lie crop.pitch bytes apart and may start on any byte; every other source is a contiguous, 16-byte aligned frame.
// The camera tick fetches its new frame into buffer 1 (the default); a burst alternates the buffers.  `crop` (aof_crop.hpp)
// is the windows' source; its pixel format and binning are looked at by the PACKED instantiations only (the kernels with
// a sensor argument), every other one fetches grey, unbinned rows.
// `search` false: only the fetch (passes A and B) -- the buffers named by `load` then hold their frame, its level-1
// image and its sums for a later call that names them as the older frame (a stream's first frame inside a burst).
// FILLED (the tick with the warp inside it, k_bank_tick_warp.hip): bit b of `filled` (uniform) says that the caller has
// written buffer b's level-0 frame into LDS itself, in front of this call -- pass A does not fetch it, and bit b of `load`
// then means only "make its sums and its level-1 image"; `filled_sum` is the lane's share of the byte sum of what it wrote
// (one filled buffer at most).  The first barrier below stands between the caller's stores and every read of them.
// Without FILLED the two arguments are not looked at and the function is the one it was, instruction for instruction.
template <bool SUBPIXEL, bool PITCHED = false, bool PACKED = false, bool FILLED = false>
__device__ __forceinline__ void flow_small_pair(const SmallArgs &a, uint32_t pair, const uint8_t *src0, const uint8_t *src1,
                                                int cur_buf, uint32_t load, aof_flow *final_copy = nullptr,
                                                const CropSource &crop = crop_grey(0), uint32_t pitched = 2u, bool search = true,
                                                uint32_t filled = 0u, uint32_t filled_sum = 0u)
{
    const int pitch = crop.pitch, gb = crop.gb, shift = crop.shift, bin = crop.bin;
    extern __shared__ __attribute__((aligned(16))) uint8_t s_mem[];
    __shared__ uint32_t s_keys[kThreads];
    __shared__ uint32_t s_votes[2][kMaxBins];
    __shared__ int s_tot[3];
    __shared__ aof_flow s_flow1;     // the level-1 flow record: predictor of level 0
    __shared__ uint32_t s_sums[4];   // [buffer][level]
    const int tid = threadIdx.x;
    const int w = a.l0.w, h = a.l0.h, w1 = w / 2, h1 = h / 2;
    const int frame0 = w * h, frame1 = w1 * h1;
    const bool two = a.levels == 2;
    uint8_t *f0[2] = {s_mem, s_mem + frame0 + kPad};
    uint8_t *f1[2] = {s_mem + 2 * (frame0 + kPad), s_mem + 2 * (frame0 + kPad) + ((frame1 + kPad + 15) & ~15)};
    const int first = (load & 1u) ? 0 : 1, count = (load == 3u) ? 2 : (load ? 1 : 0);   // buffers to fetch: first, first + 1, ...

    if (tid < 4 && ((load >> (tid >> 1)) & 1u)) s_sums[tid] = 0;
    __syncthreads();

    // ---- A: level-0 frames -> LDS (a frame is contiguous: row stride == w) ----
    {
        const int per_frame = frame0 / 16;
        uint32_t sum[2] = {0, 0};
        uint32_t fetch = load;   // the buffers pass A fetches: all that are loaded, but for those the caller has filled
        if constexpr (FILLED) {
            fetch = load & ~filled;
            sum[0] = (filled & 1u) ? filled_sum : 0u;
            sum[1] = (filled & 2u) ? filled_sum : 0u;
        }
        uint32_t rest = fetch;   // the buffers the loop of 16-byte pieces below fetches: all, but for windows of packed pixels
        if constexpr (PITCHED && PACKED) {
            // crop_fetch's three answers (aof_crop.hpp), spelled out: asked through the function, or through crop_piece in
            // the loop below, the four sensor kernels of the tick and the burst come out as other code (LAB_LOG.md)
            if (bin != 1 || gb > 2) {   // (uniform) binned windows come first as well: one piece per lane and trip -- a piece
                              // is bin rows of up to eight loads, and its eight sums are all it keeps.  MIPI-packed windows
                              // (gb 5, 3) go the same way, binned or not: a loop of their own, pieces one behind the other

                const int row_chunks = w / 16;
#pragma unroll
                for (int buf = 0; buf < 2; buf++) {
                    if (!(((fetch & pitched) >> buf) & 1u)) continue;
                    const uint8_t *src = buf ? src1 : src0;
#pragma unroll 1
                    for (int c = tid; c < per_frame; c += kThreads) {
                        const int y = c / row_chunks, x = c - y * row_chunks;
                        uint4 v;
                        if (bin != 1) crop_piece16_binned(v, src, y, pitch, x, gb, shift, bin);
                        else crop_piece16(v, src, y, pitch, x, gb, shift);
                        uint32_t s = 0;
                        s = byte_sum(v.x, s); s = byte_sum(v.y, s);
                        s = byte_sum(v.z, s); s = byte_sum(v.w, s);
                        sum[buf] += s;
                        *reinterpret_cast<uint4 *>(f0[buf] + c * 16) = v;
                    }
                }
                rest = fetch & ~pitched;
            } else if (gb != 1) {   // (uniform) two source bytes per pixel: the windows come first, in trips of half as many
                              // pieces -- as many 16-byte loads in flight as below, not twice the registers
                constexpr int kHalf = kLoads / 2;
                const int row_chunks = w / 16;
#pragma unroll
                for (int buf = 0; buf < 2; buf++) {
                    if (!(((fetch & pitched) >> buf) & 1u)) continue;
                    const uint8_t *src = buf ? src1 : src0;
                    for (int base = 0; base < per_frame; base += kHalf * kThreads) {
                        uint4 v[kHalf];
#pragma unroll
                        for (int k = 0; k < kHalf; k++) {
                            const int c = base + k * kThreads + tid;
                            v[k] = make_uint4(0, 0, 0, 0);
                            if (c < per_frame) {
                                const int y = c / row_chunks, x = c - y * row_chunks;
                                crop_piece16(v[k], src, y, pitch, x, 2, shift);
                            }
                        }
#pragma unroll
                        for (int k = 0; k < kHalf; k++) {
                            const int c = base + k * kThreads + tid;
                            if (c >= per_frame) continue;
                            uint32_t s = 0;
                            s = byte_sum(v[k].x, s); s = byte_sum(v[k].y, s);
                            s = byte_sum(v[k].z, s); s = byte_sum(v[k].w, s);
                            sum[buf] += s;
                            *reinterpret_cast<uint4 *>(f0[buf] + c * 16) = v[k];
                        }
                    }
                }
                rest = fetch & ~pitched;
            }
        }
        const int first_a = (rest & 1u) ? 0 : 1, count_a = (rest == 3u) ? 2 : (rest ? 1 : 0);   // (first, count of `rest`)
        const int items = count_a * per_frame;
        for (int base = 0; base < items; base += kLoads * kThreads) {
            uint4 v[kLoads];
#pragma unroll
            for (int k = 0; k < kLoads; k++) {
                const int it = base + k * kThreads + tid;
                v[k] = make_uint4(0, 0, 0, 0);
                if (it < items) {
                    const int buf = first_a + (it >= per_frame), c = it - (it >= per_frame) * per_frame;
                    if (PITCHED && ((pitched >> buf) & 1u)) {   // one 16-byte load wherever the window starts (as k_ingest fetches its crop)
                        if constexpr (PITCHED) {
                            const int y = c / (w / 16), x = c - y * (w / 16);
                            crop_piece16(v[k], buf ? src1 : src0, y, pitch, x, 1, 0);
                        }
                    } else {
                        v[k] = *reinterpret_cast<const uint4 *>((buf ? src1 : src0) + c * 16);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kLoads; k++) {
                const int it = base + k * kThreads + tid;
                if (it >= items) continue;
                const int buf = first_a + (it >= per_frame), c = it - (it >= per_frame) * per_frame;
                uint32_t s = 0;
                s = byte_sum(v[k].x, s); s = byte_sum(v[k].y, s);
                s = byte_sum(v[k].z, s); s = byte_sum(v[k].w, s);
                sum[buf] += s;
                *reinterpret_cast<uint4 *>(f0[buf] + c * 16) = v[k];
            }
        }
        if (a.sums) {
#pragma unroll
            for (int buf = 0; buf < 2; buf++) {
                const uint32_t t = wave_sum_u32(sum[buf]);
                if ((tid & 63) == 0 && ((load >> buf) & 1u)) atomicAdd(&s_sums[buf * 2], t);
            }
        }
    }
    __syncthreads();

    // ---- B: level-1 frames, LDS -> LDS ----
    if (two) {
        const int chunks = w / 16, per_frame = h1 * chunks;
        uint32_t sum[2] = {0, 0};
        for (int it = tid; it < count * per_frame; it += kThreads) {
            const int buf = first + (it >= per_frame), rest = it - (it >= per_frame) * per_frame;
            const int y1 = rest / chunks, c = rest - y1 * chunks;
            const uint4 r0 = *reinterpret_cast<const uint4 *>(f0[buf] + (2 * y1) * w + c * 16);
            const uint4 r1 = *reinterpret_cast<const uint4 *>(f0[buf] + (2 * y1 + 1) * w + c * 16);
            const uint32_t p0 = box2(r0.x, r1.x), p1 = box2(r0.y, r1.y);
            const uint32_t p2 = box2(r0.z, r1.z), p3 = box2(r0.w, r1.w);
            uint2 o;
            o.x = __builtin_amdgcn_perm(p1, p0, 0x06040200u);
            o.y = __builtin_amdgcn_perm(p3, p2, 0x06040200u);
            sum[buf] = byte_sum(o.x, sum[buf]);
            sum[buf] = byte_sum(o.y, sum[buf]);
            *reinterpret_cast<uint2 *>(f1[buf] + y1 * w1 + c * 8) = o;
        }
        if (a.sums) {
#pragma unroll
            for (int buf = 0; buf < 2; buf++) {
                const uint32_t t = wave_sum_u32(sum[buf]);
                if ((tid & 63) == 0 && ((load >> buf) & 1u)) atomicAdd(&s_sums[buf * 2 + 1], t);
            }
        }
        __syncthreads();
    }
    if (!search) return;

    const int pb = 1 - cur_buf;   // the buffer of the older frame
    LevelMeta m0 = {0, 0, 0}, m1 = {0, 0, 0};
    if (a.sums) {
        const uint32_t n0 = (uint32_t)frame0;
        m0.delta = (int)((s_sums[pb * 2] + n0 / 2) / n0) - (int)((s_sums[cur_buf * 2] + n0 / 2) / n0);
        if (two) {
            const uint32_t n1 = (uint32_t)frame1;
            m1.delta = (int)((s_sums[pb * 2 + 1] + n1 / 2) / n1) - (int)((s_sums[cur_buf * 2 + 1] + n1 / 2) / n1);
        }
        // workspace layout: [frame: 0 prev, 1 cur][level]
        if (tid < 4) a.sums[(size_t)pair * 4 + tid] = s_sums[((tid >> 1) ? cur_buf : pb) * 2 + (tid & 1)];
    }

    if (two) {
        run_level<SUBPIXEL>(a.l1, a.t1, pair, f1[pb], f1[cur_buf], m1, s_keys, s_votes, s_tot, &s_flow1, nullptr);
        __syncthreads();
        m0.px = s_flow1.pred_x;
        m0.py = s_flow1.pred_y;
    }
    // (final_copy: an LDS copy of the pair's flow record for the caller; visible after its next barrier)
    run_level<SUBPIXEL>(a.l0, a.t0, pair, f0[pb], f0[cur_buf], m0, s_keys, s_votes, s_tot, final_copy, two ? &s_flow1 : nullptr);
}

// Dynamic LDS of a workgroup that runs flow_small_pair: both level-0 frames and, with two levels, their level-1 images
// (small_plan_make, aof_small_plan.hpp).
inline size_t small_lds_bytes(const SmallArgs &a) { return small_plan_make(a).lds; }

// The ONE launcher of the one-workgroup class (k_flow_small.hip, k_bank.hip, k_bank_burst.hip): `grid` workgroups of
// kThreads lanes run `fn` on the plan `sm`; `args` are the kernel's own arguments.  `fn` is the instantiation that is
// launched: the dynamic-LDS limit above 48 KiB is an attribute of that one function.
template <typename... Params, typename... Args>
inline int launch_small_class(void (*fn)(Params...), uint32_t grid, const SmallArgs &sm, void *stream, const Args &...args)
{
    const SmallPlan plan = small_plan_make(sm);
    if (plan.verdict != SMALL_OK) return (int)hipErrorInvalidValue;
    const size_t lds = plan.lds;
    if (plan.attr) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fn),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kSmallLdsLimit - kSmallStaticLds));
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(fn, dim3(grid), dim3(kThreads), lds, static_cast<hipStream_t>(stream), args...);
    return (int)hipGetLastError();
}

}  // namespace

}  // namespace aof
