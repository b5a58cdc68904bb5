// The sequence pipeline's motion field (aof_sequence_field_device, include/aof_sequence_field.h), the window pass: behind
// the per-pair fit (k_field.hip, launched by aof_sequence_field.cpp over the workspace's block records) the fits of ONE
// recorded stream of n frames are integrated over the rate limiter's windows.  The stream bank walks a stream serially, a
// tick per launch; a recording's publications are all known, so the serial run is restated in parallel (DESIGN.md section
// 2, "Sequence motion field"; exact, not approximate).  With F(m) = the frame of record m and F(-1) = 0:
//   * window m is the pairs F(m-1) <= k < F(m) (pair k = frames k, k + 1), read straight from the records: no scan;
//   * its sums are the valid fits of those pairs added in pair order from 0.0: one lane walks one window, every pair
//     through bank_field_step (aof_bank_field_step.hpp) on a held tick, then the step on the record's tick publishes;
//   * the lane behind the last record walks the tail window F(M-1) <= k < n - 1 and stores the state, published = M.
// The arithmetic is that header's; nothing of it is written here.
//   k_seq_field_windows  a lane per record and one for the tail.  A lane reads the second half of every record of its
//                        window -- used, the four floats, the flags; the first half is never looked at -- from global
//                        memory, four pairs in flight.  The fits were written by the launch in front and lie in L2:
//                        staging a workgroup's span in LDS first was measured and is no faster (LAB_LOG.md, "Sequence
//                        motion field").
// No workgroup waits for another, and none has a barrier.  Every index read from device memory is clamped: count[0] to n, a
// frame index into [0, n); a window with F(m) <= F(m-1) is empty, so no walk is longer than n - 1 pairs.
#include "aof_device.hpp"   // (the HIP runtime first: the rule headers' qualifiers are its)
#include "aof_bank_field_step.hpp"
#include "aof_sequence_field_args.hpp"

namespace aof {

namespace {

constexpr int kThreads = (int)kSeqFieldThreads;
constexpr uint32_t kGroup = 4;           // pairs whose loads are in flight together
// The half of an aof_field the step reads, as four 8-byte words (d_fields is 8-byte aligned, no more).
constexpr uint32_t kHalfWords = 4, kRecordWords = sizeof(aof_field) / 8;
static_assert(sizeof(aof_field) == 64 && offsetof(aof_field, fitted) == 32 && offsetof(aof_field, used) == 36 &&
              offsetof(aof_field, zoom) == 40 && offsetof(aof_field, rotation) == 44 && offsetof(aof_field, centre_x) == 48 &&
              offsetof(aof_field, centre_y) == 52 && offsetof(aof_field, flags) == 56,
              "words 4..7 of a field record: (fitted, used), (zoom, rotation), (centre_x, centre_y), (flags, reserved)");
static_assert(sizeof(aof_seq_record) == 32, "a record is eight words");

struct Half {
    uint64_t w[kHalfWords];
};

// What the step looks at of a fit: everything else stays zero.
__device__ __forceinline__ aof_field fit_of(const Half &h)
{
    aof_field f = {};
    f.used = (uint32_t)(h.w[0] >> 32);
    f.zoom = __uint_as_float((uint32_t)h.w[1]); f.rotation = __uint_as_float((uint32_t)(h.w[1] >> 32));
    f.centre_x = __uint_as_float((uint32_t)h.w[2]); f.centre_y = __uint_as_float((uint32_t)(h.w[2] >> 32));
    f.flags = (uint32_t)h.w[3];
    return f;
}

__device__ __forceinline__ Half half_of(const uint64_t *fields, uint32_t k)
{
    const uint64_t *p = fields + (size_t)k * kRecordWords + kHalfWords;
    return Half{{p[0], p[1], p[2], p[3]}};
}

// F of record m (m < M), clamped into the recording
__device__ __forceinline__ uint32_t frame_of(const SeqFieldArgs &a, uint32_t m, uint32_t last) { return min(a.records[m].frame, last); }

__global__ __launch_bounds__(kThreads) void k_seq_field_windows(SeqFieldArgs a)
{
    const uint32_t n = (uint32_t)a.n_frames, last = n - 1u;   // (n < 2^31: the launcher)
    const uint32_t M = min(a.count[0], n);
    const uint32_t m = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (m > M) return;   // (m == M: the tail window, which no record takes)
    const uint64_t *fields = reinterpret_cast<const uint64_t *>(a.fields);
    aof_seq_record rec = {};
    if (m < M) rec = a.records[m];
    const uint32_t frame = min(rec.frame, last);
    const uint32_t lo = m > 0u ? frame_of(a, m - 1u, last) : 0u;
    const uint32_t hi = max(m < M ? frame : last, lo);   // (F(m) <= F(m-1): empty)

    aof_bank_field_state st = {};
    const BankFieldTick held = seq_field_tick(false, 0u, 0);
    for (uint32_t k0 = lo; k0 < hi; k0 += min(kGroup, hi - k0)) {
        // (a slot behind the window's last pair reads the last one again and is not stepped)
        Half h[kGroup];
#pragma unroll
        for (uint32_t g = 0; g < kGroup; g++) h[g] = half_of(fields, k0 + min(g, hi - 1u - k0));
#pragma unroll
        for (uint32_t g = 0; g < kGroup; g++)
            if (g < hi - k0) bank_field_step(held, true, fit_of(h[g]), a.focal_x, a.focal_y, st);
    }
    if (m < M) {
        st.published = m;   // (the messages in front of this one: the step adds its own)
        a.out[m] = bank_field_step(seq_field_tick(true, frame, rec.dt_us), false, aof_field{}, a.focal_x, a.focal_y, st);
    } else if (a.state) {
        st.published = M;
        *a.state = st;
    }
}

}  // namespace

int launch_sequence_field(const SeqFieldArgs &a, void *stream)
{
    if (a.n_frames < 1 || a.n_frames >= 0x7FFFFFF0ll || !a.count || !a.records || !a.out || (!a.fields && a.n_frames > 1))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_seq_field_windows, dim3((uint32_t)seq_field_groups(a.n_frames)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

}  // namespace aof
