// The auto-exposure controller of a stream bank (aof_bank_exposure_control_device / aof_bank_exposure_reset_device,
// include/aof.h "the stream bank's auto-exposure control"): the PID step of mainloop.cpp:222-271 for S streams behind a
// camera push, ONE launch, a lane per stream:
//   * a lane loads the (msv, due) words of its K exposure records first -- they do not depend on the state, so all K
//     loads are in flight before the first step and the rounds do not serialise on memory -- and its 16-byte state once;
//   * it walks the rounds in order (exposure_step, aof_exposure_step.hpp: the arithmetic the host function runs) and
//     stores one 16-byte command per round, lane-consecutive within a round, all zero for a record that was not due;
//   * it stores the state once, and the kernel ends with a system-scope release behind its stores: commands kept in
//     pinned host memory are there for a host that sees the tag of a collect call enqueued behind this launch.
// No LDS, no cross-lane traffic, no waiting.  The entry point's alignment rule is 4 bytes: the (msv, due) pair is one
// 8-byte access declared 4-byte aligned, states and commands are written in 4-byte words which the compiler joins into
// one access each; gfx950 takes wider accesses at any 4-byte address.
#include <hip/hip_runtime.h>

#include "aof_bank_calls.hpp"
#include "aof_exposure_step.hpp"

namespace aof {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kRecordBytes = sizeof(aof_exposure_record);
static_assert(kRecordBytes == 48 && offsetof(aof_exposure_record, msv) == 40 && offsetof(aof_exposure_record, due) == 44,
              "msv and due are the record's last two words");
static_assert(sizeof(aof_exposure_state) == 16 && sizeof(aof_exposure_command) == 16, "one 16-byte access each");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef u32x2 u32x2_a4 __attribute__((aligned(4)));     // one 8-byte access at a 4-byte aligned address

__device__ __forceinline__ u32x4 load16(const void *p)
{
    const uint32_t *w = reinterpret_cast<const uint32_t *>(p);
    return u32x4{w[0], w[1], w[2], w[3]};
}
__device__ __forceinline__ void store16(void *p, u32x4 v)
{
    uint32_t *w = reinterpret_cast<uint32_t *>(p);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
}

__global__ __launch_bounds__(kThreads) void k_bank_exposure(ExposureArgs a)
{
    const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
    if (s < a.n_streams) {
        // the K (msv, due) pairs of this stream: every load issued before the first step.  The loads carry no branch: a
        // round behind the last one reads the last one's words again (the same cache line) and is never stepped.
        u32x2 in[AOF_BANK_BURST_MAX];
        const uint32_t last = a.n_rounds - 1u;
#pragma unroll
        for (uint32_t k = 0; k < AOF_BANK_BURST_MAX; k++) {
            // (one load of the pair: two loads of a word each let the compiler move the msv's behind the test of `due`)
            in[k] = *reinterpret_cast<const u32x2_a4 *>(a.records + ((size_t)min(k, last) * a.n_streams + s) * kRecordBytes + 40u);
        }
        aof_exposure_state st;
        const u32x4 raw = load16(a.state + s);
        __builtin_memcpy(&st, &raw, sizeof(st));
#pragma unroll
        for (uint32_t k = 0; k < AOF_BANK_BURST_MAX; k++) {
            if (k <= last) {
                u32x4 out = {0u, 0u, 0u, 0u};
                if (in[k].y != 0u) {
                    const aof_exposure_command c = exposure_step(a.ec, st, __uint_as_float(in[k].x));
                    __builtin_memcpy(&out, &c, sizeof(c));
                }
                store16(a.commands + ((size_t)k * a.n_streams + s), out);
            }
        }
        u32x4 back;
        __builtin_memcpy(&back, &st, sizeof(st));
        store16(a.state + s, back);
    }
    // the commands out to where a host reads them, before the launch counts as done
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

__global__ __launch_bounds__(kThreads) void k_bank_exposure_reset(aof_exposure_state *state, const uint8_t *mask, uint32_t n,
                                                                  uint32_t exposure0, uint32_t gain0, const uint16_t *exposures,
                                                                  const uint8_t *gains)
{
    const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
    if (s >= n || (mask && !mask[s])) return;
    const uint32_t e = exposures ? exposures[s] : exposure0, g = gains ? gains[s] : gain0;
    uint32_t *w = reinterpret_cast<uint32_t *>(state + s);
    w[0] = 0u;              // msv_error_old = 0.0f
    w[1] = 0u;              // msv_error_int = 0.0f
    w[2] = e | g << 16;     // exposure, gain, reserved = 0
    w[3] = 0u;              // updates
}

}  // namespace

int launch_bank_exposure(const ExposureArgs &a, void *stream)
{
    if (a.n_streams < 1 || a.n_rounds < 1 || a.n_rounds > AOF_BANK_BURST_MAX || !a.records || !a.state || !a.commands)
        return (int)hipErrorInvalidValue;
    const uint32_t groups = (a.n_streams + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k_bank_exposure, dim3(groups), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

int launch_bank_exposure_reset(aof_exposure_state *state, const uint8_t *mask, uint32_t n_streams, uint16_t exposure0,
                               uint8_t gain0, const uint16_t *d_exposure0, const uint8_t *d_gain0, void *stream)
{
    if (!state || n_streams < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bank_exposure_reset, dim3((n_streams + kThreads - 1) / kThreads), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), state, mask, n_streams, (uint32_t)exposure0, (uint32_t)gain0,
                       d_exposure0, d_gain0);
    return (int)hipGetLastError();
}

}  // namespace aof
