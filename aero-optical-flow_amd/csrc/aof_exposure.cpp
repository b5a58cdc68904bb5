// The stream bank's auto-exposure control (include/aof.h, "the stream bank's auto-exposure control"), host side: the
// reference's constants, the argument checks and the launches of k_bank_exposure.hip behind a camera push, and the same
// function as a plain loop on host memory.  The device calls know nothing about the bank: they read the push's exposure
// records and a state array of the caller's.  Nothing here synchronises or allocates.  This file is compiled with
// floating-point contraction off: aof_exposure_control_host rounds every operation on its own, as the kernel does.
#include <cerrno>
#include <cmath>
#include <cstring>

#include "aof_bank_calls.hpp"
#include "aof_ctx.hpp"
#include "aof_exposure_step.hpp"
#include "aof_host.hpp"

using namespace aof;

namespace {

// nullptr, or what is wrong with the constants
const char *bad_control(const aof_exposure_control &ec)
{
    const float all[] = {ec.msv_target, ec.exposure_p, ec.exposure_i, ec.exposure_d, ec.gain_p, ec.gain_i, ec.gain_d,
                         ec.exposure_change_threshold, ec.exposure_max, ec.gain_change_threshold, ec.gain_max};
    for (const float v : all)
        if (!std::isfinite(v)) return "exposure control: a constant is not finite";
    if (!(ec.exposure_max >= 1.0f && ec.exposure_max <= 65535.0f)) return "exposure control: exposure_max outside 1..65535";
    if (!(ec.gain_max >= 1.0f && ec.gain_max <= 255.0f)) return "exposure control: gain_max outside 1..255";
    return nullptr;
}

}  // namespace

extern "C" {

int aof_exposure_control_default(aof_exposure_control *ec)
{
    if (!ec) return -EINVAL;
    // /root/reference/src/mainloop.cpp:53-63
    ec->msv_target = 5.0f;
    ec->exposure_p = 100.0f;
    ec->exposure_i = 0.5f;
    ec->exposure_d = 0.5f;
    ec->gain_p = 50.0f;
    ec->gain_i = 0.5f;
    ec->gain_d = 0.5f;
    ec->exposure_change_threshold = 30.0f;
    ec->exposure_max = 1727.0f;
    ec->gain_change_threshold = 15.0f;
    ec->gain_max = 127.0f;
    return 0;
}

int aof_bank_exposure_reset_device(aof_ctx *ctx, int32_t n_streams, const uint8_t *d_mask, uint16_t exposure0, uint8_t gain0,
                                   const uint16_t *d_exposure0, const uint8_t *d_gain0, aof_exposure_state *d_state,
                                   void *stream)
{
    if (!ctx) return -EINVAL;
    if (!d_state) return ctx_fail(ctx, -EINVAL, "exposure reset: null state pointer");
    if (n_streams < 1) return ctx_fail(ctx, -EINVAL, "exposure reset: n_streams < 1");
    if (!aligned(d_state, 4) || !aligned(d_exposure0, 2))
        return ctx_fail(ctx, -EINVAL, "exposure reset: the state must be 4-byte aligned, the exposure values 2-byte aligned");
    if (const int rc = precheck(ctx)) return rc;
    if (launch_bank_exposure_reset(d_state, d_mask, (uint32_t)n_streams, exposure0, gain0, d_exposure0, d_gain0, stream))
        return ctx_fail(ctx, -EIO, "exposure reset launch failed");
    return 0;
}

int aof_bank_exposure_control_device(aof_ctx *ctx, const aof_exposure_control *ec, int32_t n_streams, int32_t n_rounds,
                                     const aof_exposure_record *d_exposure, aof_exposure_state *d_state,
                                     aof_exposure_command *d_commands, void *stream)
{
    if (!ctx) return -EINVAL;
    if (!ec || !d_exposure || !d_state || !d_commands)
        return ctx_fail(ctx, -EINVAL, "exposure control: null constants, record, state or command pointer");
    if (n_streams < 1) return ctx_fail(ctx, -EINVAL, "exposure control: n_streams < 1");
    if (n_rounds < 1 || n_rounds > AOF_BANK_BURST_MAX)
        return ctx_fail(ctx, -EINVAL, "exposure control: n_rounds outside 1..AOF_BANK_BURST_MAX");
    if (!aligned(d_exposure, 4) || !aligned(d_state, 4) || !aligned(d_commands, 4))
        return ctx_fail(ctx, -EINVAL, "exposure control: records, state and commands must be 4-byte aligned");
    if (const char *what = bad_control(*ec)) return ctx_fail(ctx, -EINVAL, what);
    if (const int rc = precheck(ctx)) return rc;

    ExposureArgs a;
    std::memset(&a, 0, sizeof(a));
    a.ec = *ec;
    a.n_streams = (uint32_t)n_streams;
    a.n_rounds = (uint32_t)n_rounds;
    a.records = reinterpret_cast<const uint8_t *>(d_exposure);
    a.state = d_state;
    a.commands = d_commands;
    if (launch_bank_exposure(a, stream)) return ctx_fail(ctx, -EIO, "exposure control launch failed");
    return 0;
}

int aof_exposure_control_host(const aof_exposure_control *ec, int32_t n_streams, int32_t n_rounds,
                              const aof_exposure_record *records, aof_exposure_state *states, aof_exposure_command *commands)
{
    if (!ec || !records || !states || !commands) return -EINVAL;
    if (n_streams < 1 || n_rounds < 1 || n_rounds > AOF_BANK_BURST_MAX) return -EINVAL;
    if (bad_control(*ec)) return -EINVAL;
    for (int32_t k = 0; k < n_rounds; k++) {
        for (int32_t s = 0; s < n_streams; s++) {
            const size_t o = (size_t)k * (size_t)n_streams + (size_t)s;
            aof_exposure_command c;
            std::memset(&c, 0, sizeof(c));
            if (records[o].due) c = exposure_step(*ec, states[s], records[o].msv);
            commands[o] = c;
        }
    }
    return 0;
}

}  // extern "C"
