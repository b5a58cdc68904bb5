// The exposure statistics of a frame and one step of the auto-exposure controller (include/aof.h, "auto-exposure
// control per stream"; mainloop.cpp:203-271), the ONE place their arithmetic is written.  The bin
// and the mean sample value: k_ingest.hip and the bank's tail (aof_bank_stream.hpp) on the device, aof_exposure_bin and
// aof_exposure_msv on the host.  The step: k_bank_exposure.hip runs it per lane, aof_exposure_control_host per element.
// IEEE float32 throughout, every operation rounded on its own: nothing is contracted into a multiply-add, on either
// side.  The pragma that says so is clang's; a host file built by another compiler, or without the flag (aof_params.cpp),
// computes the same: these builds target baseline x86-64, which has no fused multiply-add to contract into.
#pragma once

#include "aof_hd.hpp"

namespace aof {

// The histogram bin of a grey value 0..255: == cvFloor(grey * (10 / 255.0)) for every 8-bit value.  10 for 255, which
// lies outside cv::calcHist's half-open range and is counted nowhere.
AOF_HD_INLINE int exposure_bin(uint32_t v) { return (int)((v * 10u) / 255u); }

// mainloop.cpp:216-220, the same float operations in the same order.
AOF_HD_INLINE float exposure_msv(const uint32_t *hist)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float msv = 0.0f;
    for (int i = 0; i < AOF_EXPOSURE_BINS; i++) msv += (i + 1) * (float)hist[i] / 16384.0f;
    return msv;
}

// `st` is what the camera runs with and the controller's memory; `msv` the mean sample value of a frame that passed the
// exposure gate.  Returns the command record of the step.  The reference's quirks stay: no anti-windup, the gain
// branch never touches the exposure, the controller restarts from the integers the camera holds, and a NaN sets
// nothing (every comparison with it is false, so it never reaches a conversion).
AOF_HD_INLINE aof_exposure_command exposure_step(const aof_exposure_control &ec, aof_exposure_state &st, float msv)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float err = ec.msv_target - msv;
    const float d = err - st.msv_error_old;
    const float integral = st.msv_error_int + err;
    const float ce = (float)st.exposure, cg = (float)st.gain;
    float e = ce + ((ec.exposure_p * err + ec.exposure_i * integral) + ec.exposure_d * d);
    uint32_t flags = AOF_EXPOSURE_UPDATED;
    if (cg > 1.0f || (e > ec.exposure_max - 1.0f && ce > ec.exposure_max - 1.0f)) {
        // the exposure is saturated (or the gain already in use): the gain follows the MSV
        float g = cg + ((ec.gain_p * err + ec.gain_i * integral) + ec.gain_d * d);
        if (g > ec.gain_max) g = ec.gain_max;
        else if (g < 1.0f) g = 1.0f;
        const float step = g - cg;
        if ((step < 0.0f ? -step : step) > ec.gain_change_threshold || (g < 2.0f && cg > 1.0f) ||
            (g > ec.gain_max - 1.0f && cg < ec.gain_max)) {
            st.gain = (uint8_t)g;
            flags |= AOF_EXPOSURE_SET_GAIN;
        }
    } else {
        if (e > ec.exposure_max) e = ec.exposure_max;
        else if (e < 1.0f) e = 1.0f;
        const float step = e - ce;
        if ((step < 0.0f ? -step : step) > ec.exposure_change_threshold || (e < 2.0f && ce > 1.0f) ||
            (e > ec.exposure_max - 1.0f && ce < ec.exposure_max)) {
            st.exposure = (uint16_t)e;
            flags |= AOF_EXPOSURE_SET_EXPOSURE;
        }
    }
    st.msv_error_old = err;
    st.msv_error_int = integral;
    st.updates += 1u;
    aof_exposure_command c;
    c.exposure = st.exposure;
    c.gain = st.gain;
    c.flags = (uint8_t)flags;
    c.msv_error = err;
    c.msv_error_int = integral;
    c.update = st.updates;
    return c;
}

}  // namespace aof
