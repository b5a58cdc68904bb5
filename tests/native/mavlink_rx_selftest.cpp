// A stand-alone driver of aof_bank_mavlink_rx_host for a sanitizer build (tests/test_bank_mavlink_rx_asan.py): the
// split-invariance case.  One byte stream -- a MAVLink 1 HIGHRES_IMU frame, junk, a signed MAVLink 2 frame, a frame of
// another message whose payload holds a valid HIGHRES_IMU frame, a MAVLink 2 frame -- is taken whole and then in every
// cut into two calls, each call's bytes in a heap block of exactly the slot's size: the samples in order and the final
// 128 state bytes must be the same.  The device entry points of the translation unit are never called; what they would
// call is stubbed at the bottom.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "aof.h"

namespace {

typedef std::vector<uint8_t> Bytes;

uint16_t crc_accumulate(uint8_t byte, uint16_t crc)
{
    uint8_t tmp = (uint8_t)(byte ^ (uint8_t)(crc & 0xFF));
    tmp = (uint8_t)(tmp ^ (uint8_t)(tmp << 4));
    return (uint16_t)((crc >> 8) ^ ((uint16_t)tmp << 8) ^ ((uint16_t)tmp << 3) ^ (tmp >> 4));
}

Bytes imu_payload(uint64_t t, float x, float y, float z)
{
    Bytes p(62, 0);
    std::memcpy(&p[0], &t, 8);
    std::memcpy(&p[20], &x, 4);
    std::memcpy(&p[24], &y, 4);
    std::memcpy(&p[28], &z, 4);
    p[61] = 0x1F;   // fields_updated: keeps the MAVLink 2 form from truncating to 32 bytes
    return p;
}

// v2: with a 13-byte signature where `sign`
Bytes frame(bool v2, uint32_t msgid, const Bytes &payload, uint8_t seq, bool sign)
{
    Bytes f;
    f.push_back(v2 ? 0xFD : 0xFE);
    f.push_back((uint8_t)payload.size());
    if (v2) {
        f.push_back(sign ? 1 : 0);
        f.push_back(0);
    }
    f.push_back(seq);
    f.push_back(1);
    f.push_back(1);
    f.push_back((uint8_t)msgid);
    if (v2) {
        f.push_back((uint8_t)(msgid >> 8));
        f.push_back((uint8_t)(msgid >> 16));
    }
    f.insert(f.end(), payload.begin(), payload.end());
    uint16_t crc = 0xFFFF;
    for (size_t i = 1; i < f.size(); i++) crc = crc_accumulate(f[i], crc);
    crc = crc_accumulate(93, crc);
    f.push_back((uint8_t)(crc & 0xFF));
    f.push_back((uint8_t)(crc >> 8));
    if (sign)
        for (int i = 0; i < 13; i++) f.push_back((uint8_t)(0xA0 + i));
    return f;
}

void append(Bytes &to, const Bytes &b) { to.insert(to.end(), b.begin(), b.end()); }

struct Result {
    std::vector<aof_imu_sample> samples;
    aof_mavlink_rx_state state;
};

const int kSlots = 16;

// one call on `n` bytes held in a heap block of exactly B bytes (B: n rounded up to the slot granularity)
void call(const uint8_t *bytes, size_t n, aof_mavlink_rx_state *state, Result &r)
{
    const size_t B = n < 16 ? 16 : (n + 15) / 16 * 16;
    uint8_t *slot = static_cast<uint8_t *>(std::aligned_alloc(16, B));
    uint16_t *len = static_cast<uint16_t *>(std::malloc(sizeof(uint16_t)));
    aof_imu_sample *samples = static_cast<aof_imu_sample *>(std::malloc(kSlots * sizeof(aof_imu_sample)));
    uint8_t *count = static_cast<uint8_t *>(std::malloc(1));
    if (!slot || !len || !samples || !count) std::abort();
    std::memset(slot, 0xFE, B);          // (behind the length: start bytes that must not be taken)
    if (n) std::memcpy(slot, bytes, n);
    *len = (uint16_t)n;
    aof_mavlink_rx_params rp = {1, 1, (int32_t)B, kSlots};
    const int rc = aof_bank_mavlink_rx_host(&rp, slot, len, state, samples, count);
    if (rc) {
        std::printf("aof_bank_mavlink_rx_host returned %d\n", rc);
        std::exit(1);
    }
    for (int j = 0; j < *count; j++) r.samples.push_back(samples[j]);
    std::free(count);
    std::free(samples);
    std::free(len);
    std::free(slot);
}

Result run(const Bytes &stream, size_t cut)
{
    Result r;
    aof_mavlink_rx_state *state = static_cast<aof_mavlink_rx_state *>(std::calloc(1, sizeof(aof_mavlink_rx_state)));
    if (!state) std::abort();
    call(stream.data(), cut, state, r);
    call(stream.data() + cut, stream.size() - cut, state, r);
    r.state = *state;
    std::free(state);
    return r;
}

}  // namespace

int main()
{
    Bytes stream;
    append(stream, frame(false, 105, imu_payload(1000, 0.1f, 0.2f, 0.3f), 1, false));
    const uint8_t junk[11] = {0, 1, 2, 0xFC, 0xFF, 9, 0x55, 0xAA, 3, 4, 5};
    stream.insert(stream.end(), junk, junk + 11);
    append(stream, frame(true, 105, imu_payload(2000, -0.1f, -0.2f, -0.3f), 2, true));
    Bytes inner = frame(false, 105, imu_payload(9, 9.0f, 9.0f, 9.0f), 0, false);
    inner.push_back(7);
    append(stream, frame(true, 33, inner, 3, false));
    append(stream, frame(true, 105, imu_payload(3000, 1.0f, 2.0f, 3.0f), 4, false));

    const Result whole = run(stream, stream.size());
    const aof_mavlink_rx_state &st = whole.state;
    bool ok = whole.samples.size() == 3 && whole.samples[0].time_usec == 1000 && whole.samples[1].time_usec == 2000 &&
              whole.samples[2].time_usec == 3000 && whole.samples[2].zgyro == 3.0f && whole.samples[1].xgyro == -0.1f &&
              st.bytes == stream.size() && st.frames == 4 && st.imu_samples == 3 && st.skipped == 11 && st.bad_check == 0 &&
              st.overflowed == 0 && st.rejected_flags == 0;
    for (size_t i = 0; i < sizeof(st.in_progress); i++) ok = ok && st.in_progress[i] == 0;
    if (!ok) {
        std::printf("the whole stream: %zu samples, %u frames, %u skipped\n", whole.samples.size(), st.frames, st.skipped);
        return 1;
    }
    for (size_t cut = 0; cut <= stream.size(); cut++) {
        const Result r = run(stream, cut);
        if (r.samples.size() != whole.samples.size() ||
            std::memcmp(r.samples.data(), whole.samples.data(), r.samples.size() * sizeof(aof_imu_sample)) != 0 ||
            std::memcmp(&r.state, &whole.state, sizeof(r.state)) != 0) {
            std::printf("cut at %zu differs\n", cut);
            return 1;
        }
    }
    std::printf("%zu cuts of %zu bytes agree\n", stream.size() + 1, stream.size());
    return 0;
}

// what the device entry points of aof_mavlink_rx.cpp link against; never reached
namespace aof {
struct MavlinkRxArgs;
int precheck(aof_ctx *) { std::abort(); }
int ctx_fail(aof_ctx *, int, const char *) { std::abort(); }
int launch_bank_mavlink_rx(const MavlinkRxArgs &, void *) { std::abort(); }
int launch_bank_mavlink_rx_reset(aof_mavlink_rx_state *, const uint8_t *, uint32_t, void *) { std::abort(); }
}  // namespace aof
