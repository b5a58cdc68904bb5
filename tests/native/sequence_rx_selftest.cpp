// aof_sequence_mavlink_rx_host (csrc/aof_sequence_mavlink_rx.cpp over csrc/aof_mavlink_rx_step.hpp) under ASan and UBSan, as a
// stand-alone program: the logs of a listing that tests/test_sequence_rx_sanitized.py writes from the model's family
// (tests/sequence_rx_ref.py) and from a few frames cut at every length, every array allocated at its exact size on the heap
// -- the log flush against the end of its allocation --, the outputs compared byte for byte with the model's, and refused
// calls that must write nothing.  Usage: sequence_rx_selftest <listing>.  The listing, little-endian, per log: u64 N, n, M,
// written; u8 log[N]; u32 byte_end[n]; then what the model wants: samples[written] of 24 bytes, u32 sample_end[n], the
// 128-byte state.
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "aof.h"
#include "aof_host.hpp"
#include "aof_sequence_mavlink_rx_args.hpp"

// the device side of the translation unit under test: never reached from here
namespace aof {
int precheck(aof_ctx *) { return -EIO; }
int ctx_fail(aof_ctx *, int code, const char *) { return code; }
int launch_sequence_mavlink_rx(const SeqRxArgs &, const SeqRxPlan &, void *) { return 1; }
}  // namespace aof

namespace {

struct Reader {
    std::vector<uint8_t> bytes;
    size_t at = 0;
    bool take(void *out, size_t n)
    {
        if (n > bytes.size() - at) return false;
        if (n) std::memcpy(out, bytes.data() + at, n);
        at += n;
        return true;
    }
};

int fail(const char *what, size_t index)
{
    std::printf("FAIL log %zu: %s\n", index, what);
    return 1;
}

bool all_are(const uint8_t *p, size_t n, uint8_t v)
{
    for (size_t i = 0; i < n; i++)
        if (p[i] != v) return false;
    return true;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    Reader in;
    if (FILE *f = std::fopen(argv[1], "rb")) {
        uint8_t block[65536];
        for (size_t n; (n = std::fread(block, 1, sizeof(block), f)) > 0;) in.bytes.insert(in.bytes.end(), block, block + n);
        std::fclose(f);
    } else {
        return 2;
    }
    size_t done = 0, refused = 0;
    while (in.at < in.bytes.size()) {
        uint64_t head[4];
        if (!in.take(head, sizeof(head))) return fail("short header", done);
        const size_t N = head[0], n = head[1], M = head[2], written = head[3];
        // exact sizes, and none of them a std::vector's (whose capacity may exceed its size)
        std::unique_ptr<uint8_t[]> log(new uint8_t[N]), samples(new uint8_t[M * 24]), want_samples(new uint8_t[written * 24]);
        std::unique_ptr<uint32_t[]> byte_end(new uint32_t[n]), sample_end(new uint32_t[n]), want_end(new uint32_t[n]);
        uint8_t want_state[128];
        aof_mavlink_rx_state state;
        if (!in.take(log.get(), N) || !in.take(byte_end.get(), 4 * n) || !in.take(want_samples.get(), 24 * written) ||
            !in.take(want_end.get(), 4 * n) || !in.take(want_state, 128) || written > M)
            return fail("short listing", done);
        std::memset(samples.get(), 0xEE, M * 24);
        std::memset(sample_end.get(), 0xEE, 4 * n);
        std::memset(&state, 0xEE, sizeof(state));
        aof_imu_sample *out = reinterpret_cast<aof_imu_sample *>(samples.get());
        const uint8_t *bytes = N ? log.get() : nullptr;
        const uint32_t *ends = n ? byte_end.get() : nullptr;
        uint32_t *out_end = n ? sample_end.get() : nullptr;

        // the refusals first: nothing may be written
        aof_seq_rx_params bad[4] = {{-1, (int64_t)M}, {(int64_t)N, 0}, {(int64_t)1 << 31, (int64_t)M}, {(int64_t)N, (int64_t)1 << 31}};
        for (const aof_seq_rx_params &rp : bad) {
            if (aof_sequence_mavlink_rx_host(&rp, (int64_t)n, bytes, ends, out, out_end, &state) != -EINVAL) return fail("a bad size was accepted", done);
            refused++;
        }
        aof_seq_rx_params rp = {(int64_t)N, (int64_t)M};
        if (aof_sequence_mavlink_rx_host(&rp, -1, bytes, ends, out, out_end, &state) != -EINVAL ||
            aof_sequence_mavlink_rx_host(nullptr, (int64_t)n, bytes, ends, out, out_end, &state) != -EINVAL ||
            aof_sequence_mavlink_rx_host(&rp, (int64_t)n, bytes, ends, nullptr, out_end, &state) != -EINVAL ||
            (N && aof_sequence_mavlink_rx_host(&rp, (int64_t)n, nullptr, ends, out, out_end, &state) != -EINVAL) ||
            (n && aof_sequence_mavlink_rx_host(&rp, (int64_t)n, bytes, ends, out, nullptr, &state) != -EINVAL))
            return fail("a null pointer or a negative frame count was accepted", done);
        refused += 3;
        if (!all_are(samples.get(), M * 24, 0xEE) || !all_are(reinterpret_cast<uint8_t *>(sample_end.get()), 4 * n, 0xEE) ||
            !all_are(reinterpret_cast<uint8_t *>(&state), sizeof(state), 0xEE))
            return fail("a refused call wrote something", done);

        if (aof_sequence_mavlink_rx_host(&rp, (int64_t)n, bytes, ends, out, out_end, &state)) return fail("the call was refused", done);
        if (written && std::memcmp(samples.get(), want_samples.get(), written * 24)) return fail("samples differ", done);
        if (!all_are(samples.get() + written * 24, (M - written) * 24, 0xEE)) return fail("a slot behind the written samples was written", done);
        if (n && std::memcmp(sample_end.get(), want_end.get(), 4 * n)) return fail("sample_end differs", done);
        if (std::memcmp(&state, want_state, 128)) return fail("the state differs", done);
        // without a state and without frames
        if (aof_sequence_mavlink_rx_host(&rp, 0, bytes, nullptr, out, nullptr, nullptr)) return fail("the call without frames was refused", done);
        if (written && std::memcmp(samples.get(), want_samples.get(), written * 24)) return fail("samples differ without frames", done);
        done++;
    }
    std::printf("agree: %zu logs, %zu refusals\n", done, refused);
    return done ? 0 : 1;
}
