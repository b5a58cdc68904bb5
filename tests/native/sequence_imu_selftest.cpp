// aof_sequence_imu_host (csrc/aof_sequence_imu.cpp over csrc/aof_imu_step.hpp and csrc/aof_mavlink.hpp) under ASan and UBSan,
// as a stand-alone program: the recordings of a listing that tests/test_sequence_imu_sanitized.py writes from the model's
// family (tests/sequence_imu_ref.py), every array allocated at its exact size on the heap, the outputs compared byte for
// byte with the model's, and the refusals of a recording whose sample_end decreases or whose records name a frame that is
// not there.  Usage: sequence_imu_selftest <listing>.  The listing, little-endian, per recording: u64 n, M, T, offset0,
// first_seq; u64 times[n]; samples[T] of 24 bytes; u32 sample_end[n]; records[n] of 32 bytes; then what the model wants:
// records[n], u8 frames[n][56] (0xA5 where nothing is written), u8 lengths[n], u32 sent, the 64-byte state.
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "aof.h"
#include "aof_host.hpp"
#include "aof_sequence_imu_args.hpp"

// the device side of the translation unit under test: never reached from here
namespace aof {
int precheck(aof_ctx *) { return -EIO; }
int ctx_fail(aof_ctx *, int code, const char *) { return code; }
int launch_sequence_imu(const SeqImuArgs &, void *) { return 1; }
}  // namespace aof
extern "C" int aof_get_params(const aof_ctx *, aof_params *) { return -EINVAL; }
extern "C" int aof_sequence_layout(const aof_params *, const aof_sequence_params *, int64_t, aof_seq_layout *) { return -EINVAL; }

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
    template <typename T> bool vec(std::vector<T> &v, size_t count)
    {
        v.resize(count);
        return take(v.data(), count * sizeof(T));
    }
};

int fail(const char *what, size_t index)
{
    std::printf("FAIL recording %zu: %s\n", index, what);
    return 1;
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
        uint64_t head[5];
        if (!in.take(head, sizeof(head))) return fail("short header", done);
        const size_t n = head[0], M = head[1], T = head[2];
        std::vector<uint64_t> times;
        std::vector<aof_imu_sample> samples;
        std::vector<uint32_t> sample_end;
        std::vector<aof_seq_record> records, want_records;
        std::vector<uint8_t> want_frames, want_lengths;
        uint32_t want_sent;
        aof_imu_state want_state;
        if (!in.vec(times, n) || !in.vec(samples, T) || !in.vec(sample_end, n) || !in.vec(records, n) || !in.vec(want_records, n) ||
            !in.vec(want_frames, n * AOF_SEQ_FRAME_BYTES) || !in.vec(want_lengths, n) || !in.take(&want_sent, 4) ||
            !in.take(&want_state, sizeof(want_state)))
            return fail("short listing", done);
        aof_seq_imu_params ip;
        std::memset(&ip, 0, sizeof(ip));
        ip.n_samples = (int64_t)T;
        ip.offset0 = head[3];
        ip.system_id = 1; ip.component_id = 100; ip.first_seq = (uint8_t)head[4];
        std::vector<uint8_t> frames(n * AOF_SEQ_FRAME_BYTES, 0xA5), lengths(n, 0);
        uint32_t count[4] = {(uint32_t)M, 0xEEEEEEEEu, 0x77u, 0x55u};
        aof_imu_state state;
        std::memset(&state, 0xEE, sizeof(state));
        const aof_imu_sample *sp = T ? samples.data() : nullptr;

        // the refusals first: nothing may be written
        if (n >= 2) {
            std::vector<uint32_t> bad(sample_end);
            bad[n - 1] = bad[n - 2] ? bad[n - 2] - 1 : 0;
            if (bad[n - 2]) {
                std::vector<aof_seq_record> r2(records);
                if (aof_sequence_imu_host(&ip, (int64_t)n, times.data(), sp, bad.data(), r2.data(), count, frames.data(), lengths.data(),
                                          &state) != -EINVAL)
                    return fail("a decreasing sample_end was accepted", done);
                refused++;
            }
        }
        if (M >= 1) {
            std::vector<aof_seq_record> r2(records);
            r2[M - 1].frame = (uint32_t)n;
            if (aof_sequence_imu_host(&ip, (int64_t)n, times.data(), sp, sample_end.data(), r2.data(), count, frames.data(), lengths.data(),
                                      &state) != -EINVAL)
                return fail("a record of a frame behind the recording was accepted", done);
            refused++;
        }
        for (uint8_t b : frames)
            if (b != 0xA5) return fail("a refused call wrote a frame byte", done);
        if (count[1] != 0xEEEEEEEEu) return fail("a refused call wrote count[1]", done);

        if (aof_sequence_imu_host(&ip, (int64_t)n, times.data(), sp, sample_end.data(), records.data(), count, frames.data(), lengths.data(),
                                  &state))
            return fail("the call was refused", done);
        if (n && std::memcmp(records.data(), want_records.data(), n * sizeof(aof_seq_record))) return fail("records differ", done);
        if (n && std::memcmp(frames.data(), want_frames.data(), frames.size())) return fail("frames differ", done);
        if (n && std::memcmp(lengths.data(), want_lengths.data(), n)) return fail("lengths differ", done);
        if (count[0] != M || count[1] != want_sent || count[2] != 0x77u || count[3] != 0x55u) return fail("count words differ", done);
        if (std::memcmp(&state, &want_state, sizeof(state))) return fail("final state differs", done);
        done++;
    }
    std::printf("agree: %zu recordings, %zu refusals\n", done, refused);
    return done ? 0 : 1;
}
