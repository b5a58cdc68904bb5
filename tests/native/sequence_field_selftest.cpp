// aof_sequence_field_host (csrc/aof_sequence_field.cpp over csrc/aof_bank_field_step.hpp and csrc/aof_field.cpp) under ASan and
// UBSan, as a stand-alone program: recordings of made-up block records and record lists -- windows of 1, 2, 5, 63, 64, 65 and
// 300 pairs, windows without a valid fit, a record per frame, empty and long tails, one frame, no frame --, every array
// allocated at its exact size on the heap, the outputs compared byte for byte with the frame-by-frame loop the contract
// names: aof_field_host for the fits, then bank_field_step for every frame with a held tick or the record's.  Then the
// refusals, which must write nothing.
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "aof_bank_field_step.hpp"
#include "aof_host.hpp"
#include "aof_sequence_field_args.hpp"

// the device side of the translation units under test: never reached from here
namespace aof {
int precheck(aof_ctx *) { return -EIO; }
int ctx_fail(aof_ctx *, int code, const char *) { return code; }
int launch_field(const FieldArgs &, void *) { return 1; }
int launch_sequence_field(const SeqFieldArgs &, void *) { return 1; }
}  // namespace aof
extern "C" int aof_get_params(const aof_ctx *, aof_params *) { return -EINVAL; }
extern "C" int aof_sequence_layout(const aof_params *, const aof_sequence_params *, int64_t, aof_seq_layout *) { return -EINVAL; }

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static long records_checked = 0, pairs_checked = 0;

static aof_sequence_params sequence_params(const aof_params &p, float fx, float fy)
{
    aof_sequence_params sp;
    std::memset(&sp, 0, sizeof(sp));
    sp.ingest.camera_width = sp.ingest.crop_width = p.width;
    sp.ingest.camera_height = sp.ingest.crop_height = p.height;
    sp.focal_x = fx; sp.focal_y = fy; sp.output_rate = 15;
    return sp;
}

// windows: the pairs in front of every record behind record 0 (frame 0); tail: the pairs behind the last record
static int recording(const aof_params &p, const std::vector<uint32_t> &windows, uint32_t tail, bool record0)
{
    aof_field_params fp;
    aof_field_params_default(&fp);
    int32_t x0, y0, sx, sy, nx, ny;
    REQUIRE(aof_grid(&p, 0, &x0, &y0, &sx, &sy, &nx, &ny) == 0);
    const size_t nb = (size_t)nx * ny;
    std::vector<aof_seq_record> records;
    uint32_t frame = 0;
    if (record0) records.push_back(aof_seq_record{0, 0, 0, 0, 0, 0, 0, 0});
    for (uint32_t w : windows) {
        frame += w;
        const int32_t quality[4] = {200, AOF_TICK_STALE_GYRO, 0, AOF_TICK_NO_OFFSET};
        records.push_back(aof_seq_record{frame, quality[rnd() % 4], (int32_t)(rnd() % 300000), 0.01f, -0.02f, 0.1f, 0.2f, 0.3f});
    }
    const size_t n = (size_t)frame + tail + 1, pairs = n - 1, M = records.size();
    std::vector<aof_block> blocks(pairs * nb);
    std::vector<uint8_t> subdirs(pairs * nb);
    std::vector<aof_flow> flows(pairs);
    for (size_t k = 0; k < pairs; k++) {
        const bool invalid = rnd() % 4 == 0 || (k >= 7 && k < 12);   // every record skipped: no fit (pairs 7..11: a whole window)
        const int tx = (int)(rnd() % 5) - 2, ty = (int)(rnd() % 5) - 2;
        std::memset(&flows[k], 0, sizeof(aof_flow));
        flows[k].pred_x = (int8_t)(k % 3 - 1); flows[k].pred_y = (int8_t)(k % 2);
        for (size_t i = 0; i < nb; i++) {
            const uint64_t r = rnd();
            aof_block &b = blocks[k * nb + i];
            b.dx = (int8_t)(tx + (int)(r % 3) - 1); b.dy = (int8_t)(ty + (int)((r >> 8) % 3) - 1);
            b.sad = invalid ? 0xFFFF : (uint16_t)((r >> 16) % 2900);
            subdirs[k * nb + i] = (uint8_t)((r >> 40) % 10);
        }
    }
    const aof_sequence_params sp = sequence_params(p, 216.6677f, 180.25f);

    // the loop the contract names
    std::vector<aof_field> want_fields(pairs);
    if (pairs) REQUIRE(aof_field_host(&p, &fp, blocks.data(), p.subpixel ? subdirs.data() : nullptr, flows.data(), (int64_t)pairs, want_fields.data()) == 0);
    std::vector<aof_bank_field_record> want_out(M);
    aof_bank_field_state want_state;
    std::memset(&want_state, 0, sizeof(want_state));
    size_t m = 0;
    for (size_t j = 0; j < n; j++) {
        aof::BankFieldTick tick{AOF_TICK_HELD, 0, (uint32_t)j, 0, 0};
        const bool record = m < M && records[m].frame == j;
        if (record) { tick.quality = records[m].quality; tick.dt_us = records[m].dt_us; }
        aof_field none;
        std::memset(&none, 0, sizeof(none));
        const aof_bank_field_record o = aof::bank_field_step(tick, j >= 1, j >= 1 ? want_fields[j - 1] : none, sp.focal_x, sp.focal_y, want_state);
        if (record) want_out[m++] = o;
    }
    REQUIRE(m == M && want_state.published == M && want_state.pairs == (M ? tail : (uint32_t)pairs));

    std::vector<aof_field> fields(pairs);
    std::vector<aof_bank_field_record> out(M);
    aof_bank_field_state state;
    if (pairs) std::memset(fields.data(), 0xEE, pairs * sizeof(aof_field));
    if (M) std::memset(out.data(), 0xEE, M * sizeof(out[0]));
    std::memset(&state, 0xEE, sizeof(state));
    aof_bank_field_record no_out;
    REQUIRE(aof_sequence_field_host(&p, &sp, &fp, (int64_t)n, pairs ? blocks.data() : nullptr, pairs ? subdirs.data() : nullptr,
                                    pairs ? flows.data() : nullptr, M ? records.data() : nullptr, (uint32_t)M, pairs ? fields.data() : nullptr,
                                    M ? out.data() : &no_out, &state) == 0);
    REQUIRE(!pairs || std::memcmp(fields.data(), want_fields.data(), pairs * sizeof(aof_field)) == 0);
    REQUIRE(!M || std::memcmp(out.data(), want_out.data(), M * sizeof(out[0])) == 0);
    REQUIRE(std::memcmp(&state, &want_state, sizeof(state)) == 0);
    // without a state: the same records
    std::vector<aof_bank_field_record> out2(M);
    REQUIRE(aof_sequence_field_host(&p, &sp, &fp, (int64_t)n, pairs ? blocks.data() : nullptr, pairs ? subdirs.data() : nullptr,
                                    pairs ? flows.data() : nullptr, M ? records.data() : nullptr, (uint32_t)M, pairs ? fields.data() : nullptr,
                                    M ? out2.data() : &no_out, nullptr) == 0);
    REQUIRE(!M || std::memcmp(out2.data(), want_out.data(), M * sizeof(out[0])) == 0);

    // refusals write nothing
    if (M >= 2 && pairs) {
        const std::vector<aof_field> f0 = fields;
        const aof_bank_field_state s0 = state;
        std::vector<aof_seq_record> r2 = records;
        r2[M - 1].frame = (uint32_t)n;
        REQUIRE(aof_sequence_field_host(&p, &sp, &fp, (int64_t)n, blocks.data(), subdirs.data(), flows.data(), r2.data(), (uint32_t)M, fields.data(),
                                        out.data(), &state) == -EINVAL);
        r2[M - 1].frame = r2[M - 2].frame;
        REQUIRE(aof_sequence_field_host(&p, &sp, &fp, (int64_t)n, blocks.data(), subdirs.data(), flows.data(), r2.data(), (uint32_t)M, fields.data(),
                                        out.data(), &state) == -EINVAL);
        REQUIRE(aof_sequence_field_host(&p, &sp, &fp, (int64_t)M - 1, blocks.data(), subdirs.data(), flows.data(), records.data(), (uint32_t)M,
                                        fields.data(), out.data(), &state) == -EINVAL);
        REQUIRE(aof_sequence_field_host(&p, &sp, &fp, (int64_t)n, nullptr, subdirs.data(), flows.data(), records.data(), (uint32_t)M, fields.data(),
                                        out.data(), &state) == -EINVAL);
        REQUIRE(aof_sequence_field_host(&p, &sp, &fp, (int64_t)n, blocks.data(), subdirs.data(), flows.data(), records.data(), (uint32_t)M, fields.data(),
                                        nullptr, &state) == -EINVAL);
        REQUIRE(std::memcmp(fields.data(), f0.data(), pairs * sizeof(aof_field)) == 0 && std::memcmp(&state, &s0, sizeof(state)) == 0);
        REQUIRE(std::memcmp(out.data(), want_out.data(), M * sizeof(out[0])) == 0);
    }
    records_checked += (long)M;
    pairs_checked += (long)pairs;
    return 0;
}

int main()
{
    aof_params px4, dense;
    aof_params_px4flow(&px4, 64, 64, 4, 30, 3000);    // 25 blocks, sub-pixel: the sub-directions reach the fit
    aof_params_default(&dense, 144, 136);             // 272 blocks, no sub-pixel context: the sub-directions are not read
    if (recording(px4, {3, 4, 5, 1, 2, 63, 64, 65, 300, 1, 1}, 0, true)) return 1;
    if (recording(px4, {5, 5, 5, 5}, 1, true)) return 1;
    if (recording(px4, std::vector<uint32_t>(40, 1), 0, true)) return 1;      // a record per frame
    if (recording(px4, {2, 2}, 700, true)) return 1;                          // a stalled recording's tail
    if (recording(px4, {}, 0, true)) return 1;                                // one frame
    if (recording(px4, {}, 9, false)) return 1;                               // nothing published
    if (recording(dense, {4, 3, 6, 1}, 2, true)) return 1;
    // no frames: nothing to do, nothing written
    aof_field_params fp;
    aof_field_params_default(&fp);
    const aof_sequence_params sp = sequence_params(px4, 200.0f, 200.0f);
    aof_bank_field_record o;
    aof_bank_field_state st;
    std::memset(&o, 0xEE, sizeof(o));
    std::memset(&st, 0xEE, sizeof(st));
    const aof_bank_field_state st0 = st;
    REQUIRE(aof_sequence_field_host(&px4, &sp, &fp, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &o, &st) == 0);
    REQUIRE(aof_sequence_field_host(nullptr, &sp, &fp, 1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &o, &st) == -EINVAL);
    REQUIRE(aof_sequence_field_host(&px4, nullptr, &fp, 1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &o, &st) == -EINVAL);
    REQUIRE(aof_sequence_field_host(&px4, &sp, nullptr, 1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &o, &st) == -EINVAL);
    fp.passes = 3;
    REQUIRE(aof_sequence_field_host(&px4, &sp, &fp, 1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &o, &st) == -EINVAL);
    fp.passes = 2;
    REQUIRE(aof_sequence_field_host(&px4, &sp, &fp, 1, nullptr, nullptr, nullptr, nullptr, 1, nullptr, &o, &st) == -EINVAL);   // records NULL
    REQUIRE(aof_sequence_field_device(nullptr, &sp, &fp, 1, &st, 64, nullptr, &o, &st, nullptr) == -EINVAL);
    REQUIRE(std::memcmp(&st, &st0, sizeof(st)) == 0 && o.status == (int32_t)0xEEEEEEEE);
    std::printf("agree: %ld records over %ld pairs\n", records_checked, pairs_checked);
    return 0;
}
