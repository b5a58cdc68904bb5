// The stream bank's motion-field step (csrc/aof_bank_field_step.hpp -- include/aof.h "the stream bank's motion field") and the
// host loop around it (csrc/aof_bank_field.cpp over csrc/aof_field.cpp), compiled for the host under UBSan and ASan and held to
// ONE restatement of the four rules: a window of three pairs worked by hand, and a sweep of every quality code over frame
// counters 0, 1, 2 and beyond, valid and invalid fits, with and without a per-stream focal table, for several ticks on end,
// the pair's fit taken from aof_field_host.  Arrays are allocated at their exact size: a read outside them ends the run.
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "aof_bank_args.hpp"
#include "aof_bank_calls.hpp"
#include "aof_bank_field_step.hpp"
#include "aof_bank_tables.hpp"
#include "aof_host.hpp"

// what the device-side entry points of aof_field.cpp and aof_bank_field.cpp link against: not called here
namespace aof {
int precheck(aof_ctx *) { return -EIO; }
int ctx_fail(aof_ctx *, int code, const char *) { return code; }
int launch_field(const FieldArgs &, void *) { return 1; }
int launch_bank_field(const BankFieldArgs &, void *) { return 1; }
int launch_bank_imu_reset(aof_imu_state *, const uint8_t *, uint32_t, uint64_t, void *) { return 1; }
int bank_layout(const aof_params *, const aof_bank_params *, BankLayout *) { return -EINVAL; }
static BankCtx no_bank;
BankCtx &bank_ctx(aof_ctx *) { return no_bank; }
}  // namespace aof
extern "C" int aof_get_params(const aof_ctx *, aof_params *) { return -EINVAL; }

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static long checked = 0;
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

// ---- the rules, restated: every addition through a volatile, so that no compiler joins two roundings ----
struct Window {
    double zoom = 0, rotation = 0, cx = 0, cy = 0;
    uint32_t pairs = 0, fits = 0, used = 0, published = 0;
};

static bool same_bits(const void *a, const void *b, size_t n) { return std::memcmp(a, b, n) == 0; }

static int expect(const aof_tick_record &r, const aof_field &f, float fx, float fy, Window &w, const aof_bank_field_record &got,
                  const aof_field &got_field, const aof_bank_field_state &st, const aof_bank_field_state &before)
{
    aof_bank_field_record want;
    aof_field zero;
    std::memset(&want, 0, sizeof(want));
    std::memset(&zero, 0, sizeof(zero));
    if (r.quality == AOF_TICK_IDLE || r.quality == AOF_TICK_BAD_SENSOR) {
        want.status = r.quality;
        REQUIRE(same_bits(&want, &got, sizeof(want)) && same_bits(&zero, &got_field, sizeof(zero)) && same_bits(&st, &before, sizeof(st)));
        checked++;
        return 0;
    }
    const bool pair = r.frame >= 2;
    REQUIRE(same_bits(pair ? &f : &zero, &got_field, sizeof(zero)));
    if (pair) {
        w.pairs++;
        if (f.flags & AOF_FIELD_VALID) {
            w.fits++;
            w.used += f.used;
            volatile double z = w.zoom + (double)f.zoom, ro = w.rotation + (double)f.rotation;
            volatile double x = w.cx + (double)f.centre_x, y = w.cy + (double)f.centre_y;
            w.zoom = z; w.rotation = ro; w.cx = x; w.cy = y;
        }
    }
    want.status = AOF_TICK_HELD;
    want.frame = r.frame;
    if (r.quality >= 0 || r.quality == AOF_TICK_STALE_GYRO || r.quality == AOF_TICK_NO_OFFSET) {
        want.status = (int32_t)w.fits;
        want.dt_us = r.dt_us;
        want.zoom = (float)w.zoom; want.rotation = (float)w.rotation; want.centre_x = (float)w.cx; want.centre_y = (float)w.cy;
        want.flow_x = aof_atan2f(want.centre_x, fx);
        want.flow_y = aof_atan2f(want.centre_y, fy);
        REQUIRE(std::fabs((double)want.flow_x - std::atan2((double)want.centre_x, (double)fx)) < 1e-6);
        want.pairs = w.pairs; want.fits = w.fits; want.used = w.used;
        const uint32_t n = w.published + 1;
        w = Window();
        w.published = n;
    }
    REQUIRE(same_bits(&want, &got, sizeof(want)));
    REQUIRE(same_bits(&st.sum_zoom, &w.zoom, 8) && same_bits(&st.sum_rotation, &w.rotation, 8) && same_bits(&st.sum_centre_x, &w.cx, 8) &&
            same_bits(&st.sum_centre_y, &w.cy, 8));
    REQUIRE(st.pairs == w.pairs && st.fits == w.fits && st.used == w.used && st.published == w.published);
    REQUIRE(same_bits(st.reserved, before.reserved, sizeof(st.reserved)));
    checked++;
    return 0;
}

// ---- the window by hand: dense 64 x 64, 7 x 7 blocks at X, Y = -48 .. 48 in steps of 16 half-pixels ----
static int hand_window()
{
    aof_params p;
    aof_params_default(&p, 64, 64);
    aof_field_params fp;
    aof_field_params_default(&fp);
    aof_bank_params bp;
    std::memset(&bp, 0, sizeof(bp));
    bp.n_streams = 1; bp.focal_x = 100.0f; bp.focal_y = 50.0f;
    aof_bank_field_state st;
    std::memset(&st, 0, sizeof(st));
    const int qualities[3] = {AOF_TICK_HELD, AOF_TICK_HELD, 180};
    aof_bank_field_record out[3];
    aof_field f[3];
    for (int k = 0; k < 3; k++) {
        std::vector<aof_block> blocks(49);
        for (int i = 0; i < 49; i++) {
            const int X = 16 * (i % 7) - 48, Y = 16 * (i / 7) - 48;
            // a zoom of 1/8, a rotation of -1/8, a shift of (6, 2) half-pixels
            const int U = k == 0 ? X / 8 : (k == 1 ? Y / 8 : 6), V = k == 0 ? Y / 8 : (k == 1 ? -X / 8 : 2);
            blocks[i].dx = (int8_t)(U / 2); blocks[i].dy = (int8_t)(V / 2); blocks[i].sad = 100;
        }
        aof_tick_record r;
        std::memset(&r, 0, sizeof(r));
        r.quality = qualities[k]; r.dt_us = k == 2 ? 66667 : 0; r.frame = (uint32_t)k + 2;
        REQUIRE(aof_bank_field_host(&p, &bp, nullptr, &fp, blocks.data(), nullptr, &r, &st, &f[k], &out[k]) == 0);
    }
    REQUIRE(f[0].zoom == 0.125f && f[0].rotation == 0.0f && f[1].zoom == 0.0f && f[1].rotation == -0.125f);
    REQUIRE(f[2].centre_x == 3.0f && f[2].centre_y == 1.0f && f[0].used == 49 && f[1].used == 49 && f[2].used == 49);
    for (int k = 0; k < 2; k++)
        REQUIRE(out[k].status == AOF_TICK_HELD && out[k].frame == (uint32_t)k + 2 && out[k].pairs == 0 && out[k].zoom == 0.0f && out[k].dt_us == 0);
    REQUIRE(out[2].status == 3 && out[2].dt_us == 66667 && out[2].pairs == 3 && out[2].fits == 3 && out[2].used == 147 && out[2].frame == 4);
    REQUIRE(out[2].zoom == 0.125f && out[2].rotation == -0.125f && out[2].centre_x == 3.0f && out[2].centre_y == 1.0f);
    REQUIRE(std::fabs((double)out[2].flow_x - std::atan2(3.0, 100.0)) < 1e-7 && std::fabs((double)out[2].flow_y - std::atan2(1.0, 50.0)) < 1e-7);
    REQUIRE(st.pairs == 0 && st.fits == 0 && st.used == 0 && st.published == 1 && st.sum_zoom == 0.0 && st.sum_centre_x == 0.0);
    checked += 3;
    return 0;
}

// ---- every quality code x frame counter x fit, several ticks on end ----
static int sweep(const aof_params &p, bool table)
{
    aof_field_params fp;
    aof_field_params_default(&fp);
    int32_t x0, y0, sx, sy, nx, ny;
    REQUIRE(aof_grid(&p, 0, &x0, &y0, &sx, &sy, &nx, &ny) == 0);
    const size_t nb = (size_t)nx * ny;
    const int quality[8] = {200, 0, AOF_TICK_HELD, AOF_TICK_IDLE, AOF_TICK_BAD_SENSOR, AOF_TICK_STALE_GYRO, AOF_TICK_NO_OFFSET, 255};
    const uint32_t frames[4] = {0, 1, 2, 4000000000u};
    const int S = 8 * 4;
    aof_bank_params bp;
    std::memset(&bp, 0, sizeof(bp));
    bp.n_streams = S; bp.focal_x = 216.6677f; bp.focal_y = 216.2457f;
    std::vector<aof_bank_stream> streams((size_t)S);
    for (int s = 0; s < S; s++) {
        std::memset(&streams[s], 0, sizeof(aof_bank_stream));
        streams[s].focal_x = 90.0f + 7.5f * s; streams[s].focal_y = 400.0f - 3.25f * s;
    }
    std::vector<aof_bank_field_state> st((size_t)S);
    std::vector<Window> win((size_t)S);
    std::memset(st.data(), 0, st.size() * sizeof(st[0]));
    for (int s = 0; s < S; s++) std::memset(st[s].reserved, 0x5A, sizeof(st[s].reserved));
    for (int tick = 0; tick < 9; tick++) {
        std::vector<aof_block> blocks(nb * S);
        std::vector<uint8_t> subdirs(nb * S);
        std::vector<aof_tick_record> rec((size_t)S);
        std::vector<aof_field> fields((size_t)S), pairwise((size_t)S);
        std::vector<aof_flow> flows((size_t)S);
        std::vector<aof_bank_field_record> out((size_t)S);
        for (int s = 0; s < S; s++) {
            std::memset(&rec[s], 0, sizeof(rec[s]));
            rec[s].quality = quality[(s + tick) % 8];
            rec[s].frame = frames[(s / 8 + tick / 3) % 4];
            rec[s].dt_us = (int32_t)(rnd() % 200000);
            rec[s].pixel.pred_x = (int8_t)(s % 3 - 1); rec[s].pixel.pred_y = (int8_t)(tick % 2);
            flows[s] = rec[s].pixel;
            const bool invalid = (s + 2 * tick) % 5 == 0;   // every record skipped: the fit cannot be valid
            const int tx = (int)(rnd() % 5) - 2, ty = (int)(rnd() % 5) - 2;
            for (size_t k = 0; k < nb; k++) {
                aof_block &b = blocks[s * nb + k];
                const uint64_t r = rnd();
                b.dx = (int8_t)(tx + (int)(r % 3) - 1); b.dy = (int8_t)(ty + (int)((r >> 8) % 3) - 1);
                b.sad = invalid ? 0xFFFF : (uint16_t)((r >> 16) % 2900);
                subdirs[s * nb + k] = (uint8_t)((r >> 40) % 10);
            }
        }
        const std::vector<aof_bank_field_state> before = st;
        REQUIRE(aof_field_host(&p, &fp, blocks.data(), p.subpixel ? subdirs.data() : nullptr, flows.data(), S, pairwise.data()) == 0);
        REQUIRE(aof_bank_field_host(&p, &bp, table ? streams.data() : nullptr, &fp, blocks.data(), subdirs.data(), rec.data(), st.data(),
                                    fields.data(), out.data()) == 0);
        for (int s = 0; s < S; s++)
            if (expect(rec[s], pairwise[s], table ? streams[s].focal_x : bp.focal_x, table ? streams[s].focal_y : bp.focal_y, win[s], out[s],
                       fields[s], st[s], before[s]))
                return 1;
        // fields = NULL: the same records, the same state
        std::vector<aof_bank_field_state> again = before;
        std::vector<aof_bank_field_record> out2((size_t)S);
        REQUIRE(aof_bank_field_host(&p, &bp, table ? streams.data() : nullptr, &fp, blocks.data(), subdirs.data(), rec.data(), again.data(),
                                    nullptr, out2.data()) == 0);
        REQUIRE(same_bits(again.data(), st.data(), st.size() * sizeof(st[0])) && same_bits(out2.data(), out.data(), out.size() * sizeof(out[0])));
    }
    uint32_t published = 0, valid_windows = 0;
    for (int s = 0; s < S; s++) published += st[s].published;
    for (int s = 0; s < S; s++) valid_windows += win[s].fits;
    REQUIRE(published > (uint32_t)S);
    (void)valid_windows;
    return 0;
}

int main()
{
    if (hand_window()) return 1;
    aof_params p;
    aof_params_px4flow(&p, 64, 64, 4, 30, 3000);      // sub-pixel: the sub-directions reach the fit
    if (sweep(p, false) || sweep(p, true)) return 1;
    aof_params_default(&p, 144, 136);                 // 272 blocks, no sub-pixel context: the sub-directions are not read
    if (sweep(p, true)) return 1;
    // refusals
    aof_field_params fp;
    aof_field_params_default(&fp);
    aof_bank_params bp;
    std::memset(&bp, 0, sizeof(bp));
    bp.n_streams = 1; bp.focal_x = bp.focal_y = 200.0f;
    std::vector<aof_block> b(272);
    aof_tick_record r;
    std::memset(&r, 0, sizeof(r));
    aof_bank_field_state st;
    std::memset(&st, 0, sizeof(st));
    aof_bank_field_record o;
    REQUIRE(aof_bank_field_host(&p, &bp, nullptr, &fp, b.data(), nullptr, &r, &st, nullptr, &o) == 0 && o.status == 0 && st.published == 1);
    REQUIRE(aof_bank_field_host(nullptr, &bp, nullptr, &fp, b.data(), nullptr, &r, &st, nullptr, &o) == -EINVAL);
    REQUIRE(aof_bank_field_host(&p, &bp, nullptr, &fp, b.data(), nullptr, &r, &st, nullptr, nullptr) == -EINVAL);
    bp.n_streams = 0;
    REQUIRE(aof_bank_field_host(&p, &bp, nullptr, &fp, b.data(), nullptr, &r, &st, nullptr, &o) == -EINVAL);
    bp.n_streams = 1; fp.passes = 3;
    REQUIRE(aof_bank_field_host(&p, &bp, nullptr, &fp, b.data(), nullptr, &r, &st, nullptr, &o) == -EINVAL);
    fp.passes = 2;
    REQUIRE(aof_bank_field_device(nullptr, &bp, &fp, b.data(), 0, &r, &st, nullptr, &o, nullptr) == -EINVAL);
    REQUIRE(aof_bank_field_reset_device(nullptr, 1, nullptr, &st, nullptr) == -EINVAL);
    REQUIRE(st.published == 1);
    std::printf("bank field step and its restatement agree on %ld stream ticks\n", checked);
    return 0;
}
