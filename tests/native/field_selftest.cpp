// The motion-field rule (csrc/aof_field_step.hpp -- include/aof.h "the motion FIELD of a batch") and the host side around it
// (csrc/aof_field.cpp: the geometry and its range check, the plain loop), compiled for the host under UBSan and ASan and
// held to ONE restatement whose integers are __int128: every sum, product and determinant is formed there without any
// bound, must fit int64, and must be what the record holds.  Geometries: the largest dense grid the range check admits
// (4096 x 4096, 261 121 blocks), a sparse grid of odd step whose determinants beyond 2^53 need rounding (206 116 blocks),
// VGA and the 64 x 64 grid; records: shifts at the ends of int8 pointing away from the centre everywhere (the largest sums
// there are), random records with every sub-direction and SADs around both gates.  A step that wrapped ends the run, as
// does a read outside the arrays, which are allocated at their exact size.
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "aof_field_step.hpp"
#include "aof_host.hpp"

// what aof_field.cpp's device-side entry point links against: not called here
namespace aof {
int precheck(aof_ctx *) { return -EIO; }
int ctx_fail(aof_ctx *, int code, const char *) { return code; }
int launch_field(const FieldArgs &, void *) { return 1; }
}  // namespace aof
extern "C" int aof_get_params(const aof_ctx *, aof_params *) { return -EINVAL; }

typedef __int128 i128;
static long checked = 0;
static bool saw_det_beyond_53 = false;
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static bool fits64(i128 v) { return v >= (i128)INT64_MIN && v <= (i128)INT64_MAX; }

struct Sums128 {
    i128 n = 0, SX = 0, SY = 0, SU = 0, SV = 0, Q = 0, A = 0, C = 0;
    void add(i128 X, i128 Y, i128 U, i128 V) { n += 1; SX += X; SY += Y; SU += U; SV += V; Q += X * X + Y * Y; A += X * U + Y * V; C += X * V - Y * U; }
};

struct Model128 {
    i128 D, Na, Nb;
    double a = 0, b = 0, tU = 0, tV = 0;
    bool fits;
};

static int solve(const Sums128 &s, int min_blocks, Model128 *m)
{
    m->D = s.n * s.Q - s.SX * s.SX - s.SY * s.SY;
    m->Na = s.n * s.A - s.SX * s.SU - s.SY * s.SV;
    m->Nb = s.n * s.C - s.SX * s.SV + s.SY * s.SU;
    // nothing the rule forms may leave int64
    REQUIRE(fits64(s.n * s.Q) && fits64(s.n * s.A) && fits64(s.n * s.C) && fits64(s.SX * s.SX) && fits64(s.SY * s.SY));
    REQUIRE(fits64(s.n * s.Q - s.SX * s.SX) && fits64(s.n * s.A - s.SX * s.SU) && fits64(s.n * s.C - s.SX * s.SV));
    REQUIRE(fits64(s.SX * s.SU) && fits64(s.SY * s.SV) && fits64(s.SX * s.SV) && fits64(s.SY * s.SU));
    REQUIRE(fits64(m->D) && fits64(m->Na) && fits64(m->Nb) && m->D >= 0);
    m->fits = s.n >= min_blocks && m->D > 0;
    if (m->fits) {
        m->a = (double)m->Na / (double)m->D;
        m->b = (double)m->Nb / (double)m->D;
        volatile double aSX = m->a * (double)s.SX, bSY = m->b * (double)s.SY, bSX = m->b * (double)s.SX, aSY = m->a * (double)s.SY;
        volatile double u1 = (double)s.SU - aSX, v1 = (double)s.SV - bSX;
        volatile double u2 = u1 + bSY, v2 = v1 - aSY;
        m->tU = u2 / (double)s.n;
        m->tV = v2 / (double)s.n;
    }
    return 0;
}

static const int kHalf[9][2] = {{1, 0}, {1, 1}, {0, 1}, {-1, 1}, {-1, 0}, {-1, -1}, {0, -1}, {1, -1}, {0, 0}};

static int check_pair(const aof_params &p, const aof_field_params &fp, const aof_block *blocks, const uint8_t *subdirs, const aof_flow &flow,
                      const aof_field &got, bool *beyond53)
{
    int32_t x0, y0, sx, sy, nx, ny;
    REQUIRE(aof_grid(&p, 0, &x0, &y0, &sx, &sy, &nx, &ny) == 0);
    const int vthr = p.value_threshold > 0xFFFF ? 0xFFFF : p.value_threshold;
    const int nb = nx * ny;
    std::vector<char> member((size_t)nb);
    std::vector<int> U((size_t)nb), V((size_t)nb);
    auto X = [&](int k) { return (i128)2 * (x0 + (k % nx) * (i128)sx) + p.tile - p.width; };
    auto Y = [&](int k) { return (i128)2 * (y0 + (k / nx) * (i128)sy) + p.tile - p.height; };
    Sums128 s1;
    uint32_t accepted = 0, at_reach = 0;
    for (int k = 0; k < nb; k++) {
        const int sd = subdirs && subdirs[k] < 8 ? subdirs[k] : 8;
        U[k] = 2 * blocks[k].dx + kHalf[sd][0];
        V[k] = 2 * blocks[k].dy + kHalf[sd][1];
        const bool ok = blocks[k].sad != 0xFFFF && (int)blocks[k].sad < vthr;
        const bool reach = ok && (std::abs(blocks[k].dx - flow.pred_x) == p.search || std::abs(blocks[k].dy - flow.pred_y) == p.search);
        accepted += ok; at_reach += reach;
        member[k] = ok && !(fp.exclude_reach && reach);
        if (member[k]) s1.add(X(k), Y(k), U[k], V[k]);
    }
    Model128 m1, pub;
    if (solve(s1, fp.min_blocks, &m1)) return 1;
    REQUIRE(got.accepted == accepted && got.at_reach == at_reach && got.reserved == 0);
    if (!m1.fits) {
        aof_field zero;
        std::memset(&zero, 0, sizeof(zero));
        zero.accepted = accepted; zero.at_reach = at_reach;
        REQUIRE(std::memcmp(&zero, &got, sizeof(zero)) == 0);
        checked++;
        return 0;
    }
    pub = m1;
    i128 used = s1.n;
    uint32_t flags = AOF_FIELD_VALID;
    if (fp.passes == 2) {
        const double g = 2.0 * (double)fp.gate_px;
        Sums128 s2;
        for (int k = 0; k < nb; k++) {
            if (!member[k]) continue;
            const double x = (double)(int64_t)X(k), y = (double)(int64_t)Y(k);
            volatile double aX = m1.a * x, bY = m1.b * y, bX = m1.b * x, aY = m1.a * y;
            volatile double mu = m1.tU + aX, mv = m1.tV + bX;
            volatile double mu2 = mu - bY, mv2 = mv + aY;
            volatile double ru = (double)U[k] - mu2, rv = (double)V[k] - mv2;
            if (std::fabs(ru) <= g && std::fabs(rv) <= g) s2.add(X(k), Y(k), U[k], V[k]);
        }
        Model128 m2;
        if (solve(s2, fp.min_blocks, &m2)) return 1;
        if (m2.fits) { pub = m2; used = s2.n; flags |= AOF_FIELD_REFIT; }
    }
    REQUIRE(got.det == (int64_t)pub.D && got.num_zoom == (int64_t)pub.Na && got.num_rot == (int64_t)pub.Nb);
    REQUIRE(got.fitted == (uint32_t)s1.n && got.used == (uint32_t)used && got.flags == flags);
    const float zoom = (float)pub.a, rot = (float)pub.b, cx = (float)(pub.tU * 0.5), cy = (float)(pub.tV * 0.5);
    REQUIRE(std::memcmp(&zoom, &got.zoom, 4) == 0 && std::memcmp(&rot, &got.rotation, 4) == 0);
    REQUIRE(std::memcmp(&cx, &got.centre_x, 4) == 0 && std::memcmp(&cy, &got.centre_y, 4) == 0);
    const i128 two53 = (i128)1 << 53;
    if (pub.D > two53) saw_det_beyond_53 = true;
    if (pub.D > two53 && (pub.Na > two53 || pub.Na < -two53) && (i128)(double)(int64_t)pub.D != pub.D) *beyond53 = true;
    checked++;
    return 0;
}

static int run(const aof_params &p, int pairs, bool expect53)
{
    REQUIRE(aof_params_check(&p) == 0 && aof_field_supported(&p) == 0);
    int32_t x0, y0, sx, sy, nx, ny;
    REQUIRE(aof_grid(&p, 0, &x0, &y0, &sx, &sy, &nx, &ny) == 0);
    const size_t nb = (size_t)nx * ny;
    bool beyond53 = false;
    for (int design = 0; design < 3; design++) {
        // exact sizes: a read past the last record or sub-direction is ASan's
        std::vector<aof_block> blocks(nb * pairs);
        std::vector<uint8_t> subdirs(nb * pairs);
        std::vector<aof_flow> flows((size_t)pairs);
        std::vector<aof_field> out((size_t)pairs);
        for (int i = 0; i < pairs; i++) {
            std::memset(&flows[i], 0, sizeof(aof_flow));
            flows[i].pred_x = (int8_t)(i % 3 - 1); flows[i].pred_y = (int8_t)(2 * (i % 2));
            for (size_t k = 0; k < nb; k++) {
                aof_block &b = blocks[i * nb + k];
                const int64_t X = 2 * (x0 + (int64_t)(k % nx) * sx) + p.tile - p.width, Y = 2 * (y0 + (int64_t)(k / nx) * sy) + p.tile - p.height;
                const uint64_t r = rnd();
                if (design == 0) {          // away from the centre at the ends of int8: the largest |A|; a tenth skipped
                    b.dx = X > 0 ? 127 : -128; b.dy = Y > 0 ? 127 : -128; b.sad = r % 10 == 0 ? 0xFFFF : 0;
                    subdirs[i * nb + k] = X > 0 ? 1 : 5;
                } else if (design == 1) {   // a vortex at the ends of int8: the largest |C|
                    b.dx = Y > 0 ? -128 : 127; b.dy = X > 0 ? 127 : -128; b.sad = (uint16_t)(r % 3000);
                    subdirs[i * nb + k] = (uint8_t)(r >> 20) % 9;
                } else {                    // every record on its own
                    b.dx = (int8_t)((r >> 8) % (2 * p.search + 1)) - p.search; b.dy = (int8_t)((r >> 16) % (2 * p.search + 1)) - p.search;
                    const uint16_t edge[5] = {0, (uint16_t)(p.value_threshold - 1), (uint16_t)p.value_threshold, 0xFFFE, 0xFFFF};
                    b.sad = (r >> 24) % 4 == 0 ? edge[(r >> 32) % 5] : (uint16_t)((r >> 32) % 3000);
                    subdirs[i * nb + k] = (uint8_t)((r >> 48) % 10);   // (9: above the table, no half step)
                }
            }
        }
        for (int variant = 0; variant < 4; variant++) {
            aof_field_params fp;
            REQUIRE(aof_field_params_default(&fp) == 0);
            fp.passes = 1 + variant % 2;
            fp.exclude_reach = variant / 2;
            if (design < 2) fp.gate_px = 600.0f;   // (the extreme fields are no similarity: a gate that keeps them)
            const bool with_sub = variant != 1;
            REQUIRE(aof_field_host(&p, &fp, blocks.data(), with_sub ? subdirs.data() : nullptr, flows.data(), pairs, out.data()) == 0);
            for (int i = 0; i < pairs; i++)
                if (check_pair(p, fp, &blocks[i * nb], with_sub ? &subdirs[i * nb] : nullptr, flows[i], out[i], &beyond53)) return 1;
        }
    }
    REQUIRE(beyond53 == expect53);
    return 0;
}

int main()
{
    aof_params p;
    // the largest dense grid both checks accept; the same frame is refused one power of two wider
    aof_params_default(&p, 4096, 4096);
    if (run(p, 1, false)) return 1;   // (X, Y multiples of 16: D beyond 2^53 converts exactly)
    REQUIRE(saw_det_beyond_53);
    aof_params_default(&p, 8192, 2048);
    REQUIRE(aof_params_check(&p) == 0 && aof_field_supported(&p) == -EINVAL);
    // a sparse grid of step 9: D and Na beyond 2^53 that have to be rounded
    aof_params_px4flow(&p, 4096, 4096, 4, 30, 3000);
    p.num_blocks = 500;
    if (run(p, 1, true)) return 1;
    aof_params_default(&p, 640, 480);
    if (run(p, 3, false)) return 1;
    aof_params_default(&p, 1280, 960);
    p.tile = 16; p.search = 8; p.value_threshold = 12000; p.pyramid_levels = 2;
    if (run(p, 2, false)) return 1;
    aof_params_px4flow(&p, 64, 64, 4, 30, 3000);
    if (run(p, 5, false)) return 1;
    // refusals
    aof_field_params fp;
    aof_field_params_default(&fp);
    aof_block b[25] = {};
    aof_flow f = {};
    aof_field o;
    REQUIRE(aof_field_host(&p, &fp, b, nullptr, &f, 1, &o) == 0 && o.accepted == 25 && o.flags == (AOF_FIELD_VALID | AOF_FIELD_REFIT));
    fp.min_blocks = 2;
    REQUIRE(aof_field_host(&p, &fp, b, nullptr, &f, 1, &o) == -EINVAL);
    fp.min_blocks = 8; fp.gate_px = NAN;
    REQUIRE(aof_field_host(&p, &fp, b, nullptr, &f, 1, &o) == -EINVAL);
    REQUIRE(aof_field_batch_device(nullptr, &fp, b, nullptr, &f, 1, &o, nullptr) == -EINVAL);
    std::printf("field rule and its __int128 restatement agree on %ld pairs\n", checked);
    return 0;
}
