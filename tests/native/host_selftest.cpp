// Sanitizer self-test of the product's HOST-ONLY logic (no HIP calls) and of the rules the host shares with the kernels,
// compiled for the host.  Built with -fsanitize=address,undefined and run by tests/test_host_asan.py, one check a run:
//
//   host_selftest list                  the names of the checks, one per line
//   host_selftest <check> [case-file]   runs that check (the table above main says which read a case file)
//
// A check that holds prints its "host selftest: ..." line and exits 0; a plan check first prints one line of fields per case
// of its file, which the test holds to the Python model of that plan.  A check that fails says which condition failed on
// stderr and exits 1.  An unknown name or a case file that cannot be read: a sentence on stderr, exit 2.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "aof.h"
#include "aof_bank_args.hpp"
#include "aof_bank_tables.hpp"
#include "aof_batch_plan.hpp"
#include "aof_coarse_plan.hpp"
#include "aof_cols8_plan.hpp"
#include "aof_engine_args.hpp"
#include "aof_exposure_step.hpp"
#include "aof_fastdiv.hpp"
#include "aof_host.hpp"
#include "aof_ingest_args.hpp"
#include "aof_lane8_plan.hpp"
#include "aof_mavlink.hpp"
#include "aof_small_plan.hpp"
#include "aof_tile16_plan.hpp"
#include "aof_warp_plan.hpp"
#include "aof_xcd_remap.hpp"
#include "bank_table.hpp"
#include "optical_flow_rad.hpp"

// The random inputs: a check that draws any seeds the generator itself, so what it draws depends on no other check.
static unsigned rng_state;
static void rnd_seed() { rng_state = 777u; }
static unsigned rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static uint64_t rnd64() { return ((uint64_t)rnd() << 48) ^ ((uint64_t)rnd() << 24) ^ rnd(); }
template <typename T, typename U> static T bits_as(U u) { T t; static_assert(sizeof(T) == sizeof(U), "same size"); std::memcpy(&t, &u, sizeof(T)); return t; }

// ---- reporting and case files ---------------------------------------------------------------------------------------------

static const char *check_name, *case_path;   // the running check; the case file it reads and the line of the current case
static int case_line;

// The report of a failed check: the sentence, the case it was found at where there is one, exit 1.  (Nothing a caller
// allocated is live when it reports: a leak report would replace the exit status.)
[[noreturn]] static void fail(const char *fmt, ...)
{
    std::fprintf(stderr, "%s: ", check_name);
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    if (case_path) std::fprintf(stderr, " (line %d of %s)", case_line, case_path);
    std::fputc('\n', stderr);
    std::exit(1);
}
#define HOLD(cond, ...) do { if (!(cond)) fail(__VA_ARGS__); } while (0)

// The n whitespace-separated integers of f's next line into v: signed 64-bit values, and unsigned ones (an address with
// its top bit set) by their bits.  False at end of file; a line that is not n integers fails the check.
static bool read_ints(std::FILE *f, int n, int64_t *v)
{
    char line[1024], *s = line, *end;
    if (!std::fgets(line, sizeof line, f)) return false;
    case_line++;
    int got = 0;
    for (;; got++, s = end) {
        const int64_t x = (int64_t)std::strtoull(s, &end, 10);   // (takes a sign too, and negates: the signed value's bits)
        if (end == s) break;
        if (got < n) v[got] = x;
    }
    HOLD(got == n && s[std::strspn(s, " \t\r\n")] == 0, "a line of %d integers%s where a case is %d integers", got, got == n ? " and more" : "", n);
    return true;
}

// fn(v) on the n integers of every line of the case file; returns the number of cases.
template <typename Fn> static int for_each_case(const char *path, int n, Fn fn)
{
    std::FILE *f = std::fopen(path, "r");
    if (!f) { std::fprintf(stderr, "host_selftest: cannot read the case file %s\n", path); std::exit(2); }
    case_path = path;
    int64_t v[32];   // (the longest case has 31)
    int cases = 0;
    while (read_ints(f, n, v)) { fn(v); cases++; }
    std::fclose(f);
    return cases;
}

static aof::Grid grid_of(const int64_t *g) { return {(int32_t)g[0], (int32_t)g[1], (int32_t)g[2], (int32_t)g[3], (int32_t)g[4], (int32_t)g[5]}; }
template <typename T> static const T *place_at(int64_t address) { return reinterpret_cast<const T *>((uintptr_t)address); }
static uint32_t somewhere[1];   // a place for what a plan only looks at for being there: directions, hints, vote memory, a fault word
static uint8_t *const somewhere8 = reinterpret_cast<uint8_t *>(somewhere);

// ---- the packer, the checksum step, the exposure rule ---------------------------------------------------------------------

struct Fields {
    uint64_t time_usec;
    int dt_us;
    float ang_x, ang_y;
    double gx, gy, gz;
    int quality;
    uint8_t seq, system_id, component_id;
};

// The kernels' packer and the facade's on one field set, each into heap blocks of exactly the documented sizes (the
// sanitizer sees a byte too many).  Returns the frame's length, or -1 where lengths or bytes differ.
static int packers_agree(const Fields &f)
{
    uint8_t *mine = (uint8_t *)std::malloc(AOF_SEQ_FRAME_BYTES), *theirs = (uint8_t *)std::malloc(AOF_SEQ_FRAME_BYTES);
    uint8_t *payload = (uint8_t *)std::malloc(aof::kMavlinkPayloadBytes);
    const int n = aof::pack_optical_flow_rad(mine, payload, f.time_usec, f.dt_us, f.ang_x, f.ang_y, f.gx, f.gy, f.gz, f.quality, f.seq,
                                             f.system_id, f.component_id);
    OpticalFlowRad m;
    fillOpticalFlowRad(m, 0, f.time_usec, f.dt_us, f.ang_x, f.ang_y, f.gx, f.gy, f.gz, f.quality);
    const size_t want = packOpticalFlowRad(m, f.seq, f.system_id, f.component_id, theirs);
    const bool same = n > 0 && (size_t)n == want && want <= AOF_SEQ_FRAME_BYTES && std::memcmp(mine, theirs, want) == 0;
    std::free(mine); std::free(theirs); std::free(payload);
    return same ? n : -1;
}

// packer: the kernels' packer == the facade's on a few thousand random field sets and the fixed cases; both frame lengths
// must occur (quality 0 truncates the payload to 40 bytes, anything else leaves 44).
static void check_packer(const char *)
{
    rnd_seed();
    int frames = 0, n52 = 0, n56 = 0;
    auto one = [&](const Fields &f) {
        const int n = packers_agree(f), want = f.quality & 0xFF ? 56 : 52;
        HOLD(n == want, "frame %d (quality %d): the kernels' packer and the facade's differ, or the frame is not %d bytes", frames, f.quality, want);
        if (n == 52) n52++;
        if (n == 56) n56++;
        frames++;
    };
    for (int it = 0; it < 4000; it++) {
        Fields f;
        f.time_usec = rnd64();
        f.dt_us = (int)rnd64();
        // any bit pattern but a NaN's (a NaN's payload need not survive being passed by value)
        f.ang_x = bits_as<float>((uint32_t)rnd64()); f.ang_y = bits_as<float>((uint32_t)rnd64());
        if (f.ang_x != f.ang_x) f.ang_x = 0.25f;
        if (f.ang_y != f.ang_y) f.ang_y = -0.0f;
        if (it & 1) {   // sums of a plausible size, or any finite or infinite double
            f.gx = 1e-3 * ((double)(rnd() % 20001) - 10000.0); f.gy = 1e-4 * ((double)(rnd() % 20001) - 10000.0); f.gz = 1e-5 * (double)rnd();
        } else {
            f.gx = bits_as<double>(rnd64()); f.gy = bits_as<double>(rnd64()); f.gz = bits_as<double>(rnd64());
            if (f.gx != f.gx) f.gx = 1.0;
            if (f.gy != f.gy) f.gy = -2.0;
            if (f.gz != f.gz) f.gz = 3.0;
        }
        f.quality = it % 7 == 0 ? 0 : (int)(rnd() % 256);
        f.seq = (uint8_t)rnd(); f.system_id = (uint8_t)rnd(); f.component_id = (uint8_t)rnd();
        one(f);
    }
    const Fields base = {5000000123ull, 66667, 0.01f, -0.02f, 0.1, 0.2, 0.3, 200, 7, 1, 100};
    const int ends[2] = {0, 255};
    for (int q : ends)
        for (int seq : ends) {
            Fields f = base;
            f.quality = q; f.seq = (uint8_t)seq;
            one(f);
            f.gx = -0.0; f.gy = 0.0; f.gz = -1e-60;              // all three convert to float -0.0 (gy through its sign switch)
            HOLD((float)f.gx == 0.0f && std::signbit((float)f.gx) && std::signbit((float)(-f.gy)) && std::signbit((float)f.gz), "a sum does not convert to float -0.0");
            one(f);
            f.time_usec = 0xFF00000000000000ull | (uint64_t)seq; // the top byte set
            one(f);
        }
    HOLD(n52 > 0 && n56 > 0, "a frame length never occurred: %d frames of 52 bytes, %d of 56", n52, n56);
    std::printf("host selftest: packer: %d frames equal to the facade's, lengths 52 and 56\n", frames);
}

// packer-range: the facade's packer alone on random messages: a frame's length within its bounds, its magic and length
// bytes; and the ends of the public exposure functions.
static void check_packer_range(const char *)
{
    rnd_seed();
    uint8_t wire[OPTICAL_FLOW_RAD_MAX_FRAME];
    for (int it = 0; it < 2000; it++) {
        OpticalFlowRad m;
        fillOpticalFlowRad(m, rnd(), rnd(), (int)rnd(), 0.001f * (float)(rnd() % 100), -0.002f * (float)(rnd() % 100),
                           0.1, 0.2, 0.3, (int)(rnd() % 256));
        size_t n = packOpticalFlowRad(m, (uint8_t)it, 1, 100, wire);
        HOLD(n >= 13 && n <= OPTICAL_FLOW_RAD_MAX_FRAME && wire[0] == 0xFD && wire[1] == n - 12,
             "message %d: a frame of %zu bytes, first byte 0x%02X, length byte %d", it, n, wire[0], wire[1]);
    }
    uint32_t hist[AOF_EXPOSURE_BINS] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10};
    HOLD(aof_exposure_msv(hist) > 0.0f, "the mean sample value of a filled histogram is not positive");
    HOLD(aof_exposure_bin(255) == -1 && aof_exposure_bin(-3) == -1, "aof_exposure_bin gives 255 or -3 a bin");
    std::printf("host selftest: packer range: 2000 frames within their bounds, the exposure functions' ends as documented\n");
}

// checksum: the two forms of the checksum step (aof_mavlink.hpp) on every (checksum, byte), and the facade's with them.
static void check_crc_steps(const char *)
{
    for (uint32_t crc = 0; crc < 65536u; crc++)
        for (uint32_t b = 0; b < 256u; b++) {
            const uint8_t byte = (uint8_t)b;
            const uint32_t narrow = aof::crc_accumulate(byte, (uint16_t)crc);
            HOLD(narrow == aof::rx_crc(b, crc) && narrow == mavlinkCrcAccumulate(&byte, 1, (uint16_t)crc),
                 "checksum 0x%04X, byte 0x%02X: crc_accumulate gives 0x%04X, rx_crc or the facade's step another", crc, b, narrow);
        }
    std::printf("host selftest: checksum: both steps and the facade's agree on 65536 x 256 inputs\n");
}

// exposure: the shared bin and mean sample value (aof_exposure_step.hpp) against the public functions.
static void check_exposure(const char *)
{
    rnd_seed();
    for (int v = 0; v < 256; v++) {
        const int shared = aof::exposure_bin((uint32_t)v), pub = aof_exposure_bin(v);
        HOLD(shared >= 0 && shared <= AOF_EXPOSURE_BINS && (shared == AOF_EXPOSURE_BINS ? -1 : shared) == pub, "sample value %d: shared bin %d, public bin %d", v, shared, pub);
    }
    HOLD(aof::exposure_bin(255u) == AOF_EXPOSURE_BINS && aof_exposure_bin(254) == 9 && aof_exposure_bin(0) == 0, "the bins of 255, 254 and 0 are not saturated, 9 and 0");
    int hists = 0;
    for (int it = 0; it < 2002; it++) {
        uint32_t hist[AOF_EXPOSURE_BINS];
        for (uint32_t &h : hist) h = it == 0 ? 0u : it == 1 ? 16384u : (it & 1) ? rnd() % 16385u : (uint32_t)rnd64();
        const float shared = aof::exposure_msv(hist), pub = aof_exposure_msv(hist);
        HOLD(std::memcmp(&shared, &pub, sizeof(float)) == 0, "histogram %d: the shared mean sample value is %.9g, the public one %.9g", it, shared, pub);
        HOLD(it != 0 || shared == 0.0f, "the empty histogram's mean sample value is %.9g", shared);
        HOLD(it != 1 || shared == 55.0f, "the level histogram's mean sample value is %.9g, not 55", shared);   // 1 + 2 + ... + 10, every term exact
        hists++;
    }
    std::printf("host selftest: exposure: 256 bins and %d mean sample values equal to the public functions\n", hists);
}

// ---- the plan checks: one line of fields per case of the file, in the order of the Python model's field names ---------------

// cols-plan: cols_plan_make (aof_cols8_plan.hpp), fields in the order of cols_plan_ref.PLAN_FIELDS.  A case: nx ny step_x w h
// pair_stride cur n_pairs done.
static void print_cols_plans(const char *path)
{
    const int cases = for_each_case(path, 9, [](const int64_t *v) {
        const int64_t nx = v[0], ny = v[1], step_x = v[2], w = v[3], h = v[4], stride = v[5], cur = v[6], n_pairs = v[7], done = v[8];
        aof::Grid g = {4, 4, (int32_t)step_x, 8, (int32_t)nx, (int32_t)ny};
        const aof::ColsLaunch l = aof::cols_plan_make(g, (int)w, (int)h, stride, (uintptr_t)cur, n_pairs, done);
        const aof::ColsSegments *cls[2] = {&l.plan.head, &l.plan.tail};
        std::printf("cols plan:");
        for (const aof::ColsSegments *s : cls) std::printf(" %d %d %u %u %u", s->len, s->segs, s->units_per_pair, s->div_units.mul, s->div_units.shift);
        std::printf(" %u %u %u %u %u %lld %lld %lld %lld %lld\n", l.plan.head_pairs, l.plan.head_units, l.plan.div_nx.mul, l.plan.div_nx.shift,
                    l.plan.aligned, (long long)l.per, (long long)l.pairs, (long long)l.tail_pairs, (long long)l.units, (long long)l.wgs);
    });
    std::printf("host selftest: cols plan: %d cases\n", cases);
}

// coarse-plan: coarse_plan_make (aof_coarse_plan.hpp), fields in the order of coarse_plan_ref.COARSE_FIELDS.  A case: w h
// pair_stride prev cur x0 y0 step_x step_y nx ny range tile search subpixel n_pairs cus.
static void print_coarse_plans(const char *path)
{
    const int cases = for_each_case(path, 17, [](const int64_t *v) {
        const int64_t w = v[0], h = v[1], stride = v[2], prev = v[3], cur = v[4], range = v[11], tile = v[12], search = v[13], subpixel = v[14],
                      n_pairs = v[15], cus = v[16];
        const aof::CoarsePlan p = aof::coarse_plan_make((int)w, (int)h, stride, (uintptr_t)prev, (uintptr_t)cur, grid_of(v + 5), (int)range, (int)tile,
                                                        (int)search, (int)subpixel, n_pairs, (int)cus);
        std::printf("coarse plan: %d %d %d %d %d %u %u %u %u %u %u %zu %d %d %lld\n", (int)p.verdict, p.rows_per_sweep, p.nkf, p.nk, p.nk_pad,
                    p.div_nb.mul, p.div_nb.shift, p.div_nx.mul, p.div_nx.shift, p.div_chunks.mul, p.div_chunks.shift, p.lds, p.stagger_groups,
                    p.stagger_ticks, (long long)p.wgs);
    });
    std::printf("host selftest: coarse plan: %d cases\n", cases);
}

// pyramid-plan: pyramid_plan_make (aof_coarse_plan.hpp), fields in the order of coarse_plan_ref.PYRAMID_FIELDS.  A case: w h
// pair_stride prev cur sequence n_pairs sums.
static void print_pyramid_plans(const char *path)
{
    const int cases = for_each_case(path, 8, [](const int64_t *v) {
        const int64_t w = v[0], h = v[1], stride = v[2], prev = v[3], cur = v[4], sequence = v[5], n_pairs = v[6], sums = v[7];
        const aof::PyramidPlan p = aof::pyramid_plan_make((int)w, (int)h, stride, (uintptr_t)prev, (uintptr_t)cur, (int)sequence, n_pairs, sums != 0);
        std::printf("pyramid plan: %d %d %d %lld %lld %lld\n", p.vec, p.rows_per_strip, p.nstrips, (long long)p.units, (long long)p.total,
                    (long long)p.zero_words);
    });
    std::printf("host selftest: pyramid plan: %d cases\n", cases);
}

// small-plan: small_plan_make and lane8_group_plan (aof_small_plan.hpp), two lines a case, fields in the order of
// small_plan_ref.PLAN_FIELDS and GROUP_FIELDS.  A case: w h levels, the level-0 and the level-1 grid (x0 y0 step_x step_y nx ny
// each), n_pairs pair_stride prev cur subpixel tile search, the histogram ranges of level 0 and 1, whether levels 0 and 1
// have a place for their half-pixel directions, and level 1's size as the caller states it.
static void print_small_plans(const char *path)
{
    const int cases = for_each_case(path, 28, [](const int64_t *v) {
        const int64_t w = v[0], h = v[1], levels = v[2], *g[2] = {v + 3, v + 9}, n_pairs = v[15], stride = v[16], prev = v[17], cur = v[18],
                      subpixel = v[19], tile = v[20], search = v[21], rng0 = v[22], rng1 = v[23], sub0 = v[24], sub1 = v[25], l1_w = v[26], l1_h = v[27];
        aof::SmallArgs a = {};
        aof::SearchArgs *lv[2] = {&a.l0, &a.l1};
        for (int l = 0; l < 2; l++) {
            aof::SearchArgs &s = *lv[l];
            s.prev = place_at<uint8_t>(prev);
            s.cur = place_at<uint8_t>(cur);
            s.pair_stride = stride;
            s.w = (int32_t)(l ? l1_w : w); s.h = (int32_t)(l ? l1_h : h);
            s.tile = (int32_t)tile; s.search = (int32_t)search;
            s.grid = grid_of(g[l]);
            s.subpixel = (int32_t)subpixel;
            s.subdirs = (l ? sub1 : sub0) ? somewhere8 : nullptr;
            s.n_pairs = n_pairs;
            s.hist_range = (int32_t)(l ? rng1 : rng0);
            s.level = l;
        }
        a.t0.range = (int32_t)rng0; a.t1.range = (int32_t)rng1;
        a.levels = (int32_t)levels;
        const aof::SmallPlan p = aof::small_plan_make(a);
        std::printf("small plan: %d %zu %zu %zu %zu %zu %d %d %d %d %d %d %d %d %d %d\n", (int)p.verdict, p.lds, p.f0[0], p.f0[1], p.f1[0], p.f1[1], p.attr,
                    p.trips_a[0], p.trips_a[1], p.trips_a[2], p.trips_b[0], p.trips_b[1], p.trips_c[0], p.trips_c[1], p.trips_d1[0], p.trips_d1[1]);
        const aof::Lane8GroupPlan gp = aof::lane8_group_plan(a.l0);
        std::printf("group plan: %d %lld %d %zu\n", gp.ppw, (long long)gp.wgs, gp.last_live, gp.lds);
    });
    std::printf("host selftest: small plan: %d cases\n", cases);
}

// lane8-plan: lane8_flat_plan (aof_lane8_plan.hpp), fields in the order of lane8_plan_ref.PLAN_FIELDS.  A case: nb n_pairs
// pair_stride w h prune fused rng votes_memory votes_fault votes_stride (votes_memory -1: no VoteMem at all) capacity slice
// tile search.
static void print_lane8_plans(const char *path)
{
    const int cases = for_each_case(path, 15, [](const int64_t *v) {
        const int64_t nb = v[0], n_pairs = v[1], stride = v[2], w = v[3], h = v[4], prune = v[5], fused = v[6], rng = v[7], mem = v[8], fault = v[9],
                      vstride = v[10], capacity = v[11], slice = v[12], tile = v[13], search = v[14];
        aof::SearchArgs a = {};
        a.pair_stride = stride;
        a.w = (int32_t)w; a.h = (int32_t)h;
        a.tile = (int32_t)tile; a.search = (int32_t)search;
        a.grid = {4, 4, 8, 8, (int32_t)nb, nb > 0 ? 1 : 0};
        a.n_pairs = n_pairs;
        a.hist_range = (int32_t)rng;
        a.prune = (int32_t)prune;
        aof::VoteMem vm = {mem > 0 ? somewhere : nullptr, (uint32_t)vstride, fault > 0 ? somewhere : nullptr, 0};
        const aof::Lane8FlatPlan p = aof::lane8_flat_plan(a, fused != 0, mem < 0 ? nullptr : &vm, capacity, slice);
        std::printf("lane8 plan: %d %d %d %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %d %d %lld %lld %lld %d %lld %d %d %u %u\n", p.supported, p.votes,
                    p.prune_large, (long long)p.chunks_all, (long long)p.per, (long long)p.slices, (long long)p.done, (long long)p.pairs,
                    (long long)p.frame_off, (long long)p.block_off, (long long)p.pred_off, (long long)p.sums_off, (long long)p.items, p.kind,
                    p.threads, (long long)p.wgs, (long long)p.finalisers, (long long)p.grid, p.last_live, (long long)p.chunks, p.spw, p.last_chunks,
                    p.stride, p.expected);
    });
    std::printf("host selftest: lane8 plan: %d cases\n", cases);
}

// A call as tests/batch_plan_ref.py writes it: w h tile search px4 num_blocks subpixel levels mean_subtract n_pairs pair_stride
// prev cur mode force_generic split cus k1_ready.  Parameters aof_params_check refuses get an empty grid and an empty layout
// (no context exists for them; the plan is then only the function's answer).  The workspace is a place, nothing reads it.
struct PlannedCall {
    aof::BatchConfig cfg;
    aof::BatchView view;
    int64_t n_pairs;
    bool valid, k1_ready;
};
enum { kCallInts = 18 };

static PlannedCall planned_call(const int64_t *v)
{
    const int64_t w = v[0], h = v[1], tile = v[2], search = v[3], px4 = v[4], num_blocks = v[5], subpixel = v[6], levels = v[7], mean_subtract = v[8],
                  n_pairs = v[9], stride = v[10], prev = v[11], cur = v[12], mode = v[13], force_generic = v[14], split = v[15], cus = v[16],
                  k1_ready = v[17];
    PlannedCall c = {};
    aof::BatchConfig &cfg = c.cfg;
    aof_params &p = cfg.params;
    aof_params_default(&p, (int)w, (int)h);
    p.tile = (int)tile; p.search = (int)search;
    p.grid_mode = px4 ? AOF_GRID_PX4FLOW : AOF_GRID_DENSE;
    p.num_blocks = (int)num_blocks;
    p.subpixel = (int)subpixel; p.pyramid_levels = (int)levels; p.mean_subtract = (int)mean_subtract;
    c.valid = aof_params_check(&p) == 0;
    aof::Grid *g[2] = {&cfg.g0, &cfg.g1};
    for (int l = 0; l < (int)levels && l < 2; l++)
        if (aof::grid_for_level(p, l, g[l])) *g[l] = {};
    cfg.cus = (int)cus; cfg.search_mode = (int)mode; cfg.force_generic = force_generic != 0; cfg.split_coarse = split != 0;
    aof_ws_layout L = {};
    HOLD(!c.valid || aof_workspace_layout(&p, (int64_t)n_pairs, &L) == 0, "valid parameters of a call have no workspace layout");
    c.n_pairs = n_pairs;
    c.k1_ready = k1_ready != 0;
    c.view = aof::batch_view(cfg, L, place_at<uint8_t>(prev), place_at<uint8_t>(cur), (int64_t)stride, nullptr, nullptr,
                             reinterpret_cast<aof_flow *>((uintptr_t)0x7E0000000000ull), reinterpret_cast<void *>((uintptr_t)0x7D0000000000ull));
    return c;
}

// batch-plan: plan_batch (aof_batch_plan.hpp) on a call per line, fields in the order of batch_plan_ref.PLAN_FIELDS.  The
// summary counts how often each SearchKind was planned (level 0, and level 1 where K1 is followed by a search) and each
// CoarseKind.
static void print_batch_plans(const char *path)
{
    int kinds[4] = {}, coarse[3] = {};
    const int cases = for_each_case(path, kCallInts, [&](const int64_t *v) {
        const PlannedCall c = planned_call(v);
        const aof::BatchPlan P = aof::plan_batch(c.cfg, c.view, c.n_pairs, c.k1_ready);
        const bool level1 = !P.small && P.coarse == aof::COARSE_K1 && c.cfg.params.pyramid_levels == 2;
        std::printf("batch plan: %d %d %d %d %d %d %d %d %d %d %d %d\n", c.valid ? 1 : 0, P.small ? 1 : 0, P.small_class ? 1 : 0, (int)P.coarse,
                    P.k1_pass ? 1 : 0, P.sequence ? 1 : 0, (int)P.level[0].kind, P.level[0].refine ? 1 : 0, P.level[0].a.prune,
                    level1 ? (int)P.level[1].kind : 0, level1 && P.level[1].refine ? 1 : 0, level1 ? P.level[1].a.prune : 0);
        kinds[P.level[0].kind]++;
        if (level1) kinds[P.level[1].kind]++;
        coarse[P.coarse]++;
    });
    std::printf("host selftest: batch plan: %d cases, kinds %d %d %d %d, coarse %d %d %d\n", cases, kinds[0], kinds[1], kinds[2], kinds[3],
                coarse[0], coarse[1], coarse[2]);
}

// tile16-plan: tile16_plan (aof_tile16_plan.hpp), fields in the order of batch_plan_ref.T16_FIELDS, and the three questions the
// plan answers asked one by one; the summary counts the verdicts.  A case: w h pair_stride prev cur tile search grid[6] subpixel
// subdirs prune hints n_pairs forced.
static void print_tile16_plans(const char *path)
{
    int verdicts[9] = {};
    const int cases = for_each_case(path, 19, [&](const int64_t *v) {
        const int64_t w = v[0], h = v[1], stride = v[2], prev = v[3], cur = v[4], tile = v[5], search = v[6], subpixel = v[13], subdirs = v[14],
                      prune = v[15], hints = v[16], n_pairs = v[17], forced = v[18];
        aof::SearchArgs a = {};
        a.prev = place_at<uint8_t>(prev);
        a.cur = place_at<uint8_t>(cur);
        a.pair_stride = stride;
        a.w = (int32_t)w; a.h = (int32_t)h;
        a.tile = (int32_t)tile; a.search = (int32_t)search;
        a.grid = grid_of(v + 7);
        a.subpixel = (int32_t)subpixel;
        a.subdirs = subdirs ? somewhere8 : nullptr;
        a.prune = (int32_t)prune;
        a.hints = hints ? somewhere : nullptr;
        a.n_pairs = n_pairs;
        const aof::Tile16Plan p = aof::tile16_plan(a, (int)forced);
        HOLD((p.verdict == aof::TILE16_OK) == aof::tile16_supported(a) && (p.refines != 0) == aof::tile16_refines(a) && p.lds == aof::tile16_lds(a),
             "the plan (verdict %d, refines %d, lds %zu) is not what tile16_supported, tile16_refines and tile16_lds answer", p.verdict, p.refines, p.lds);
        std::printf("tile16 plan: %d %d %zu %d %d %d %lld %d %d %d %lld %d %d %d %d\n", p.verdict, p.refines, p.lds, p.attr, p.prune, p.refine,
                    (long long)p.total, p.overflow, p.front, p.refused, (long long)p.front_wgs, p.stx, p.sty, p.sx, p.sy);
        if (p.verdict >= 0 && p.verdict < 9) verdicts[p.verdict]++;
    });
    std::printf("host selftest: tile16 plan: %d cases, verdicts %d %d %d %d %d %d %d %d %d\n", cases, verdicts[0], verdicts[1], verdicts[2],
                verdicts[3], verdicts[4], verdicts[5], verdicts[6], verdicts[7], verdicts[8]);
}

// warp-plan: warp_plan_make (aof_warp_plan.hpp), fields in the order of warp_plan_ref.WARP_FIELDS; the summary counts the
// verdicts.  A case: w h n_frames cropped cropped_stride hist.
static void print_warp_plans(const char *path)
{
    int verdicts[3] = {};
    const int cases = for_each_case(path, 6, [&](const int64_t *v) {
        const int64_t w = v[0], h = v[1], n_frames = v[2], cropped = v[3], stride = v[4], hist = v[5];
        const aof::WarpPlan p = aof::warp_plan_make((int32_t)w, (int32_t)h, n_frames, (uintptr_t)cropped, stride, hist != 0);
        std::printf("warp plan: %d %d %d %d %d %d %d %d %d %lld %lld %d %zu %d %d %lld %lld %d %d %lld\n", (int)p.verdict, p.nx, p.ny, p.strip_rows, p.nstrips,
                    p.rows[0], p.rows[1], p.node_rows[0], p.node_rows[1], (long long)p.node_bytes[0], (long long)p.node_bytes[1], p.vec, p.lds, p.attr,
                    p.zero_hist, (long long)p.items[0], (long long)p.items[1], p.trips[0], p.trips[1], (long long)p.wgs);
        if (p.verdict >= 0 && p.verdict < 3) verdicts[p.verdict]++;
    });
    std::printf("host selftest: warp plan: %d cases, verdicts %d %d %d\n", cases, verdicts[0], verdicts[1], verdicts[2]);
}

// The report a pruned launch leaves in the context's pinned words: the first `arrived` of `expected` carry the launch's
// tag with `paying` of `seen` chunks each, the rest a stale tag.
static uint32_t report_words[aof::kPruneSlots];

static aof::AdaptiveSearch adaptive_state(int belief, int since_probe, uint32_t launch_no, uint32_t expected, uint32_t arrived, uint32_t paying,
                                          uint32_t seen)
{
    aof::AdaptiveSearch st = {};
    st.slots = report_words;
    st.launch_no = launch_no;
    st.expected = expected;
    st.belief = belief;
    st.since_probe = since_probe;
    st.stats.belief = belief;
    const uint32_t tag = launch_no & 0xFFFFu;
    for (uint32_t i = 0; i < (uint32_t)aof::kPruneSlots; i++)
        report_words[i] = i < arrived ? (tag << 16 | paying << 8 | seen) : ((tag ^ 1u) << 16 | 0xFFFFu);
    return st;
}

// choose-lane8: choose_lane8 (aof_batch_plan.hpp) on a row per line: a call (its level-0 search must be a flat 8x8 launch),
// then belief since_probe launch_no expected arrived paying seen capture captured separate votes_memory votes_fault
// votes_stride.  One line per row: the launch and the state after it, in the order of batch_plan_ref.CHOOSE_FIELDS.
static void print_choose_lane8(const char *path)
{
    const int rows = for_each_case(path, kCallInts + 13, [](const int64_t *v) {
        const PlannedCall c = planned_call(v);
        const int64_t *r = v + kCallInts, belief = r[0], since = r[1], launch_no = r[2], expected = r[3], arrived = r[4], paying = r[5], seen = r[6],
                      capture = r[7], captured = r[8], separate = r[9], mem = r[10], fault = r[11], vstride = r[12];
        const aof::BatchPlan P = aof::plan_batch(c.cfg, c.view, c.n_pairs, c.k1_ready);
        HOLD(c.valid && !P.small && P.level[0].kind == aof::SK_LANE8, "the row's call is not a flat 8x8 launch at level 0");
        aof::AdaptiveSearch st = adaptive_state((int)belief, (int)since, (uint32_t)launch_no, (uint32_t)expected, (uint32_t)arrived, (uint32_t)paying,
                                                (uint32_t)seen);
        const aof::VoteMem vm = {mem ? somewhere : nullptr, (uint32_t)vstride, fault ? somewhere : nullptr, 0};
        const aof::Lane8Launch l = aof::choose_lane8(c.cfg, st, P.level[0].a, (aof::Capture)capture, vm, 2048 /* kVotePairs, aof_ctx.hpp */, separate != 0, captured != 0);
        std::printf("choose lane8: %d %d %d %d %u %d %d %u %llu %llu %llu %d %d\n", l.prune, l.cols ? 1 : 0, l.fused ? 1 : 0, l.rep.slots ? 1 : 0,
                    l.rep.launch_no, st.belief, st.since_probe, st.launch_no, (unsigned long long)st.stats.pruned_launches,
                    (unsigned long long)st.stats.exhaustive_launches, (unsigned long long)st.stats.reports_read, st.stats.belief, st.stats.paying_pct);
    });
    std::printf("host selftest: choose lane8: %d rows printed\n", rows);
}

// choose-lane8-written: choose_lane8, row by row against the values written here: 1 024 VGA pairs on the dense grid (4 661
// blocks: a launch large enough to prune, the column walk's grid), 19 vote bins, vote records for 2 048 pairs, the last
// reporting launch number 7.
static void check_choose_lane8(const char *)
{
    using namespace aof;
    enum { EX = AOF_SEARCH_EXHAUSTIVE, PR = AOF_SEARCH_PRUNED, AD = AOF_SEARCH_ADAPTIVE };
    const struct {
        int mode, belief, since; uint32_t launch_no, expected, arrived, paying; Capture cap; bool captured, separate;   // (every word: `paying` of 100 chunks)
        int prune; bool cols, fused; int belief_after, since_after; uint32_t launch_after, tag; uint64_t pruned, exhaustive, read;
    } rows[] = {
        // the fixed modes read and change nothing
        {EX, -1, 14, 7, 0, 0, 0, CAPTURE_NONE, false, false, 0, false, true, -1, 14, 7, 0, 0, 0, 0},
        {PR, -1, 14, 7, 0, 0, 0, CAPTURE_NONE, false, false, 1, true, true, -1, 14, 7, 0, 0, 0, 0},
        // nothing known: the first chunk of every wave judges; pruning pays: every wave prunes at once
        {AD, -1, 14, 7, 0, 0, 0, CAPTURE_NONE, false, false, 2, true, true, -1, 14, 8, 8, 1, 0, 0},
        {AD, 1, 14, 7, 0, 0, 0, CAPTURE_NONE, false, false, 1, true, true, 1, 14, 8, 8, 1, 0, 0},
        // it does not pay: the exhaustive kernel, and the pruned one with the 16th launch
        {AD, 0, 14, 7, 0, 0, 0, CAPTURE_NONE, false, false, 0, false, true, 0, 15, 7, 0, 0, 1, 0},
        {AD, 0, 15, 7, 0, 0, 0, CAPTURE_NONE, false, false, 2, true, true, 0, 0, 8, 8, 1, 0, 0},
        // a report counts once a quarter of its words have arrived, and says "pays" from 40 % on
        {AD, 0, 14, 7, 8, 1, 100, CAPTURE_NONE, false, false, 0, false, true, 0, 15, 7, 0, 0, 1, 0},
        {AD, 0, 14, 7, 8, 2, 39, CAPTURE_NONE, false, false, 0, false, true, 0, 15, 7, 0, 0, 1, 1},
        {AD, 0, 14, 7, 8, 2, 40, CAPTURE_NONE, false, false, 1, true, true, 1, 14, 8, 8, 1, 0, 1},
        {AD, 1, 14, 7, 8, 8, 39, CAPTURE_NONE, false, false, 0, false, true, 0, 15, 7, 0, 0, 1, 1},
        {AD, -1, 15, 7, 8, 8, 40, CAPTURE_NONE, false, false, 1, true, true, 1, 15, 8, 8, 1, 0, 1},
        // the reduction in the launch: inside a capture always, eagerly until a graph holds one, never where the capture
        // state is unknown or the caller keeps K3
        {AD, 1, 14, 7, 0, 0, 0, CAPTURE_ACTIVE, true, false, 1, true, true, 1, 14, 8, 8, 1, 0, 0},
        {AD, 1, 14, 7, 0, 0, 0, CAPTURE_NONE, true, false, 1, true, false, 1, 14, 8, 8, 1, 0, 0},
        {AD, 1, 14, 7, 0, 0, 0, CAPTURE_UNKNOWN, false, false, 1, true, false, 1, 14, 8, 8, 1, 0, 0},
        {AD, 1, 14, 7, 0, 0, 0, CAPTURE_ACTIVE, false, true, 1, true, false, 1, 14, 8, 8, 1, 0, 0},
        {EX, -1, 14, 7, 0, 0, 0, CAPTURE_NONE, false, true, 0, false, false, -1, 14, 7, 0, 0, 0, 0},
        // the launch counter skips tag 0
        {AD, 1, 14, 0xFFFFu, 0, 0, 0, CAPTURE_NONE, false, false, 1, true, true, 1, 14, 0x10001u, 1, 1, 0, 0},
    };
    aof_params p;
    aof_params_default(&p, 640, 480);
    BatchConfig cfg = {};
    cfg.params = p;
    HOLD(grid_for_level(p, 0, &cfg.g0) == 0 && cfg.g0.blocks() == 4661, "the dense VGA grid does not have 4661 blocks");
    cfg.cus = 256;
    const VoteMem vm = {somewhere, 128, somewhere, 0};
    int n = 0;
    for (const auto &r : rows) {
        cfg.search_mode = r.mode;
        const SearchArgs a = search_args(cfg, 0, nullptr, nullptr, 640 * 480, nullptr, nullptr, nullptr, nullptr, 1024);
        AdaptiveSearch st = adaptive_state(r.belief, r.since, r.launch_no, r.expected, r.arrived, r.paying, 100);
        const Lane8Launch l = choose_lane8(cfg, st, a, r.cap, vm, 2048, r.separate, r.captured);
        HOLD(l.prune == r.prune && l.cols == r.cols && l.fused == r.fused && (l.rep.slots != nullptr) == (r.tag != 0) && (!r.tag || l.rep.launch_no == r.tag),
             "row %d: the launch (prune %d, cols %d, fused %d) or its report tag is not the one written", n, l.prune, (int)l.cols, (int)l.fused);
        HOLD(st.belief == r.belief_after && st.since_probe == r.since_after && st.launch_no == r.launch_after,
             "row %d: the state after the launch (belief %d, since_probe %d, launch_no %u) is not the one written", n, st.belief, st.since_probe, st.launch_no);
        HOLD(st.stats.pruned_launches == r.pruned && st.stats.exhaustive_launches == r.exhaustive && st.stats.reports_read == r.read,
             "row %d: the counters after the launch are not the ones written", n);
        n++;
    }
    std::printf("host selftest: choose lane8: %d rows equal to the values written\n", n);
}

// xcd-permutation: xcd_remap (aof_xcd_remap.hpp, the text the kernels run) is a permutation of [0, total) for every total up
// to 4096: every logical id hit once.
static void check_xcd_remap(const char *)
{
    static uint8_t hit[4096];
    for (uint32_t total = 1; total <= 4096u; total++) {
        std::memset(hit, 0, total);
        for (uint32_t b = 0; b < total; b++) {
            const uint32_t wg = aof::xcd_remap(b, total);
            HOLD(wg < total && !hit[wg]++, "total %u: hardware id %u maps to %u, beyond the total or taken", total, b, wg);
            HOLD(b < 8 || wg == aof::xcd_remap(b - 8, total) + 1, "total %u: hardware ids %u and %u do not map to neighbours", total, b - 8, b);   // an XCD's logical ids are contiguous
        }
    }
    std::printf("host selftest: xcd_remap: a permutation for every total up to 4096\n");
}

// xcd-probes: xcd_remap printed value by value for the test to hold to the model's.  A probe: total b.
static void print_xcd_probes(const char *path)
{
    const int probes = for_each_case(path, 2, [](const int64_t *v) { std::printf("xcd remap: %u\n", aof::xcd_remap((uint32_t)v[1], (uint32_t)v[0])); });
    std::printf("host selftest: xcd_remap: %d probes\n", probes);
}

// fastdiv: fastdiv_make against the division it replaces, with the kernels' fast_div (aof_device.hpp) restated -- the high
// half of the product, the sum and the shift in 32 bits.  Divisors: every d up to 4096 (grid widths, blocks per pair) and
// every multiple of 64 up to 2^20 (units per pair); numerators: all below 2^16, and around 65 multiples of d spread up to the
// top of the 31 bits the launchers keep to.
static uint32_t fast_div_host(uint32_t n, aof::FastDiv d) { return ((uint32_t)(((uint64_t)n * d.mul) >> 32) + n) >> d.shift; }

static void check_fastdiv(const char *)
{
    int extra = 0, divisors = 0;   // extra: the numerators per divisor beyond the first 2^16
    for (uint32_t i = 1; i <= 4096u + (1u << 20) / 64u; i++) {
        const uint32_t d = i <= 4096u ? i : (i - 4096u) * 64u;
        if (i > 4096u && d <= 4096u) continue;   // (already seen)
        const aof::FastDiv fd = aof::fastdiv_make(d);
        HOLD(fd.shift <= 31u, "divisor %u: a shift of %u", d, fd.shift);
        uint32_t q = 0, r = 0;
        for (uint32_t n = 0; n < 65536u; n++) {
            HOLD(fast_div_host(n, fd) == q, "%u / %u: fast_div gives %u", n, d, fast_div_host(n, fd));
            if (++r == d) { r = 0; q++; }
        }
        const uint32_t top = 0x7FFFFFFFu / d;
        int count = 0;
        for (uint32_t step = 0; step <= 64u; step++) {
            const uint32_t k = (uint32_t)((uint64_t)top * step / 64u);
            const uint64_t around[3] = {(uint64_t)k * d - 1u, (uint64_t)k * d, (uint64_t)k * d + 1u};
            for (uint64_t n : around) {
                if (n > 0x7FFFFFFFull) continue;   // (k = 0: -1 wraps; the top multiple + 1 may pass 2^31)
                HOLD(fast_div_host((uint32_t)n, fd) == (uint32_t)(n / d), "%u / %u: fast_div gives %u", (uint32_t)n, d, fast_div_host((uint32_t)n, fd));
                count++;
            }
        }
        const uint32_t ends[2] = {0x7FFEFFFFu, 0x7FFFFFFFu};
        for (uint32_t n : ends) {
            HOLD(fast_div_host(n, fd) == n / d, "%u / %u: fast_div gives %u", n, d, fast_div_host(n, fd));
            count++;
        }
        HOLD(count >= 190, "divisor %u: only %d numerators around its multiples", d, count);
        extra = count > extra ? count : extra;
        divisors++;
    }
    std::printf("host selftest: fast_div: %d divisors, all numerators below 65536 and up to %d around multiples up to 2^31 equal to n / d\n",
                divisors, extra);
}

// bank-tables: the stream bank's bound per-stream tables (aof_bank_tables.hpp): what a binding call accepts and leaves
// behind, and which tables a push or an IMU call uses or why it is refused, each case against the value written here.  The
// arrays are places in `arena`; nothing reads them.
alignas(16) static uint8_t arena[96];

static bool same_text(const char *got, const char *want)
{
    return (!got && !want) || (got && want && std::strcmp(got, want) == 0);
}

static void check_bank_tables(const char *)
{
    using namespace aof;
    const void *const A = arena + 16, *const ODD = arena + 40, *const OLD = arena + 64;   // 16-byte aligned, 8 off, the binding before
    int cases = 0;
    // ---- binding: every case starts from all four bound for 3 streams, camera_bytes 1000 ----
    const struct {
        BankTable which; const void *array; int32_t n; uint64_t camera_bytes;
        const char *refusal;                                  // nullptr: accepted, and the table then holds
        const void *array_after; int32_t n_after; uint64_t camera_bytes_after;
    } binds[] = {
        {kBankStreams, nullptr, 5, 0, nullptr, nullptr, 0, 1000},
        {kBankStreams, A, 0, 0, "bank streams: an array needs n_streams >= 1", OLD, 3, 1000},
        {kBankStreams, A, -1, 0, "bank streams: an array needs n_streams >= 1", OLD, 3, 1000},
        {kBankStreams, ODD, 4, 0, "bank streams: the array must be 16-byte aligned", OLD, 3, 1000},
        {kBankStreams, A, 4, 0, nullptr, A, 4, 1000},
        {kBankSensors, nullptr, 5, 77, nullptr, nullptr, 0, 0},
        {kBankSensors, A, 0, 77, "bank sensors: an array needs n_streams >= 1", OLD, 3, 1000},
        {kBankSensors, A, -1, 77, "bank sensors: an array needs n_streams >= 1", OLD, 3, 1000},
        {kBankSensors, ODD, 4, 77, "bank sensors: the array must be 16-byte aligned", OLD, 3, 1000},
        {kBankSensors, A, 4, 0, "bank sensors: an array needs camera_bytes > 0", OLD, 3, 1000},
        {kBankSensors, ODD, 0, 0, "bank sensors: an array needs n_streams >= 1", OLD, 3, 1000},   // (the first of three reasons)
        {kBankSensors, A, 4, 77, nullptr, A, 4, 77},
        {kBankFormats, nullptr, 5, 0, nullptr, nullptr, 0, 1000},
        {kBankFormats, A, 0, 0, "bank pixel formats: an array needs n_streams >= 1", OLD, 3, 1000},
        {kBankFormats, A, -1, 0, "bank pixel formats: an array needs n_streams >= 1", OLD, 3, 1000},
        {kBankFormats, ODD, 4, 0, nullptr, ODD, 4, 1000},
        {kBankFormats, (const uint8_t *)ODD + 1, 2, 0, nullptr, (const uint8_t *)ODD + 1, 2, 1000},
        {kBankBins, nullptr, 5, 0, nullptr, nullptr, 0, 1000},
        {kBankBins, A, 0, 0, "bank binning: an array needs n_streams >= 1", OLD, 3, 1000},
        {kBankBins, A, -1, 0, "bank binning: an array needs n_streams >= 1", OLD, 3, 1000},
        {kBankBins, ODD, 4, 0, nullptr, ODD, 4, 1000},
        {kBankBins, (const uint8_t *)ODD + 3, 1, 0, nullptr, (const uint8_t *)ODD + 3, 1, 1000},
    };
    for (const auto &c : binds) {
        BankTables before = {};
        for (int t = 0; t < kBankTableCount; t++) before.table[t] = {OLD, 3};
        before.camera_bytes = 1000;
        BankTables b = before;
        const char *got = bank_tables_bind(&b, c.which, c.array, c.n, c.camera_bytes);
        HOLD(same_text(got, c.refusal), "binding case %d: answered '%s', written '%s'", cases, got ? got : "(accepted)", c.refusal ? c.refusal : "(accepted)");
        HOLD(!c.refusal || b == before, "binding case %d: a refused binding changed the tables", cases);
        BankTables want = before;
        want.table[c.which] = {c.array_after, c.n_after};
        want.camera_bytes = c.camera_bytes_after;
        HOLD(b == want, "binding case %d: the tables after the call are not the ones written", cases);
        cases++;
    }
    // ---- resolving, for a call of 3 streams: {streams, sensors, formats, bins} bound for that many streams (0: not bound) ----
    const int64_t kBig = INT64_MAX / AOF_BANK_BURST_MAX + 1;
    enum { kImu = 2 };
    enum { S = 1, N = 2, F = 4, B = 8 };   // the arrays the call uses
    const struct {
        int32_t bound[kBankTableCount]; int form; int64_t round_stride;   // form: 0 pre-cropped frames, 1 sensor frames, kImu
        const char *refusal; int uses; uint64_t camera_bytes;
    } calls[] = {
        {{0, 0, 0, 0}, 0, 0, nullptr, 0, 0},
        {{0, 0, 0, 0}, 1, 0, nullptr, 0, 0},
        {{3, 0, 0, 0}, 0, 0, nullptr, S, 0},
        {{3, 0, 0, 0}, 1, 0, nullptr, S, 0},
        {{0, 3, 0, 0}, 1, 0, nullptr, N, 1000},
        {{0, 3, 3, 0}, 1, 0, nullptr, N | F, 1000},
        {{0, 3, 0, 3}, 1, 0, nullptr, N | B, 1000},
        {{3, 3, 3, 3}, 1, 640, nullptr, S | N | F | B, 1000},
        {{4, 0, 0, 0}, 0, 0, "bank: n_streams differs from the array bound with aof_set_bank_streams", 0, 0},
        {{4, 0, 0, 0}, 1, 0, "bank: n_streams differs from the array bound with aof_set_bank_streams", 0, 0},
        {{0, 4, 0, 0}, 1, 0, "bank: n_streams differs from the array bound with aof_set_bank_sensors", 0, 0},
        {{0, 3, 4, 0}, 1, 0, "bank: n_streams differs from the array bound with aof_set_bank_pixel_formats", 0, 0},
        {{0, 3, 0, 4}, 1, 0, "bank: n_streams differs from the array bound with aof_set_bank_binning", 0, 0},
        {{4, 4, 0, 0}, 1, 0, "bank: n_streams differs from the array bound with aof_set_bank_streams", 0, 0},
        {{0, 0, 3, 0}, 1, 0, "bank: pixel formats are bound (aof_set_bank_pixel_formats) without sensor records", 0, 0},
        {{0, 0, 4, 0}, 1, 0, "bank: pixel formats are bound (aof_set_bank_pixel_formats) without sensor records", 0, 0},
        {{0, 0, 0, 3}, 1, 0, "bank: a binning is bound (aof_set_bank_binning) without sensor records", 0, 0},
        {{0, 0, 3, 3}, 1, 0, "bank: pixel formats are bound (aof_set_bank_pixel_formats) without sensor records", 0, 0},
        {{0, 3, 4, 4}, 1, 0, "bank: n_streams differs from the array bound with aof_set_bank_pixel_formats", 0, 0},
        {{0, 3, 0, 0}, 1, kBig, "bank burst: round_stride too large for sensor records", 0, 0},
        {{0, 3, 0, 0}, 1, kBig - 1, nullptr, N, 1000},
        {{3, 0, 0, 0}, 1, kBig, nullptr, S, 0},
        {{0, 4, 0, 0}, 1, kBig, "bank: n_streams differs from the array bound with aof_set_bank_sensors", 0, 0},
        {{0, 3, 4, 0}, 1, kBig, "bank burst: round_stride too large for sensor records", 0, 0},
        {{0, 4, 4, 4}, 0, 0, nullptr, 0, 0},
        {{3, 4, 4, 4}, 0, kBig, nullptr, S, 0},
        {{0, 0, 3, 3}, 0, 0, nullptr, 0, 0},
        {{4, 0, 0, 0}, kImu, 0, "imu: n_streams differs from the array bound with aof_set_bank_streams", 0, 0},
        {{3, 4, 4, 4}, kImu, 0, nullptr, S, 0},
        {{0, 0, 3, 3}, kImu, 0, nullptr, 0, 0},
    };
    for (const auto &c : calls) {
        BankTables b = {};
        for (int t = 0; t < kBankTableCount; t++)
            if (c.bound[t]) b.table[t] = {arena + 16 * (t + 1), c.bound[t]};
        b.camera_bytes = c.bound[kBankSensors] ? 1000 : 0;
        const BankTablesUsed untouched = {(const aof_bank_stream *)arena, (const aof_bank_sensor *)arena, 5, arena, arena};
        BankTablesUsed u = untouched;
        const char *got;
        if (c.form == kImu) got = bank_tables_for_imu(b, 3, &u.streams);
        else got = bank_tables_for_push(b, 3, c.form == 1, c.round_stride, &u);
        HOLD(same_text(got, c.refusal), "case %d (bindings and calls counted together): answered '%s', written '%s'", cases, got ? got : "(accepted)", c.refusal ? c.refusal : "(accepted)");
        if (c.refusal) {   // a refused call hands nothing out
            HOLD(u.streams == untouched.streams && u.sensors == untouched.sensors && u.formats == untouched.formats && u.bins == untouched.bins, "case %d: refused, yet a table handed out", cases);
        } else {
            HOLD(u.streams == (c.uses & S ? (const void *)(arena + 16) : nullptr), "case %d: the stream table handed out is not the one written", cases);
            if (c.form != kImu) {
                HOLD(u.sensors == (c.uses & N ? (const void *)(arena + 32) : nullptr) && u.camera_bytes == c.camera_bytes, "case %d: not the sensor table or camera_bytes written", cases);
                HOLD(u.formats == (c.uses & F ? arena + 48 : nullptr) && u.bins == (c.uses & B ? arena + 64 : nullptr), "case %d: not the format or binning table written", cases);
            }
        }
        cases++;
    }
    // ---- the kernels' sensor arguments of a round: every value in its own field ----
    const BankTablesUsed u = {(const aof_bank_stream *)(arena + 16), (const aof_bank_sensor *)(arena + 32), 1000, arena + 48, arena + 64};
    const BankSensors bs = bank_sensors_of_round(u, 640);
    HOLD((const void *)bs.recs == arena + 32 && bs.camera_bytes == 1000 && bs.camera_base == 640 && bs.formats == arena + 48 && bs.bins == arena + 64,
         "bank_sensors_of_round puts a value into another field");
    const IngestSensors is = ingest_sensors_of_round(u, 640, arena + 80), plain = ingest_sensors_of_round(u, 0);
    HOLD((const void *)is.recs == arena + 32 && is.base == 640 && is.camera_bytes == 1000 && is.ok == arena + 80 && is.formats == arena + 48 &&
             is.bins == arena + 64 && plain.ok == nullptr && plain.base == 0,
         "ingest_sensors_of_round puts a value into another field");
    std::printf("host selftest: bank tables: %d cases\n", cases + 2);
}

// facade-table: the flags of one per-stream table of OpticalFlowBank (facade/src/bank_table.hpp) over a run of ticks, with
// counters in place of the copy and the binding call: after every step the numbers written here.
struct TableSim {
    BankTableFlags f = {};
    int uploads = 0, binds = 0;
    int upload_rc = 0, bind_rc = 0;   // what the copy and the binding call answer
    // one tick: the table in front of the push; `fails`: the push fails behind it, before the tag is seen
    int tick(bool fails = false)
    {
        const int rc = f.sync([&]() { uploads++; return upload_rc; }, [&]() { binds++; return bind_rc; });
        if (rc) return rc;
        if (fails) return -1;
        f.tagSeen();
        return 0;
    }
    bool at(int want_uploads, int want_binds, bool want_dirty) const
    {
        return uploads == want_uploads && binds == want_binds && f.dirty == want_dirty && !(f.copying && !f.dirty);
    }
};

static void check_facade_table(const char *)
{
    int steps = 0;
#define STEP(cond) do { HOLD(cond, "step %d does not hold: %s", steps, #cond); steps++; } while (0)
    {   // no setter, three ticks: nothing is copied or bound
        TableSim t;
        for (int k = 0; k < 3; k++) STEP(t.tick() == 0 && t.at(0, 0, false) && !t.f.used && !t.f.bound);
    }
    {   // a setter before tick 0: one copy and the binding at tick 0, nothing at tick 1; a setter between ticks 1 and 2:
        // one more copy, no second binding
        TableSim t;
        t.f.touch();
        STEP(t.tick() == 0 && t.at(1, 1, false) && t.f.bound);
        STEP(t.tick() == 0 && t.at(1, 1, false));
        t.f.touch();
        STEP(t.at(1, 1, true));
        STEP(t.tick() == 0 && t.at(2, 1, false));
        STEP(t.tick() == 0 && t.at(2, 1, false));
    }
    {   // the tick fails behind the enqueued copy, before its tag: still dirty, the next tick copies again
        TableSim t;
        t.f.touch();
        STEP(t.tick(true) == -1 && t.at(1, 1, true) && t.f.copying && t.f.bound);
        STEP(t.tick() == 0 && t.at(2, 1, false) && !t.f.copying);
        STEP(t.tick() == 0 && t.at(2, 1, false));
    }
    {   // dirty without used (setTimestampOffset()): nothing until a setter marks the table used, then one copy carries both
        TableSim t;
        t.f.touchUnused();
        STEP(t.tick() == 0 && t.at(0, 0, true) && !t.f.used);
        STEP(t.tick() == 0 && t.at(0, 0, true));
        t.f.touch();
        STEP(t.tick() == 0 && t.at(1, 1, false));
        t.f.touchUnused();   // and once the table is used, such a change is copied at the next tick
        STEP(t.tick() == 0 && t.at(2, 1, false));
    }
    {   // needed beside another table (setStreamPixelFormat(), setStreamBinning()): copied and bound once, not copied again
        TableSim t;
        t.f.rideAlong();
        STEP(t.f.used && t.f.dirty);
        STEP(t.tick() == 0 && t.at(1, 1, false));
        t.f.rideAlong();
        STEP(t.tick() == 0 && t.at(1, 1, false));
    }
    {   // the copy fails: no binding call, nothing marked; the binding call fails: asked again at the next tick
        TableSim t;
        t.f.touch();
        t.upload_rc = -5;
        STEP(t.tick() == -5 && t.at(1, 0, true) && !t.f.copying && !t.f.bound);
        t.upload_rc = 0;
        t.bind_rc = -7;
        STEP(t.tick() == -7 && t.at(2, 1, true) && t.f.copying && !t.f.bound);
        t.bind_rc = 0;
        STEP(t.tick() == 0 && t.at(3, 2, false) && t.f.bound);
    }
#undef STEP
    std::printf("host selftest: facade table: %d steps, copies and bindings as written\n", steps);
}

// params: 20 000 random parameter sets, invalid ones among them.  Every set aof_params_check takes has a grid at every level
// whose tiles and search windows lie inside the level's frame, reduction chunks that cover the grid, histogram bytes as
// the layout rule states them, and a workspace layout; more than 1 000 of the sets are valid.
static void check_params(const char *)
{
    rnd_seed();
    int bad = 0, valid = 0;
    for (int it = 0; it < 20000; it++) {
        aof_params p;
        aof_params_default(&p, (int)(rnd() % 2100) - 20, (int)(rnd() % 1300) - 20);
        p.tile = (rnd() % 5 == 0) ? (int)(rnd() % 20) : ((rnd() & 1) ? 8 : 16);
        p.search = (int)(rnd() % 11) - 1;
        p.grid_mode = (int)(rnd() % 3);
        p.num_blocks = (int)(rnd() % 12) - 1;
        p.subpixel = (int)(rnd() % 2);
        p.pyramid_levels = (int)(rnd() % 4);
        p.mean_subtract = (int)(rnd() % 2);
        p.value_threshold = (int)(rnd() % 100000) - 5;
        if (aof_params_check(&p) != 0) { bad++; continue; }
        valid++;
        for (int l = 0; l < p.pyramid_levels; l++) {
            char at[96];   // where a condition fails
            std::snprintf(at, sizeof at, "at level %d of %dx%d tile %d search %d", l, p.width, p.height, p.tile, p.search);
            int32_t g[6];
            HOLD(aof_grid(&p, l, &g[0], &g[1], &g[2], &g[3], &g[4], &g[5]) == 0, "valid parameters have no grid %s", at);
            HOLD(g[4] >= 1 && g[5] >= 1, "a grid of %d x %d blocks %s", g[4], g[5], at);
            // every tile of the grid, with its search window, lies inside the level's frame
            const int w = p.width >> l, h = p.height >> l, m = p.subpixel ? 1 : 0;
            const int lx = g[0] + (g[4] - 1) * g[2], ly = g[1] + (g[5] - 1) * g[3];
            HOLD(g[0] - p.search - m >= 0 && lx + p.tile + p.search + m <= w, "tile window leaves the frame to the left or right %s", at);
            HOLD(g[1] - p.search - m >= 0 && ly + p.tile + p.search + m <= h, "tile window leaves the frame at the top or bottom %s", at);
            // the two-step reduction of large grids covers every block with its chunks
            const int chunks = aof::reduce_chunks(g[4] * g[5]);
            HOLD(chunks >= 0 && (chunks == 0 || (long long)chunks * 4096 >= (long long)g[4] * g[5]), "%d reduction chunks do not cover %d blocks %s", chunks, g[4] * g[5], at);
            HOLD(aof::hist_bytes_per_pair(p, l) == (size_t)chunks * 2 * (2 * (2 * (size_t)aof::level_range(p, l) + 1) + 1) * 4,
                 "%zu histogram bytes a pair are not those of %d chunks %s", aof::hist_bytes_per_pair(p, l), chunks, at);
        }
        aof_ws_layout L;
        HOLD(aof_workspace_layout(&p, (int64_t)(rnd() % 5000), &L) == 0, "valid parameters (set %d, %dx%d) have no workspace layout", it, p.width, p.height);
        HOLD(L.total_bytes % 256 == 0 && L.l0_hist >= L.l0_subdirs && L.total_bytes >= L.l1_hist,
             "the workspace layout of set %d (%dx%d) is not a multiple of 256 bytes or its regions are out of order", it, p.width, p.height);
    }
    HOLD(valid > 1000, "only %d of 20000 random parameter sets are valid, no more than 1000", valid);
    std::printf("host selftest: %d valid parameter sets, %d rejected\n", valid, bad);
}

static const struct { const char *name; void (*run)(const char *case_file); bool takes_case_file; } checks[] = {
    {"params", check_params, false},
    {"packer-range", check_packer_range, false},
    {"packer", check_packer, false},
    {"checksum", check_crc_steps, false},
    {"exposure", check_exposure, false},
    {"fastdiv", check_fastdiv, false},
    {"bank-tables", check_bank_tables, false},
    {"facade-table", check_facade_table, false},
    {"choose-lane8-written", check_choose_lane8, false},
    {"xcd-permutation", check_xcd_remap, false},
    {"cols-plan", print_cols_plans, true},
    {"coarse-plan", print_coarse_plans, true},
    {"pyramid-plan", print_pyramid_plans, true},
    {"small-plan", print_small_plans, true},
    {"lane8-plan", print_lane8_plans, true},
    {"xcd-probes", print_xcd_probes, true},
    {"batch-plan", print_batch_plans, true},
    {"tile16-plan", print_tile16_plans, true},
    {"choose-lane8", print_choose_lane8, true},
    {"warp-plan", print_warp_plans, true},
};

int main(int argc, char **argv)
{
    if (argc == 2 && std::strcmp(argv[1], "list") == 0) {
        for (const auto &c : checks) std::printf("%s\n", c.name);
        return 0;
    }
    for (const auto &c : checks)
        if (argc >= 2 && std::strcmp(argv[1], c.name) == 0) {
            if (argc != (c.takes_case_file ? 3 : 2)) break;
            check_name = c.name;
            c.run(c.takes_case_file ? argv[2] : nullptr);
            return 0;
        }
    std::fprintf(stderr, "host_selftest: '%s' is no check, or is given a case file too many or too few; `host_selftest list` prints the names\n", argc >= 2 ? argv[1] : "");
    return 2;
}
