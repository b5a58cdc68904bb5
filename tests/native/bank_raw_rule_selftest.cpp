// The validity rule of a sensor record whose pixels come in groups (csrc/aof_bank_sensor_rule.hpp: bank_pixel_layout,
// bank_sensor_valid_groups, bank_sensor_valid_format -- include/aof.h "raw mono pixels"), compiled for the host under UBSan
// and ASan, against the same rule in 128-bit integers: the layout of every format byte, then a grid of edge values --
// widths and origins around the group sizes, pitch around row_bytes, width near 2^31, offsets and bases near 2^64,
// (height - 1) * pitch near 2^62, every bin byte -- and the extent at equality and one byte short for every format.
// A step that wrapped, or a signed overflow on the way, ends the run.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "aof_bank_sensor_rule.hpp"

typedef unsigned __int128 u128;
typedef __int128 i128;

// (G, Bg, shift) by the header's table; G 0: no format
static void table(uint32_t f, int &G, int &Bg, int &shift)
{
    G = 0; Bg = 0; shift = 0;
    switch (f) {
    case 0: G = 1; Bg = 1; break;
    case 1: G = 1; Bg = 2; break;
    case 2: G = 1; Bg = 2; shift = 8; break;
    case 4: G = 1; Bg = 2; shift = 2; break;
    case 5: G = 1; Bg = 2; shift = 4; break;
    case 6: G = 1; Bg = 2; shift = 6; break;
    case 7: G = 4; Bg = 5; break;
    case 8: G = 2; Bg = 3; break;
    default: break;
    }
}

static bool wide(uint64_t offset, int32_t pitch, int32_t width, int32_t height, int32_t x0, int32_t y0, int32_t w, int32_t h,
                 uint64_t base, uint64_t camera_bytes, uint32_t format, int32_t bin)
{
    int G, Bg, shift;
    table(format, G, Bg, shift);
    if (G == 0) return false;
    if (bin != 1 && bin != 2 && bin != 4) return false;
    if (width < 1 || height < 1 || width % G != 0) return false;
    const i128 row_bytes = (i128)(width / G) * Bg;
    if ((i128)pitch < row_bytes) return false;
    if (x0 < 0 || y0 < 0 || x0 % G != 0 || (i128)x0 + (i128)bin * w > width || (i128)y0 + (i128)bin * h > height) return false;
    return (u128)base + offset + (u128)(height - 1) * (u128)pitch + (u128)row_bytes <= (u128)camera_bytes;
}

static int differs(const char *what, uint32_t format, uint64_t offset, int32_t pitch, int32_t width, int32_t height, int32_t x0, int32_t y0,
                   int32_t bin, uint64_t base, uint64_t bytes, bool got, bool want)
{
    std::printf("%s differs: format %u offset %llu pitch %d width %d height %d x0 %d y0 %d bin %d base %llu bytes %llu: %d, want %d\n", what,
                format, (unsigned long long)offset, pitch, width, height, x0, y0, bin, (unsigned long long)base, (unsigned long long)bytes,
                (int)got, (int)want);
    return 1;
}

int main()
{
    const int32_t top32 = INT32_MAX, half = top32 / 2;
    const uint64_t top = UINT64_MAX;
    for (uint32_t f = 0; f < 256; f++) {
        int G, Bg, shift;
        table(f, G, Bg, shift);
        const aof::BankPixelLayout l = aof::bank_pixel_layout(f);
        if (l.group_px != G || l.group_bytes != Bg || l.shift != shift) {
            std::printf("format %u: group_px %d group_bytes %d shift %d\n", f, l.group_px, l.group_bytes, l.shift);
            return 1;
        }
        // the older helpers keep their answers: whole bytes per pixel for the first three formats, 0 for everything else
        if (aof::bank_pixel_bpp(f) != (f == 0 ? 1 : f <= 2 ? 2 : 0) || aof::bank_pixel_phase(f) != (f == 2 ? 1 : 0)) {
            std::printf("format %u: bpp %d phase %d\n", f, aof::bank_pixel_bpp(f), aof::bank_pixel_phase(f));
            return 1;
        }
    }
    const std::vector<int32_t> widths = {INT32_MIN, -1, 0, 1, 64, 126, 127, 128, 129, 130, half + 1, top32 - 3, top32};
    const std::vector<int32_t> pitches = {INT32_MIN, -1, 0, 64, 79, 80, 127, 128, 159, 160, 191, 192, 255, 256, top32};
    const std::vector<int32_t> origins = {-1, 0, 1, 2, 3, 4, 62, 64, 66, top32 - 67, top32};
    const uint64_t tall = (uint64_t)(top32 - 1) * (uint64_t)top32;
    const std::vector<uint64_t> offsets = {0, 1, 8192, (uint64_t)1 << 40, top - tall - 200, top};
    const std::vector<uint64_t> bases = {0, 1, top - 8192, top};
    const std::vector<uint64_t> sizes = {8192, 16384, tall + 6 * (uint64_t)half, top};
    long checked = 0, valid = 0;
    for (uint32_t format : {0u, 1u, 2u, 3u, 4u, 5u, 6u, 7u, 8u, 9u, 255u})
        for (int32_t pitch : pitches)
            for (int32_t width : widths)
                for (int32_t height : {0, 1, 64, 65, top32})
                    for (int32_t x0 : origins)
                        for (int32_t y0 : {-1, 0, 1})
                            for (int32_t bin : {1, 2, 4, 3})
                                for (uint64_t offset : offsets)
                                    for (uint64_t base : bases)
                                        for (uint64_t bytes : sizes) {
                                            const int32_t w = bin == 2 ? 32 : (bin == 4 ? 16 : 64);   // (footprints of 64 sensor pixels)
                                            const bool got = aof::bank_sensor_valid_format(offset, pitch, width, height, x0, y0, w, w, base, bytes, format, bin);
                                            const bool want = wide(offset, pitch, width, height, x0, y0, w, w, base, bytes, format, bin);
                                            if (got != want) return differs("the rule", format, offset, pitch, width, height, x0, y0, bin, base, bytes, got, want);
                                            const aof::BankPixelLayout l = aof::bank_pixel_layout(format);
                                            if (aof::bank_sensor_valid_groups(offset, pitch, width, height, x0, y0, w, w, base, bytes, l.group_px,
                                                                              l.group_bytes, bin) != want)
                                                return differs("the rule by groups", format, offset, pitch, width, height, x0, y0, bin, base, bytes, !want, want);
                                            if (format <= 2 && aof::bank_sensor_valid(offset, pitch, width, height, x0, y0, w, w, base, bytes,
                                                                                      aof::bank_pixel_bpp(format), bin) != want)
                                                return differs("the G = 1 case", format, offset, pitch, width, height, x0, y0, bin, base, bytes, !want, want);
                                            checked++;
                                            valid += want;
                                        }
    // every format: the extent at equality and one byte short, pitch at row_bytes and one less, width and x0 one off a group
    long edges = 0;
    for (uint32_t format : {0u, 1u, 2u, 4u, 5u, 6u, 7u, 8u})
        for (int32_t bin : {1, 2, 4}) {
            int G, Bg, shift;
            table(format, G, Bg, shift);
            const int32_t width = 4 * 64 + 8, height = 4 * 64 + 3, w = 64, x0 = 4, y0 = 3;
            const int32_t row = width / G * Bg;
            const uint64_t offset = 100, base = 7;
            for (int32_t pitch : {row, row + 3}) {
                const uint64_t end = base + offset + (uint64_t)(height - 1) * pitch + row;
                struct { int32_t pitch, width, x0; uint64_t bytes; } cases[] = {
                    {pitch, width, x0, end}, {pitch, width, x0, end - 1}, {row - 1, width, x0, top}, {pitch, width + 1, x0, top},
                    {pitch, width, x0 + 1, top}, {pitch, width, x0 + 8, top}, {pitch, width, x0 + 12, top}};
                for (auto &c : cases) {
                    const bool got = aof::bank_sensor_valid_format(offset, c.pitch, c.width, height, c.x0, y0, w, w, base, c.bytes, format, bin);
                    const bool want = wide(offset, c.pitch, c.width, height, c.x0, y0, w, w, base, c.bytes, format, bin);
                    if (got != want) return differs("an edge", format, offset, c.pitch, c.width, height, c.x0, y0, bin, base, c.bytes, got, want);
                    edges += want;
                }
                if (!wide(offset, pitch, width, height, x0, y0, w, w, base, end, format, bin) ||
                    wide(offset, pitch, width, height, x0, y0, w, w, base, end - 1, format, bin)) {
                    std::printf("the restatement misses the extent of format %u\n", format);
                    return 1;
                }
            }
        }
    std::printf("%ld records checked, %ld valid, %ld valid edges: the rule by pixel groups and its 128-bit restatement agree\n", checked,
                valid, edges);
    return valid > 100 && checked - valid > 100 && edges > 40 ? 0 : 2;
}
