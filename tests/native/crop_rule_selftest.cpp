// The validity rule of a crop source (csrc/aof_bank_sensor_rule.hpp: bank_pixel_layout, bank_sensor_valid_groups,
// bank_sensor_valid_format -- include/aof.h "per-stream sensors", "packed sensor pixels", "binned sensor pixels", "raw mono
// pixels"), compiled for the host under UBSan and ASan, against ONE restatement by pixel groups in 128-bit integers: the
// layout of every format byte, then edge values on every axis -- widths and origins around the group sizes and near 2^29,
// 2^30 and 2^31, pitch around row_bytes, crops with w != h up to 2^31 - 1, every bin byte that matters, group shapes that
// are no format, offsets and bases next to 2^64 - extent, (height - 1) * pitch near 2^62 -- and the extent at equality and
// one byte short for every format and bin.  The axes are too many for one product; three products hold every value of
// every axis, every (format or group shape) x bin and every (offset, base, bytes).  A step that wrapped, or a signed
// overflow on the way, ends the run.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "aof_bank_sensor_rule.hpp"

typedef unsigned __int128 u128;
typedef __int128 i128;

struct Shape { int32_t G, Bg, format; };   // format -1: a group shape given straight to bank_sensor_valid_groups

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
                 uint64_t base, uint64_t camera_bytes, int32_t G, int32_t Bg, int32_t bin)
{
    if ((G != 1 && G != 2 && G != 4) || Bg < 1 || Bg > 5) return false;
    if (bin != 1 && bin != 2 && bin != 4) return false;
    if (width < 1 || height < 1 || width % G != 0) return false;
    const i128 row_bytes = (i128)(width / G) * Bg;
    if ((i128)pitch < row_bytes) return false;
    if (x0 < 0 || y0 < 0 || x0 % G != 0 || (i128)x0 + (i128)bin * w > width || (i128)y0 + (i128)bin * h > height) return false;
    return (u128)base + offset + (u128)(height - 1) * (u128)pitch + (u128)row_bytes <= (u128)camera_bytes;
}

static long checked = 0, valid = 0, bin1 = 0;

// One record: the rule by groups and, for a format, the rule by format, against the restatement.  true: they differ.
static bool differs(const Shape &s, uint64_t offset, int32_t pitch, int32_t width, int32_t height, int32_t x0, int32_t y0, int32_t w, int32_t h,
                    int32_t bin, uint64_t base, uint64_t bytes)
{
    const bool want = wide(offset, pitch, width, height, x0, y0, w, h, base, bytes, s.G, s.Bg, bin);
    const bool groups = aof::bank_sensor_valid_groups(offset, pitch, width, height, x0, y0, w, h, base, bytes, s.G, s.Bg, bin);
    const bool format = s.format < 0 ? want : aof::bank_sensor_valid_format(offset, pitch, width, height, x0, y0, w, h, base, bytes,
                                                                            (uint32_t)s.format, bin);
    checked++;
    valid += want;
    bin1 += bin == 1;
    if (groups == want && format == want) return false;
    std::printf("the rule differs: G %d Bg %d format %d offset %llu pitch %d width %d height %d x0 %d y0 %d w %d h %d bin %d base %llu bytes %llu: "
                "by groups %d, by format %d, want %d\n", s.G, s.Bg, s.format, (unsigned long long)offset, pitch, width, height, x0, y0, w, h, bin,
                (unsigned long long)base, (unsigned long long)bytes, (int)groups, (int)format, (int)want);
    return true;
}

int main()
{
    const int32_t top32 = INT32_MAX, half = top32 / 2, quarter = top32 / 4;
    const uint64_t top = UINT64_MAX;
    std::vector<Shape> shapes;
    for (uint32_t f = 0; f < 256; f++) {
        int G, Bg, shift;
        table(f, G, Bg, shift);
        const aof::BankPixelLayout l = aof::bank_pixel_layout(f);
        if (l.group_px != G || l.group_bytes != Bg || l.shift != shift) {
            std::printf("format %u: group_px %d group_bytes %d shift %d\n", f, l.group_px, l.group_bytes, l.shift);
            return 1;
        }
        if (f < 10 || f == 255) shapes.push_back(Shape{G, Bg, (int32_t)f});
    }
    const std::vector<Shape> formats = shapes;   // formats 0 .. 9 and 255
    for (const Shape &s : {Shape{1, 0, -1}, Shape{1, 3, -1}, Shape{1, 6, -1}, Shape{0, 1, -1}, Shape{3, 3, -1}, Shape{8, 5, -1}, Shape{2, 6, -1},
                           Shape{4, 0, -1}, Shape{2, 3, -1}, Shape{4, 5, -1}})
        shapes.push_back(s);
    // pitch 0x7FFFFFFE..: top32 - 1, top32; -2 stands for "the width" (a grey row without padding, whatever the width is)
    const std::vector<int32_t> pitches = {INT32_MIN, -1, 0, 1, 63, 64, 65, 79, 80, 127, 128, 129, 159, 160, 191, 192, 255, 256, half, half + 1,
                                          top32 - 1, top32, -2};
    const std::vector<int32_t> widths = {INT32_MIN, -1, 0, 1, 63, 64, 65, 126, 127, 128, 129, 130, 256, 257, quarter, half, half + 1, top32 - 3,
                                         top32 - 1, top32};
    const std::vector<int32_t> heights = {INT32_MIN, -1, 0, 1, 63, 64, 65, 128, 256, 257, top32 - 1, top32};
    const std::vector<int32_t> origins = {INT32_MIN, -1, 0, 1, 2, 3, 4, 62, 64, 66, quarter - 64, half - 128, half - 127, half - 64, half - 63,
                                          top32 - 256, top32 - 255, top32 - 67, top32 - 64, top32 - 63, top32};
    const std::vector<int32_t> rows = {-1, 0, 1, 193, top32 - 63};
    const std::vector<int32_t> crops = {1, 16, 32, 64, 65, quarter, quarter + 1, half, half + 1, top32};
    const std::vector<int32_t> crop_rows = {1, 16, 32, 64, top32};
    const std::vector<int32_t> bins = {0, 1, 2, 3, 4, 5, 8, 255, -1, -4};
    const uint64_t tall = (uint64_t)(top32 - 1) * (uint64_t)top32;
    const uint64_t ext1 = tall + 64, ext2 = tall + 2 * (uint64_t)half;   // the extent of the tallest frame of 64 grey / half 16-bit pixels
    const std::vector<uint64_t> words = {0, 1, 4095, 4096, 4097, 8191, 8192, 8193, (uint64_t)1 << 40, ext1, ext1 + 5, ext2, ext2 + 5,
                                         top - ext1 - 5, top - ext1 - 4, top - ext2 - 5, top - ext2 - 4, top - tall - 200, top - 8192, top - 4096,
                                         top - 1, top};
    const std::vector<uint64_t> sizes = {4096, 8192, 16384, ext1, ext1 + 5, ext2, ext2 + 5, tall + 6 * (uint64_t)half, top - 1, top};

    // 1. rows and footprints along x: every (format or group shape) x bin, with every pitch, width, origin and crop width
    struct { int32_t height, y0, h; } const ys[] = {{top32, 0, 64}, {64, 0, 16}, {257, 193, 64}};
    struct { uint64_t offset, bytes; } const spans[] = {{0, top}, {8192, ext2 + 5}};
    for (const Shape &s : shapes)
        for (int32_t bin : bins)
            for (int32_t p : pitches)
                for (int32_t width : widths)
                    for (int32_t x0 : origins)
                        for (int32_t w : crops)
                            for (const auto &y : ys)
                                for (const auto &span : spans)
                                    if (differs(s, span.offset, p == -2 ? width : p, width, y.height, x0, y.y0, w, y.h, bin, 0, span.bytes)) return 1;
    // 2. footprints along both axes (w != h, both up to 2^31 - 1) for every bin, in the four shapes of a row
    for (const Shape &s : {formats[0], formats[1], formats[7], formats[8]})
        for (int32_t bin : bins)
            for (int32_t width : widths)
                for (int32_t pitch : {width, top32})
                    for (int32_t height : heights)
                        for (int32_t x0 : origins)
                            for (int32_t y0 : rows)
                                for (int32_t w : crops)
                                    for (int32_t h : crop_rows)
                                        if (differs(s, 8192, pitch, width, height, x0, y0, w, h, bin, 0, ext2 + 5)) return 1;
    // 3. the extent: every (offset, base, bytes) with every height and pitch, for every format
    for (const Shape &s : formats)
        for (int32_t bin : {1, 2, 3})
            for (int32_t width : {64, 128, half + 1, top32})
                for (int32_t p : pitches)
                    for (int32_t height : heights)
                        for (uint64_t offset : words)
                            for (uint64_t base : words)
                                for (uint64_t bytes : sizes)
                                    if (differs(s, offset, p == -2 ? width : p, width, height, 0, 0, 16, 16, bin, base, bytes)) return 1;
    // every format and bin: the extent at equality and one byte short, pitch at row_bytes and one less, width and x0 one off a group
    long edges = 0;
    for (const Shape &s : formats) {
        if (s.G == 0) continue;
        for (int32_t bin : {1, 2, 4}) {
            const int32_t width = 4 * 64 + 8, height = 4 * 64 + 3, w = 64, x0 = 4, y0 = 3;
            const int32_t row = width / s.G * s.Bg;
            const uint64_t offset = 100, base = 7;
            for (int32_t pitch : {row, row + 3}) {
                const uint64_t end = base + offset + (uint64_t)(height - 1) * pitch + row;
                struct { int32_t pitch, width, x0; uint64_t bytes; } const cases[] = {
                    {pitch, width, x0, end}, {pitch, width, x0, end - 1}, {row - 1, width, x0, top}, {pitch, width + 1, x0, top},
                    {pitch, width, x0 + 1, top}, {pitch, width, x0 + 8, top}, {pitch, width, x0 + 12, top}};
                for (const auto &c : cases) {
                    if (differs(s, offset, c.pitch, c.width, height, c.x0, y0, w, w, bin, base, c.bytes)) return 1;
                    edges += wide(offset, c.pitch, c.width, height, c.x0, y0, w, w, base, c.bytes, s.G, s.Bg, bin);
                }
                if (!wide(offset, pitch, width, height, x0, y0, w, w, base, end, s.G, s.Bg, bin) ||
                    wide(offset, pitch, width, height, x0, y0, w, w, base, end - 1, s.G, s.Bg, bin)) {
                    std::printf("the restatement misses the extent of format %d\n", s.format);
                    return 1;
                }
            }
        }
    }
    std::printf("%ld records checked, %ld valid, %ld with bin 1, %ld valid edges: the rule by pixel groups and its 128-bit restatement agree\n",
                checked, valid, bin1, edges);
    return valid > 100 && checked - valid > 100 && edges > 40 && bin1 > 100 ? 0 : 2;
}
