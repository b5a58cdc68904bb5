// The validity rule of a sensor record WITH a pixel format (csrc/aof_bank_sensor_rule.hpp: bank_sensor_valid's bpp
// parameter, bank_pixel_bpp, bank_pixel_phase), compiled for the host under UBSan and ASan, against the same rule in
// 128-bit integers on a grid of edge values: every format byte, pitch around width * bpp with width near 2^31, offsets and
// bases near 2^64, (height - 1) * pitch near 2^62.  A step that wrapped, or a signed overflow on the way, ends the run.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "aof_bank_sensor_rule.hpp"

typedef unsigned __int128 u128;
typedef __int128 i128;

static bool wide(uint64_t offset, int32_t pitch, int32_t width, int32_t height, int32_t x0, int32_t y0, int32_t w, int32_t h,
                 uint64_t base, uint64_t camera_bytes, uint32_t format)
{
    if (format > 2) return false;
    const int bpp = format == 0 ? 1 : 2;
    if (width < 1 || height < 1 || (i128)pitch < (i128)width * bpp) return false;
    if (x0 < 0 || y0 < 0 || (i128)x0 + w > width || (i128)y0 + h > height) return false;
    return (u128)base + offset + (u128)(height - 1) * (u128)pitch + (u128)width * bpp <= (u128)camera_bytes;
}

int main()
{
    const int32_t top32 = INT32_MAX, half = top32 / 2;
    const uint64_t top = UINT64_MAX;
    const std::vector<int32_t> dims = {INT32_MIN, -1, 0, 1, 64, 127, 128, 129, half, half + 1, top32 - 1, top32};
    const std::vector<int32_t> origins = {-1, 0, 1, 64, half - 64, half - 63, top32 - 64, top32};
    const uint64_t ext = (uint64_t)(top32 - 1) * (uint64_t)top32 + 2 * (uint64_t)half;
    const std::vector<uint64_t> words = {0, 1, 8191, 8192, 8193, (uint64_t)1 << 40, ext, ext + 5, top - ext - 5, top - ext - 4, top - 8192, top};
    for (uint32_t f = 0; f < 256; f++) {
        const int32_t bpp = aof::bank_pixel_bpp(f), phase = aof::bank_pixel_phase(f);
        if (bpp != (f == 0 ? 1 : f <= 2 ? 2 : 0) || phase != (f == 2 ? 1 : 0)) {
            std::printf("format %u: bpp %d phase %d\n", f, bpp, phase);
            return 1;
        }
    }
    long checked = 0, valid = 0;
    for (uint32_t format : {0u, 1u, 2u, 3u, 255u})
        for (int32_t pitch : dims)
            for (int32_t width : dims)
                for (int32_t height : {-1, 0, 1, 64, 65, top32})
                    for (int32_t x0 : origins)
                        for (int32_t y0 : {-1, 0, 1})
                            for (uint64_t offset : words)
                                for (uint64_t base : words)
                                    for (uint64_t bytes : {words[3], words[6], words[7], top - 1, top}) {
                                        const bool got = aof::bank_sensor_valid(offset, pitch, width, height, x0, y0, 64, 64, base, bytes,
                                                                                aof::bank_pixel_bpp(format));
                                        const bool want = wide(offset, pitch, width, height, x0, y0, 64, 64, base, bytes, format);
                                        if (got != want) {
                                            std::printf("rule differs: format %u offset %llu pitch %d width %d height %d x0 %d y0 %d base %llu bytes %llu: %d, want %d\n",
                                                        format, (unsigned long long)offset, pitch, width, height, x0, y0, (unsigned long long)base,
                                                        (unsigned long long)bytes, (int)got, (int)want);
                                            return 1;
                                        }
                                        checked++;
                                        valid += want;
                                    }
    std::printf("%ld records checked, %ld valid: the rule with a format and its 128-bit restatement agree\n", checked, valid);
    return valid > 100 && checked - valid > 100 ? 0 : 2;
}
