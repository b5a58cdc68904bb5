// The validity rule of a sensor record WITH a bin (csrc/aof_bank_sensor_rule.hpp: bank_sensor_valid's bin parameter),
// compiled for the host under UBSan and ASan, against the same rule in 128-bit integers on a grid of edge values: every
// bin byte that matters, footprints x0 + bin * w around width with both near 2^31, crop sizes up to 2^31 - 1, offsets and
// bases near 2^64.  A step that wrapped, or a signed overflow on the way, ends the run.  Bin 1 must decide as the
// call without the argument does.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "aof_bank_sensor_rule.hpp"

typedef unsigned __int128 u128;
typedef __int128 i128;

static bool wide(uint64_t offset, int32_t pitch, int32_t width, int32_t height, int32_t x0, int32_t y0, int32_t w, int32_t h,
                 uint64_t base, uint64_t camera_bytes, int32_t bpp, int32_t bin)
{
    if (bpp != 1 && bpp != 2) return false;
    if (bin != 1 && bin != 2 && bin != 4) return false;
    if (width < 1 || height < 1 || (i128)pitch < (i128)width * bpp) return false;
    if (x0 < 0 || y0 < 0 || (i128)x0 + (i128)bin * w > width || (i128)y0 + (i128)bin * h > height) return false;
    return (u128)base + offset + (u128)(height - 1) * (u128)pitch + (u128)width * bpp <= (u128)camera_bytes;
}

int main()
{
    const int32_t top32 = INT32_MAX, half = top32 / 2, quarter = top32 / 4;
    const uint64_t top = UINT64_MAX;
    const std::vector<int32_t> widths = {-1, 0, 1, 64, 127, 128, 129, 256, 257, quarter, half, half + 1, top32 - 1, top32};
    const std::vector<int32_t> origins = {-1, 0, 1, 64, quarter - 64, half - 128, half - 127, top32 - 256, top32 - 255, top32};
    const std::vector<int32_t> crops = {1, 64, 65, quarter, quarter + 1, half, half + 1, top32};
    const uint64_t ext = (uint64_t)(top32 - 1) * (uint64_t)top32 + 2 * (uint64_t)half;
    const std::vector<uint64_t> words = {0, 8192, ext, ext + 5, top - ext - 4, top};
    long checked = 0, valid = 0, same = 0;
    for (int32_t bin : {0, 1, 2, 3, 4, 5, 8, 255, -1, -4})
        for (int32_t bpp : {0, 1, 2, 3})
            for (int32_t width : widths)
                for (int32_t pitch : {width, top32})
                    for (int32_t height : {0, 1, 64, 256, 257, top32})
                        for (int32_t x0 : origins)
                            for (int32_t y0 : {-1, 0, 1, 193})
                                for (int32_t w : crops)
                                    for (int32_t h : {1, 64, top32})
                                        for (uint64_t offset : words)
                                            for (uint64_t bytes : {words[1], words[3], top}) {
                                                const uint64_t base = offset == top ? 1 : 0;
                                                const bool got = aof::bank_sensor_valid(offset, pitch, width, height, x0, y0, w, h, base, bytes, bpp, bin);
                                                const bool want = wide(offset, pitch, width, height, x0, y0, w, h, base, bytes, bpp, bin);
                                                if (got != want) {
                                                    std::printf("rule differs: bin %d bpp %d offset %llu pitch %d width %d height %d x0 %d y0 %d w %d h %d bytes %llu: %d, want %d\n",
                                                                bin, bpp, (unsigned long long)offset, pitch, width, height, x0, y0, w, h,
                                                                (unsigned long long)bytes, (int)got, (int)want);
                                                    return 1;
                                                }
                                                if (bin == 1) {
                                                    if (got != aof::bank_sensor_valid(offset, pitch, width, height, x0, y0, w, h, base, bytes, bpp)) {
                                                        std::printf("bin 1 decides otherwise than the call without a bin\n");
                                                        return 1;
                                                    }
                                                    same++;
                                                }
                                                checked++;
                                                valid += want;
                                            }
    std::printf("%ld records checked, %ld valid, %ld with bin 1: the rule with a bin and its 128-bit restatement agree\n", checked, valid, same);
    return valid > 100 && checked - valid > 100 && same > 100 ? 0 : 2;
}
