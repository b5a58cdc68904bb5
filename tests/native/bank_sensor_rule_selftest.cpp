// The validity rule of a sensor record (csrc/aof_bank_sensor_rule.hpp, the function the kernels decide with), compiled
// for the host under UBSan and ASan, against the same rule in 128-bit integers on a grid of edge values: every field at
// its limits, offsets and bases near 2^64, (height - 1) * pitch near 2^62.  A step that wrapped, or a signed overflow on
// the way, ends the run.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "aof_bank_sensor_rule.hpp"

typedef unsigned __int128 u128;
typedef __int128 i128;

static bool wide(uint64_t offset, int32_t pitch, int32_t width, int32_t height, int32_t x0, int32_t y0, int32_t w, int32_t h,
                 uint64_t base, uint64_t camera_bytes)
{
    if (width < 1 || height < 1 || pitch < width) return false;
    if (x0 < 0 || y0 < 0 || (i128)x0 + w > width || (i128)y0 + h > height) return false;
    return (u128)base + offset + (u128)(height - 1) * (u128)pitch + (u128)width <= (u128)camera_bytes;
}

int main()
{
    const int32_t top32 = INT32_MAX;
    const uint64_t top = UINT64_MAX;
    const std::vector<int32_t> dims = {INT32_MIN, -1, 0, 1, 63, 64, 65, 128, top32 - 1, top32};
    const std::vector<int32_t> origins = {INT32_MIN, -1, 0, 1, 64, top32 - 64, top32 - 63, top32};
    const uint64_t ext = (uint64_t)(top32 - 1) * (uint64_t)top32 + 64;
    const std::vector<uint64_t> words = {0, 1, 4095, 4096, 4097, (uint64_t)1 << 40, ext, ext + 5, top - ext - 5, top - ext - 4,
                                         top - 4096, top - 1, top};
    long checked = 0, valid = 0;
    for (int32_t pitch : dims)
        for (int32_t width : dims)
            for (int32_t height : dims)
                for (int32_t x0 : origins)
                    for (int32_t y0 : {-1, 0, 1, top32 - 63})
                        for (uint64_t offset : words)
                            for (uint64_t base : words)
                                for (uint64_t bytes : {words[3], words[6], words[7], top - 1, top}) {
                                    const bool got = aof::bank_sensor_valid(offset, pitch, width, height, x0, y0, 64, 64, base, bytes);
                                    const bool want = wide(offset, pitch, width, height, x0, y0, 64, 64, base, bytes);
                                    if (got != want) {
                                        std::printf("rule differs: offset %llu pitch %d width %d height %d x0 %d y0 %d base %llu bytes %llu: %d, want %d\n",
                                                    (unsigned long long)offset, pitch, width, height, x0, y0, (unsigned long long)base,
                                                    (unsigned long long)bytes, (int)got, (int)want);
                                        return 1;
                                    }
                                    checked++;
                                    valid += want;
                                }
    std::printf("%ld records checked, %ld valid: the rule and its 128-bit restatement agree\n", checked, valid);
    return valid > 100 && checked - valid > 100 ? 0 : 2;
}
