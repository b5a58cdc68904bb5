// The validity rule of a sensor record (aof_bank_sensor, include/aof.h "per-stream sensors") and of its pixel format
// (aof_set_bank_pixel_formats, "packed sensor pixels"), written once for both sides: the kernels decide with it
// (bank_sensor(), aof_bank_stream.hpp), the host answers aof_bank_sensor_valid and aof_bank_sensor_valid_format with it.
// Pure integer arithmetic on the record's fields; 64 bits, and no step can wrap.
#pragma once

#include "aof_hd.hpp"

namespace aof {

// How a format lays a row's pixels out ("raw mono pixels", include/aof.h): groups of `group_px` pixels in `group_bytes`
// bytes -- 1 in 1 (grey), 1 in 2 (every 16-bit form), 4 in 5 (Y10P), 2 in 3 (Y12P); group_px 0 for a value that is no
// format.  shift: a 16-bit form's grey value is bits shift .. shift + 7 of the pixel's little-endian word (0, 8 for the
// two LUMA16 forms, 2, 4, 6 for Y10, Y12, Y14); a packed group's leading bytes ARE its pixels' grey values.
struct BankPixelLayout {
    int32_t group_px, group_bytes, shift;
};
AOF_HD_INLINE BankPixelLayout bank_pixel_layout(uint32_t format)
{
    switch (format) {
    case 0: return BankPixelLayout{1, 1, 0};
    case 1: return BankPixelLayout{1, 2, 0};
    case 2: return BankPixelLayout{1, 2, 8};
    case 4: return BankPixelLayout{1, 2, 2};
    case 5: return BankPixelLayout{1, 2, 4};
    case 6: return BankPixelLayout{1, 2, 6};
    case 7: return BankPixelLayout{4, 5, 0};
    case 8: return BankPixelLayout{2, 3, 0};
    default: return BankPixelLayout{0, 0, 0};
    }
}

// Does the record describe a crop of w x h inside a frame whose rows are groups of G pixels in Bg bytes, the frame inside
// [0, camera_bytes) of the camera buffer, the round's frames starting `base` bytes in?  G is 1, 2 or 4 and Bg 1 .. 5
// (anything else: no); width, x0, w in pixels, pitch in bytes.  width and x0 are whole groups, so a row is
// row_bytes = width / G * Bg bytes and every 16-pixel piece of the crop starts on a group.  pitch >= row_bytes >= 1 and
// height >= 1 make (height - 1) * pitch + row_bytes a sum of non-negative terms below 2^62 + 2^34; base, then offset,
// are taken off camera_bytes only after each was seen to fit.
// bin ("binned sensor pixels"): 1, 2 or 4 (anything else: no) -- a crop pixel is the rounded mean of bin x bin sensor
// pixels, so the crop's footprint is bin * w x bin * h sensor pixels at (x0, y0); bin * w stays below 2^34.
AOF_HD_INLINE bool bank_sensor_valid_groups(uint64_t offset, int32_t pitch, int32_t width, int32_t height, int32_t x0, int32_t y0,
                                            int32_t w, int32_t h, uint64_t base, uint64_t camera_bytes, int32_t G, int32_t Bg, int32_t bin)
{
    if ((G != 1 && G != 2 && G != 4) || Bg < 1 || Bg > 5) return false;
    if (bin != 1 && bin != 2 && bin != 4) return false;
    if (width < 1 || height < 1 || (width & (G - 1)) != 0) return false;   // (G is a power of two: the remainder and, below,
    const int64_t row_bytes = (int64_t)(width >> (G >> 1)) * Bg;            //  the quotient, without a division in a kernel)
    if ((int64_t)pitch < row_bytes) return false;
    if (x0 < 0 || y0 < 0 || (x0 & (G - 1)) != 0 || (int64_t)x0 + (int64_t)bin * w > width || (int64_t)y0 + (int64_t)bin * h > height) return false;
    if (base > camera_bytes || offset > camera_bytes - base) return false;
    const uint64_t extent = (uint64_t)(height - 1) * (uint64_t)pitch + (uint64_t)row_bytes;
    return extent <= camera_bytes - base - offset;
}

// The rule for a record whose pixels have the form `format` (AOF_PIXEL_*; a value that is no format: no).
AOF_HD_INLINE bool bank_sensor_valid_format(uint64_t offset, int32_t pitch, int32_t width, int32_t height, int32_t x0, int32_t y0,
                                            int32_t w, int32_t h, uint64_t base, uint64_t camera_bytes, uint32_t format, int32_t bin)
{
    const BankPixelLayout l = bank_pixel_layout(format);
    return bank_sensor_valid_groups(offset, pitch, width, height, x0, y0, w, h, base, camera_bytes, l.group_px, l.group_bytes, bin);
}

}  // namespace aof
