// The validity rule of a sensor record (aof_bank_sensor, include/aof.h "per-stream sensors") and of its pixel format
// (aof_set_bank_pixel_formats, "packed sensor pixels"), written once for both sides: the kernels decide with it
// (bank_sensor(), aof_bank_stream.hpp), the host answers aof_bank_sensor_valid and aof_bank_sensor_valid_format with it.
// Pure integer arithmetic on the record's fields; 64 bits, and no step can wrap.
#pragma once

#include "aof_hd.hpp"

namespace aof {

// Bytes per pixel of a format (AOF_PIXEL_*): 1 for grey, 2 for the two packed forms, 0 for a value that is no format.
AOF_HD_INLINE int32_t bank_pixel_bpp(uint32_t format) { return format == 0 ? 1 : (format <= 2 ? 2 : 0); }
// Which byte of a pixel holds its grey value: 0, or 1 for AOF_PIXEL_LUMA16_HI.
AOF_HD_INLINE int32_t bank_pixel_phase(uint32_t format) { return format == 2 ? 1 : 0; }

// Does the record describe a crop of w x h inside a frame of `bpp` bytes per pixel that lies inside [0, camera_bytes) of
// the camera buffer, the round's frames starting `base` bytes in?  bpp is 1 or 2 (anything else: no); width, x0, w in
// pixels, pitch in bytes.  pitch >= width * bpp >= 1 and height >= 1 make (height - 1) * pitch + width * bpp a sum of
// non-negative terms below 2^62 + 2^32; base, then offset, are taken off camera_bytes only after each was seen to fit.
// bin ("binned sensor pixels"): 1, 2 or 4 (anything else: no) -- a crop pixel is the rounded mean of bin x bin sensor
// pixels, so the crop's footprint is bin * w x bin * h sensor pixels at (x0, y0); bin * w stays below 2^34.
AOF_HD_INLINE bool bank_sensor_valid(uint64_t offset, int32_t pitch, int32_t width, int32_t height, int32_t x0, int32_t y0,
                                     int32_t w, int32_t h, uint64_t base, uint64_t camera_bytes, int32_t bpp = 1, int32_t bin = 1)
{
    if (bpp < 1 || bpp > 2) return false;
    if (bin != 1 && bin != 2 && bin != 4) return false;
    if (width < 1 || height < 1 || (int64_t)pitch < (int64_t)width * bpp) return false;
    if (x0 < 0 || y0 < 0 || (int64_t)x0 + (int64_t)bin * w > width || (int64_t)y0 + (int64_t)bin * h > height) return false;
    if (base > camera_bytes || offset > camera_bytes - base) return false;
    const uint64_t extent = (uint64_t)(height - 1) * (uint64_t)pitch + (uint64_t)width * (uint64_t)bpp;
    return extent <= camera_bytes - base - offset;
}

}  // namespace aof
