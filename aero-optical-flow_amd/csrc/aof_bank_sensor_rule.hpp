// The validity rule of a sensor record (aof_bank_sensor, include/aof.h "per-stream sensors"), written once for both
// sides: the kernels decide with it (bank_sensor(), aof_bank_stream.hpp), the host answers aof_bank_sensor_valid with
// it.  Pure integer arithmetic on the record's fields; 64 bits, and no step can wrap.
#pragma once

#include "aof_hd.hpp"

namespace aof {

// Does the record describe a crop of w x h inside a frame that lies inside [0, camera_bytes) of the camera buffer, the
// round's frames starting `base` bytes in?  pitch >= width >= 1 and height >= 1 make (height - 1) * pitch + width a sum
// of non-negative terms below 2^62 + 2^31; base, then offset, are taken off camera_bytes only after each was seen to fit.
AOF_HD_INLINE bool bank_sensor_valid(uint64_t offset, int32_t pitch, int32_t width, int32_t height, int32_t x0, int32_t y0,
                                     int32_t w, int32_t h, uint64_t base, uint64_t camera_bytes)
{
    if (width < 1 || height < 1 || pitch < width) return false;
    if (x0 < 0 || y0 < 0 || (int64_t)x0 + w > width || (int64_t)y0 + h > height) return false;
    if (base > camera_bytes || offset > camera_bytes - base) return false;
    const uint64_t extent = (uint64_t)(height - 1) * (uint64_t)pitch + (uint64_t)width;
    return extent <= camera_bytes - base - offset;
}

}  // namespace aof
