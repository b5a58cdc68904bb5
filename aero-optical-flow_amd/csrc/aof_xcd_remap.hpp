// The workgroup placement of the 1-D launches that walk a frame row by row (the flat lane-per-block 8x8 kernels, the
// 16x16 kernel): one text for the kernels and for the host (tests/native/host_selftest.cpp).
#pragma once

#include <cstdint>

#include "aof_hd.hpp"

namespace aof {

// XCD-aware remap of a 1-D grid (workgroups b and b+8 share an XCD's L2 under round-robin placement): XCD k gets
// one contiguous chunk of logical ids, so consecutive block rows of one frame pair are served by the same L2.
// Placement affects speed, never results -- as long as the map is a bijection of [0, total).  That is proven, not
// supposed: tests/test_lane8_plan_ref.py holds the Python restatement (tests/lane8_plan_ref.py) to be a permutation of
// [0, total) for every total from 1 to 4 096 and for the workgroup count of every flat 8x8 case, with the logical ids
// of an XCD contiguous, and the sanitizer self-test holds THIS function to that restatement value by value for every
// total up to 4 096 and at the ends of the large ones.  The 16x16 kernel's launches are covered by the same proof
// (their total is a workgroup count like any other); its own block-row plan by tests/tile16_rows_ref.py, whose device
// cases launch one and two block rows per pair at totals off the multiples of 8.
AOF_HD_INLINE uint32_t xcd_remap(uint32_t b, uint32_t total)
{
    const uint32_t q = total / 8, r = total % 8, xcd = b % 8, slot = b / 8;
    const uint32_t base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + slot;
}

}  // namespace aof
