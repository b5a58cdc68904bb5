// The crop source of the camera forms: how a window of w x h grey pixels lies in a sensor frame (row pitch, pixel format,
// binning), the ONE fetch of 16 of its pixels and the order in which a kernel makes its fetches.  Below the one-workgroup
// pair (aof_flow_small.hpp, pass A) and everything of the bank (aof_bank_stream.hpp, k_ingest.hip): a new layout or
// binning factor is a change to this file.  Which sources may be read at all is aof_bank_sensor_rule.hpp.
#pragma once

#include "aof_device.hpp"

namespace aof {

namespace {

// A window's rows: `pitch` bytes apart, groups of gb bytes -- 1 (grey), 2 (a 16-bit word whose grey value is bits
// shift .. shift + 7), 5 (Y10P's four pixels), 3 (Y12P's two) --, and bin x bin sensor pixels per pixel of the window
// (1, 2, 4).  Workgroup-uniform wherever it is used; crop_grey's constants in every kernel without a sensor argument.
// (This field order keeps k_ingest's code: with pitch in front its sensor instantiation took other registers; LAB_LOG.md.)
struct CropSource { int32_t bin, shift, gb, pitch; };
// Grey, unbinned rows `pitch` bytes apart: every source without a sensor record.
__device__ __forceinline__ CropSource crop_grey(int32_t pitch) { return CropSource{1, 0, 1, pitch}; }

// The order in which a kernel fetches the 16-pixel pieces of a window, by what a piece costs: grey pieces are one load
// each, so a trip holds as many as the kernel keeps loads in flight; 16-bit pieces are two loads, so half as many; binned
// pieces (bin rows of up to eight loads) and MIPI-packed ones (gb 5, 3: a load and a part) go one behind the other.
enum CropFetch { kFetchFullTrip, kFetchHalfTrip, kFetchOnePiece };
__device__ __forceinline__ CropFetch crop_fetch(const CropSource &c)
{
    return c.bin != 1 || c.gb > 2 ? kFetchOnePiece : (c.gb != 1 ? kFetchHalfTrip : kFetchFullTrip);
}

// Source bytes of 16 pixels of a row: 16 pixels are 16, 8 or 4 whole groups of gb bytes (16, 32, 20, 24 bytes).
__device__ __forceinline__ int piece_bytes(int gb) { return gb == 5 ? 20 : (gb == 3 ? 24 : 16 * gb); }

// The grey value of pixel x of the row whose first group starts at `row` (the per-pixel path of k_ingest; the header's
// table, include/aof.h "raw mono pixels"): a grey byte, bits shift .. shift + 7 of a little-endian word, or one of a
// packed group's leading bytes.  Reads bytes of pixel x's own group only.
__device__ __forceinline__ uint32_t crop_pixel(const uint8_t *row, int64_t x, int gb, int shift)
{
    if (gb == 1) return row[x];
    if (gb == 2) return (((uint32_t)row[2 * x] | (uint32_t)row[2 * x + 1] << 8) >> shift) & 0xFFu;
    if (gb == 5) return row[(x >> 2) * 5 + (x & 3)];
    return row[(x >> 1) * 3 + (x & 1)];
}

// The ONE fetch of a crop: pixels 16 x .. 16 x + 15 of the crop row whose first group starts at `row`, as 16 grey bytes.
// gb 1: one 16-byte load wherever the row starts.  gb 2 (16-bit pixels, the grey value in bits shift .. shift + 7 of
// each little-endian word): the 32 source bytes in two 16-byte loads, every dword shifted right by the uniform `shift`
// -- byte 0 of d >> shift is one pixel's grey value, byte 2 the next one's -- and v_perm_b32 takes bytes 0 and 2 of
// each pair of dwords.  gb 5 (Y10P): exactly the piece's 20 bytes, 16 + 4; a group's four leading bytes are its grey
// values, and the groups start at bytes 0, 5, 10, 15: dword 0, then v_alignbyte_b32 by 1, 2, 3 across the seams.  gb 3
// (Y12P): exactly 24 bytes, 16 + 8; a group's two leading bytes, so a dword of four pixels is bytes 0, 1, 3, 4 of one
// pair of dwords or bytes 2, 3, 5, 6 of the next.  The bytes read are pixels x0 + 16 x .. x0 + 16 x + 15 of the sensor
// row, whole groups and nothing else: inside the row's row_bytes whenever the crop lies inside `width`, so
// bank_sensor_valid_groups is the bounds proof for every form.  gb and shift are workgroup-uniform; as the constants
// 1, 0 (every kernel without a sensor argument) the function is the single load it always was.
__device__ __forceinline__ void crop_piece16(uint4 &v, const uint8_t *src, int y, int pitch, int x, int gb, int shift)
{
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    u32x4 r;
    if (gb == 1) {
        __builtin_memcpy(&r, src + (int64_t)y * pitch + x * 16, 16);
    } else if (gb == 2) {
        u32x4 a, b;
        const uint8_t *p = src + (int64_t)y * pitch + x * 32;
        __builtin_memcpy(&a, p, 16);
        __builtin_memcpy(&b, p + 16, 16);
        constexpr uint32_t sel = 0x06040200u;
        r = u32x4{__builtin_amdgcn_perm(a.y >> shift, a.x >> shift, sel), __builtin_amdgcn_perm(a.w >> shift, a.z >> shift, sel),
                  __builtin_amdgcn_perm(b.y >> shift, b.x >> shift, sel), __builtin_amdgcn_perm(b.w >> shift, b.z >> shift, sel)};
    } else if (gb == 5) {
        u32x4 a;
        uint32_t b;
        const uint8_t *p = src + (int64_t)y * pitch + x * 20;
        __builtin_memcpy(&a, p, 16);
        __builtin_memcpy(&b, p + 16, 4);
        r = u32x4{a.x, __builtin_amdgcn_alignbyte(a.z, a.y, 1u), __builtin_amdgcn_alignbyte(a.w, a.z, 2u),
                  __builtin_amdgcn_alignbyte(b, a.w, 3u)};
    } else {
        u32x4 a;
        u32x2 b;
        const uint8_t *p = src + (int64_t)y * pitch + x * 24;
        __builtin_memcpy(&a, p, 16);
        __builtin_memcpy(&b, p + 16, 8);
        r = u32x4{__builtin_amdgcn_perm(a.y, a.x, 0x04030100u), __builtin_amdgcn_perm(a.z, a.y, 0x06050302u),
                  __builtin_amdgcn_perm(b.x, a.w, 0x04030100u), __builtin_amdgcn_perm(b.y, b.x, 0x06050302u)};
    }
    __builtin_memcpy(&v, &r, 16);   // (one whole 16-byte value for every form)
}

// B rows of a binned piece: sensor rows B y .. B y + B - 1 of the 16 B pixels behind `row` (the first one's group),
// added into eight registers of two 16-bit sums each -- crop pixel 2 i in the low half of acc[i], 2 i + 1 in the high
// half.  A row is B grey pieces of crop_piece16 (B piece_bytes source bytes, the same unaligned loads and byte
// selection).  B = 2: a grey dword gives two horizontal pair sums, the halves box2 adds; B = 4: a grey dword is one crop
// pixel's four bytes of the row, v_sad_u8 against zero adds them to the low half, v_sad_hi_u8 to the high half.  The rows
// go one behind the other (not unrolled): a row's loads are all that is in flight, eight at the most (gb 2, B = 4).
template <int B>
__device__ __forceinline__ void binned_rows(uint32_t (&acc)[8], const uint8_t *row, int pitch, int gb, int shift)
{
    constexpr uint32_t m = 0x00FF00FFu;
#pragma unroll 1
    for (int j = 0; j < B; j++, row += pitch) {
#pragma unroll
        for (int q = 0; q < B; q++) {
            uint4 g;
            crop_piece16(g, row, 0, 0, q, gb, shift);
            if constexpr (B == 2) {
                acc[4 * q + 0] += (g.x & m) + ((g.x >> 8) & m);
                acc[4 * q + 1] += (g.y & m) + ((g.y >> 8) & m);
                acc[4 * q + 2] += (g.z & m) + ((g.z >> 8) & m);
                acc[4 * q + 3] += (g.w & m) + ((g.w >> 8) & m);
            } else {
                acc[2 * q] = __builtin_amdgcn_sad_hi_u8(g.y, 0u, byte_sum(g.x, acc[2 * q]));
                acc[2 * q + 1] = __builtin_amdgcn_sad_hi_u8(g.w, 0u, byte_sum(g.z, acc[2 * q + 1]));
            }
        }
    }
}

// crop_piece16 for a binned stream (bin 2 or 4, workgroup-uniform): pixels 16 x .. 16 x + 15 of row y of the BINNED crop,
// each (the sum of its bin x bin sensor pixels + bin^2 / 2) >> (2 log2 bin) -- one rounding of the whole sum, box2's for
// bin 2.  `src` is the first byte of sensor pixel (x0, y0)'s group.  The piece reads whole pixels x0 + 16 bin x .. x0 + 16 bin
// (x + 1) - 1 of rows y0 + bin y .. y0 + bin y + bin - 1: inside width and height whenever the footprint is, so
// bank_sensor_valid_groups (with its bin) is the bounds proof here too.
__device__ __forceinline__ void crop_piece16_binned(uint4 &v, const uint8_t *src, int y, int pitch, int x, int gb, int shift, int bin)
{
    uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint8_t *row = src + (int64_t)y * bin * pitch + (int64_t)x * (bin * piece_bytes(gb));
    uint32_t half, mean;
    if (bin == 2) { binned_rows<2>(acc, row, pitch, gb, shift); half = 0x00020002u; mean = 2; }
    else { binned_rows<4>(acc, row, pitch, gb, shift); half = 0x00080008u; mean = 4; }
#pragma unroll
    for (int i = 0; i < 8; i++) acc[i] = (acc[i] + half) >> mean;   // (bytes 0 and 2 are the two pixels; bytes 1, 3 are not looked at)
    v = make_uint4(__builtin_amdgcn_perm(acc[1], acc[0], 0x06040200u), __builtin_amdgcn_perm(acc[3], acc[2], 0x06040200u),
                   __builtin_amdgcn_perm(acc[5], acc[4], 0x06040200u), __builtin_amdgcn_perm(acc[7], acc[6], 0x06040200u));
}

// Piece x of row y of the window of source `c` behind `src`, binned or not (c.bin is uniform).
__device__ __forceinline__ void crop_piece(uint4 &v, const uint8_t *src, int y, int x, const CropSource &c)
{
    if (c.bin != 1) crop_piece16_binned(v, src, y, c.pitch, x, c.gb, c.shift, c.bin);
    else crop_piece16(v, src, y, c.pitch, x, c.gb, c.shift);
}

}  // namespace

}  // namespace aof
