"""Inputs and expected values of the packed-pixel tests (tests/test_bank_pixels_ref.py, tests/test_bank_pixels_abi.py,
tests/test_gpu_bank_pixels.py): the three 8- and 16-bit pixel formats of include/aof.h (AOF_PIXEL_*,
aof_set_bank_pixel_formats) and the layout tables of bank_sensors_ref with a format column.  The validity rule, the crop,
the layouts and the packer (whose other byte per packed pixel is seeded noise independent of the luma) are
crop_source_ref's.  Nothing here touches the GPU or the library under test."""
import bank_sensors_ref as sref
import crop_source_ref as csr

GREY8, LUMA16_LO, LUMA16_HI = 0, 1, 2
FORMATS = (GREY8, LUMA16_LO, LUMA16_HI)

# bank_sensors_ref.TABLES (the same sensors, residues mod 16, crop origins and order in the buffer) with the pitch in BYTES
# of the stream's format and the format as a last column.  Each configuration carries all three formats, a padded and an
# odd packed pitch, offsets with residues 0, 1, 7 and 8 mod 16, a crop that touches the right and bottom edges of a packed
# sensor, and as the buffer's last frame a LUMA16_HI one whose crop is the sensor: the buffer's last byte is a grey byte.
PITCH_AND_FORMAT = {
    "px4-64": [(192, LUMA16_LO), (176, LUMA16_HI), (128, LUMA16_HI), (263, LUMA16_LO), (320, GREY8)],
    "opencv-128": [(320, LUMA16_HI), (152, GREY8), (395, LUMA16_LO)],
}
ORDER = {"px4-64": [0, 1, 4, 3, 2], "opencv-128": [1, 0, 2]}     # (each ends with a packed frame)
TABLES = {cfg: ([(w, h, pitch, mod, origin, fmt) for (w, h, _, mod, origin), (pitch, fmt) in zip(sref.TABLES[cfg][0], PITCH_AND_FORMAT[cfg])],
                ORDER[cfg]) for cfg in sref.TABLES}


def bpp_of(fmt):
    """Bytes per pixel of one of FORMATS."""
    return csr.GROUPS[fmt][1]


def phase_of(fmt):
    """Which byte of a pixel of one of FORMATS holds its grey value."""
    return (csr.GROUPS[fmt][2] or 0) // 8


extent, layout, pack = csr.extent, sref.layout, csr.pack


def valid(rec, fmt, w, h, camera_bytes, base=0):
    """The rule (crop_source_ref.valid) as the packed tests write it: no bin."""
    return csr.valid(rec, fmt, 1, w, h, camera_bytes, base)


def crop(buffer, rec, fmt, w, h, base=0):
    """The w x h crop the record and its format mean, out of the flat uint8 buffer."""
    return csr.crop(buffer, rec, fmt, 1, w, h, base)


def retable(cfg, fmts):
    """TABLES[cfg]'s cameras with other formats: the grey pitch of bank_sensors_ref times the format's bytes per pixel."""
    table, order = TABLES[cfg]
    return [t[:2] + (g[2] * bpp_of(f),) + t[3:5] + (f,) for t, g, f in zip(table, sref.TABLES[cfg][0], fmts)], order


def grey_twin(table, order, w, h):
    """The grey sensor path's records for the same cameras: bank_sensors_ref's layout of the de-interleaved planes -- the
    same width, height, x0 and y0, the grey buffer's own pitch and offsets."""
    return sref.layout([t[:2] + (sref_pitch,) + t[3:5] for t, sref_pitch in zip(table, _grey_pitches(table))], order, w, h)


def _grey_pitches(table):
    # a grey plane's rows: the sensor's width, padded as bank_sensors_ref pads them (whatever the packed pitch is)
    by_size = {(t[0], t[1]): t[2] for cfg in sref.TABLES for t in sref.TABLES[cfg][0]}
    return [by_size[(t[0], t[1])] for t in table]
