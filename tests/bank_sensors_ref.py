"""Inputs and expected values of the per-stream sensor tests (tests/test_bank_sensors_ref.py, tests/test_bank_sensors_abi.py,
tests/test_gpu_bank_sensors.py): the layout tables of grey sensors of different sizes, pitches and alignments and the
48-tick case.  The record, the rule, the crop, the layout and the packer are crop_source_ref's, here in the grey tests'
spelling.  Nothing here touches the GPU or the library under test."""
import bank_cases
import bank_rig
import crop_source_ref as csr
from bank_rig import GATED, LIMITED

SENSOR_DTYPE, record, extent, pack = csr.SENSOR_DTYPE, csr.record, csr.extent, csr.pack
TICK_BAD_SENSOR = -5

# (cfg, S, seed) of the two configurations; tests/test_bank_sensors_ref.py asserts the census on the oracle's records
CASES = {"px4-64": (5, 71), "opencv-128": (3, 72)}
T = 48
INTERVAL = 200_000

# sensor width, height, pitch, offset mod 16, crop origin (None: the centre); the order in which the frames lie in the buffer
TABLES = {
    "px4-64": ([(96, 80, 96, 0, None),       # the aligned case: what aof_bank_sensor_from_camera gives
                (80, 72, 88, 8, (3, 5)),     # padded rows, x0 off a dword
                (64, 64, 64, 1, (0, 0)),     # crop == sensor; placed last: its last byte is the buffer's last valid byte
                (131, 70, 131, 7, (67, 6)),  # odd pitch, the crop touches the right and bottom edges
                (320, 240, 320, 0, None)],   # a large sensor between small ones
               [0, 1, 4, 3, 2]),
    "opencv-128": ([(160, 144, 160, 0, None),
                    (144, 136, 152, 8, (3, 5)),
                    (197, 134, 197, 7, (69, 6))],
                   [0, 1, 2]),
}
UNIFORM = {"px4-64": (96, 80), "opencv-128": (160, 144)}      # rig B: every stream's sensor, its crop at the centre
SCALARS = {"px4-64": (72, 66), "opencv-128": (136, 130)}      # what aof_bank_camera holds while records are bound: no stream's


def valid(rec, w, h, camera_bytes, base=0, fmt=0):
    """The rule (crop_source_ref.valid) as the grey tests write it: no bin, the format last."""
    return csr.valid(rec, fmt, 1, w, h, camera_bytes, base)


def crop(buffer, rec, w, h, base=0):
    """The w x h crop a grey record means, out of the flat uint8 buffer."""
    return csr.crop(buffer, rec, csr.GREY8, 1, w, h, base)


def layout(table, order, w, h, start=0):
    """crop_source_ref.layout: (records, bytes) of a grey table, (records, formats, bytes) of one with a format column."""
    recs, fmts, end = csr.layout(table, order, w, h, start=start)
    return (recs, fmts, end) if len(table[0]) > 5 else (recs, end)


_cases = {}


def case(aof, orc, synth, cfg, K=None):
    """(p, run, want, wire, due, after, derot) of a configuration: bank_ref.make_run's 48 ticks with the saturated patches
    of bank_camera_ref, the oracle chain's records and wire frames, the exposure gate and the de-rotated pairs, with the
    census asserted on the oracle's records (bank_cases.prepare).  K: a burstable run (a stream keeps its leading frames
    of every K rounds), without the census.  Computed once and left unchanged."""
    if (cfg, K) not in _cases:
        S, seed = CASES[cfg]
        p = bank_rig.params_of(aof, cfg)
        if K is None:
            _cases[(cfg, K)] = (p,) + bank_cases.prepare(aof, orc, synth, p, S, T, seed, INTERVAL, 15, False, True, LIMITED, GATED, True, True)
        else:
            import bank_camera_ref as cref
            import bank_ref as ref
            run = cref.add_saturated_patches(ref.make_run(synth, p.width, p.height, S, T, seed))
            _cases[(cfg, K)] = (p, bank_rig.burstable(run, K))
    return _cases[(cfg, K)]
