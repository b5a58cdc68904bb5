"""Python harness over the C ABI of the MI355X flow engine (include/aof.h).

The product is ``csrc/libaof.so`` (hand-written gfx950 kernels behind a plain C
ABI) and the C++ facade in ``facade/``; this module only binds the C ABI with
``ctypes`` so that tests and ``bench.py`` can drive it with device memory owned
by PyTorch.  It mirrors the reference's operator surface for the path --
``OpticalFlowPX4.calcFlow`` as called from
``/root/reference/src/mainloop.cpp:322`` -- in :class:`OpticalFlowPX4`.

There is no CPU fallback anywhere in this package: if ``libaof.so`` is missing
the import raises, and every compute entry point needs a gfx950 device.

The directory name contains a hyphen, so import it through
``__graft_entry__.load_package()`` (registers it as ``aero_optical_flow_amd``).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# AOF_LIB: load another build of the same ABI (A/B timing of two kernel builds on one box)
LIB_PATH = os.environ.get("AOF_LIB") or os.path.join(_HERE, "csrc", "libaof.so")

GRID_DENSE, GRID_PX4FLOW = 0, 1
SEARCH_EXHAUSTIVE, SEARCH_PRUNED, SEARCH_ADAPTIVE = 0, 1, 2
SAD_SKIPPED = 0xFFFF
FLAG_FLOW_VALID, FLAG_PRED_VALID = 1, 2
K_PYRAMID, K_SEARCH_L1, K_REDUCE_L1, K_SEARCH, K_REDUCE = range(5)

BLOCK_DTYPE = np.dtype([("dx", "i1"), ("dy", "i1"), ("sad", "<u2")])
FLOW_DTYPE = np.dtype([("flow_x", "<f4"), ("flow_y", "<f4"), ("count", "<u4"), ("quality", "u1"),
                       ("flags", "u1"), ("pred_x", "i1"), ("pred_y", "i1")])
assert BLOCK_DTYPE.itemsize == 4 and FLOW_DTYPE.itemsize == 16


class Params(C.Structure):
    """``aof_params`` (include/aof.h)."""
    _fields_ = [(n, C.c_int32) for n in (
        "width", "height", "tile", "search", "grid_mode", "num_blocks", "feature_threshold",
        "value_threshold", "subpixel", "hist_filter", "pyramid_levels", "mean_subtract",
        "min_valid")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class IngestParams(C.Structure):
    """``aof_ingest_params`` (include/aof.h)."""
    _fields_ = [(n, C.c_int32) for n in ("camera_width", "camera_height", "crop_width", "crop_height")]


class DerotateParams(C.Structure):
    """``aof_derotate_params`` (include/aof.h)."""
    _fields_ = [(n, C.c_float) for n in ("focal_x", "focal_y", "max_flow", "rate_threshold")]


GYRO_DTYPE = np.dtype([("integ_x", "<f4"), ("integ_y", "<f4"), ("integ_z", "<f4"), ("dt_s", "<f4")])


class SequenceParams(C.Structure):
    """``aof_sequence_params`` (include/aof.h)."""
    _fields_ = [("ingest", IngestParams), ("focal_x", C.c_float), ("focal_y", C.c_float),
                ("output_rate", C.c_int32), ("offset_timestamp_usec", C.c_uint64),
                ("system_id", C.c_uint8), ("component_id", C.c_uint8), ("first_seq", C.c_uint8),
                ("derotate", C.c_uint8), ("derotate_params", DerotateParams)]


class SeqLayout(C.Structure):
    """``aof_seq_layout`` (include/aof.h)."""
    _fields_ = [(n, C.c_size_t) for n in ("total_bytes", "cropped", "exposure", "flows", "derotated", "count",
                                          "records", "frames", "frame_len", "scratch")]


SEQ_RECORD_DTYPE = np.dtype([("frame", "<u4"), ("quality", "<i4"), ("dt_us", "<i4"), ("flow_x", "<f4"),
                             ("flow_y", "<f4"), ("gyro_x", "<f4"), ("gyro_y", "<f4"), ("gyro_z", "<f4")])
SEQ_FRAME_BYTES = 56
SEQ_STATUS_STALLED = 1
assert SEQ_RECORD_DTYPE.itemsize == 32


class BankParams(C.Structure):
    """``aof_bank_params`` (include/aof.h)."""
    _fields_ = [("n_streams", C.c_int32), ("frame_stride", C.c_int64), ("focal_x", C.c_float), ("focal_y", C.c_float),
                ("output_rate", C.c_int32), ("offset_timestamp_usec", C.c_uint64),
                ("system_id", C.c_uint8), ("component_id", C.c_uint8), ("first_seq", C.c_uint8)]


class BankStream(C.Structure):
    """``aof_bank_stream`` (include/aof.h): what belongs to one camera of a bank."""
    _fields_ = [("focal_x", C.c_float), ("focal_y", C.c_float), ("output_rate", C.c_int32),
                ("system_id", C.c_uint8), ("component_id", C.c_uint8), ("first_seq", C.c_uint8), ("reserved0", C.c_uint8),
                ("offset_timestamp_usec", C.c_uint64), ("reserved1", C.c_uint64)]


BANK_STREAM_DTYPE = np.dtype([("focal_x", "<f4"), ("focal_y", "<f4"), ("output_rate", "<i4"), ("system_id", "u1"),
                              ("component_id", "u1"), ("first_seq", "u1"), ("reserved0", "u1"),
                              ("offset_timestamp_usec", "<u8"), ("reserved1", "<u8")])                # aof_bank_stream
assert BANK_STREAM_DTYPE.itemsize == 32 and C.sizeof(BankStream) == 32


class BankSensor(C.Structure):
    """``aof_bank_sensor`` (include/aof.h): where one camera's frame lies in the camera buffer, and its crop."""
    _fields_ = [("offset", C.c_uint64), ("pitch", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("x0", C.c_int32), ("y0", C.c_int32), ("reserved", C.c_uint32)]


BANK_SENSOR_DTYPE = np.dtype([("offset", "<u8"), ("pitch", "<i4"), ("width", "<i4"), ("height", "<i4"), ("x0", "<i4"),
                              ("y0", "<i4"), ("reserved", "<u4")])                                   # aof_bank_sensor
assert BANK_SENSOR_DTYPE.itemsize == 32 and C.sizeof(BankSensor) == 32


# a node of a warp mesh (aof_warp_point): the sensor-plane coordinate of a crop pixel's centre in 1/32 pixel
WARP_POINT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4")])
WARP_CELL = 8
WARP_FRAC_BITS = 5
WARP_NONE = -2**31     # AOF_WARP_NONE in a mesh's first node's x: the stream is not warped


class Lens(C.Structure):
    """aof_lens: the sensor camera and its Brown-Conrady coefficients, and the virtual pinhole camera of the crop."""
    _fields_ = [(n, C.c_double) for n in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "out_fx", "out_fy", "out_cx", "out_cy")]


class BankLayout(C.Structure):
    """``struct aof_bank_layout`` (include/aof.h)."""
    _fields_ = [(n, C.c_size_t) for n in ("total_bytes", "frames", "state", "scratch")]


class BankCamera(C.Structure):
    """``aof_bank_camera`` (include/aof.h)."""
    _fields_ = [("ingest", IngestParams), ("camera_stride", C.c_int64), ("exposure_interval_us", C.c_uint32),
                ("derotate", C.c_uint8), ("derotate_params", DerotateParams)]


class BankBurst(C.Structure):
    """``aof_bank_burst`` (include/aof.h)."""
    _fields_ = [("n_rounds", C.c_int32), ("round_stride", C.c_int64)]


BANK_BURST_MAX = 16
TICK_HELD, TICK_IDLE = -1, -2
BANK_BIN_MAX = 4   # AOF_BANK_BIN_MAX: a stream's binning is 1, 2 or 4 (aof_set_bank_binning)
PIXEL_GREY8, PIXEL_LUMA16_LO, PIXEL_LUMA16_HI = 0, 1, 2   # AOF_PIXEL_*: a stream's pixel format (aof_set_bank_pixel_formats)
PIXEL_Y10, PIXEL_Y12, PIXEL_Y14, PIXEL_Y10P, PIXEL_Y12P = 4, 5, 6, 7, 8   # raw mono pixels: 16-bit words, MIPI-packed groups (3: no format)
TICK_BAD_SENSOR = -5   # the stream's sensor record (aof_bank_sensor) does not describe memory inside the camera buffer
TICK_DTYPE = np.dtype([("quality", "<i4"), ("dt_us", "<i4"), ("flow_x", "<f4"), ("flow_y", "<f4"),
                       ("gyro_x", "<f4"), ("gyro_y", "<f4"), ("gyro_z", "<f4"), ("frame", "<u4"), ("pixel", FLOW_DTYPE)])
BANK_STATE_BYTES = 64
EXPOSURE_DTYPE = np.dtype([("hist", "<u4", (10,)), ("msv", "<f4"), ("due", "<u4")])   # aof_exposure_record
assert TICK_DTYPE.itemsize == 48 and EXPOSURE_DTYPE.itemsize == 48


class ExposureControl(C.Structure):
    """``aof_exposure_control`` (include/aof.h): the constants of the auto-exposure controller."""
    _fields_ = [(n, C.c_float) for n in ("msv_target", "exposure_p", "exposure_i", "exposure_d", "gain_p", "gain_i", "gain_d",
                                         "exposure_change_threshold", "exposure_max", "gain_change_threshold", "gain_max")]


EXPOSURE_UPDATED, EXPOSURE_SET_EXPOSURE, EXPOSURE_SET_GAIN = 1, 2, 4
EXPOSURE_STATE_DTYPE = np.dtype([("msv_error_old", "<f4"), ("msv_error_int", "<f4"), ("exposure", "<u2"), ("gain", "u1"),
                                 ("reserved", "u1"), ("updates", "<u4")])                            # aof_exposure_state
EXPOSURE_COMMAND_DTYPE = np.dtype([("exposure", "<u2"), ("gain", "u1"), ("flags", "u1"), ("msv_error", "<f4"),
                                   ("msv_error_int", "<f4"), ("update", "<u4")])                     # aof_exposure_command
assert EXPOSURE_STATE_DTYPE.itemsize == 16 and EXPOSURE_COMMAND_DTYPE.itemsize == 16


class ImuParams(C.Structure):
    """``aof_imu_params`` (include/aof.h)."""
    _fields_ = [("n_streams", C.c_int32), ("n_rounds", C.c_int32), ("max_samples", C.c_int32),
                ("system_id", C.c_uint8), ("component_id", C.c_uint8), ("first_seq", C.c_uint8)]


IMU_SLOTS_MAX = 16
TICK_STALE_GYRO, TICK_NO_OFFSET = -3, -4
IMU_SAMPLE_DTYPE = np.dtype([("time_usec", "<u8"), ("xgyro", "<f4"), ("ygyro", "<f4"), ("zgyro", "<f4"),
                             ("reserved", "<u4")])                                                   # aof_imu_sample
IMU_STATE_DTYPE = np.dtype([("gyro_x", "<f8"), ("gyro_y", "<f8"), ("gyro_z", "<f8"), ("prev_time_usec", "<u8"),
                            ("last_taken_time_usec", "<u8"), ("offset_timestamp_usec", "<u8"), ("messages", "<u4"),
                            ("samples_integrated", "<u4"), ("samples_rejected", "<u4"), ("dropped", "<u4")])   # aof_imu_state
assert IMU_SAMPLE_DTYPE.itemsize == 24 and IMU_STATE_DTYPE.itemsize == 64


class MavlinkRxParams(C.Structure):
    """``aof_mavlink_rx_params`` (include/aof.h)."""
    _fields_ = [("n_streams", C.c_int32), ("n_rounds", C.c_int32), ("max_bytes", C.c_int32), ("max_samples", C.c_int32)]


MAVLINK_RX_BYTES_MAX = 4096
MAVLINK_RX_STATE_DTYPE = np.dtype([("bytes", "<u8"), ("frames", "<u4"), ("imu_samples", "<u4"), ("bad_check", "<u4"),
                                   ("overflowed", "<u4"), ("skipped", "<u4"), ("rejected_flags", "<u4"),
                                   ("in_progress", "u1", (96,))])                                   # aof_mavlink_rx_state
assert MAVLINK_RX_STATE_DTYPE.itemsize == 128


class FieldParams(C.Structure):
    """``aof_field_params`` (include/aof.h)."""
    _fields_ = [("min_blocks", C.c_int32), ("passes", C.c_int32), ("exclude_reach", C.c_int32), ("gate_px", C.c_float)]


FIELD_VALID, FIELD_REFIT = 1, 2
FIELD_DTYPE = np.dtype([("det", "<i8"), ("num_zoom", "<i8"), ("num_rot", "<i8"), ("accepted", "<u4"), ("at_reach", "<u4"),
                        ("fitted", "<u4"), ("used", "<u4"), ("zoom", "<f4"), ("rotation", "<f4"), ("centre_x", "<f4"),
                        ("centre_y", "<f4"), ("flags", "<u4"), ("reserved", "<u4")])   # aof_field
assert FIELD_DTYPE.itemsize == 64


class OutboxLayout(C.Structure):
    """``struct aof_outbox_layout`` (include/aof.h)."""
    _fields_ = [(n, C.c_size_t) for n in ("total_bytes", "messages", "exposures")]


OUTBOX_HEADER_DTYPE = np.dtype([("tag", "<u8"), ("n_messages", "<u4"), ("messages_found", "<u4"), ("n_exposures", "<u4"),
                                ("exposures_found", "<u4"), ("reserved", "u1", (40,))])            # aof_outbox_header
OUTBOX_ENTRY_DTYPE = np.dtype([("stream", "<u4"), ("round", "<u2"), ("mavlink_len", "u1"), ("reserved0", "u1"),
                               ("mavlink", "u1", (SEQ_FRAME_BYTES,)), ("record", TICK_DTYPE), ("derotated", "<f4", (2,)),
                               ("reserved1", "u1", (8,))])                                           # aof_outbox_entry
OUTBOX_EXPOSURE_DTYPE = np.dtype([("stream", "<u4"), ("round", "<u2"), ("reserved0", "<u2"), ("exposure", EXPOSURE_DTYPE),
                                  ("reserved1", "u1", (8,))])                                        # aof_outbox_exposure
assert OUTBOX_HEADER_DTYPE.itemsize == 64 and OUTBOX_ENTRY_DTYPE.itemsize == 128 and OUTBOX_EXPOSURE_DTYPE.itemsize == 64


class WsLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in (
        "total_bytes", "sums", "l1_prev", "l1_cur", "l1_blocks", "l1_subdirs", "l1_flows",
        "l0_blocks", "l0_subdirs", "l0_hist", "l1_hist", "hints")]


class StreamStats(C.Structure):
    """``aof_stream_stats`` (include/aof.h)."""
    _fields_ = [("calls", C.c_uint64), ("resident_served", C.c_uint64), ("resident_launches", C.c_uint32),
                ("resident_fallbacks", C.c_uint32), ("resident_lost", C.c_uint32), ("tagged_slow", C.c_uint32),
                ("launch_call_us_max", C.c_float), ("start_latency_us_max", C.c_float),
                ("last_report", C.c_char * 320)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["last_report"] = d["last_report"].decode(errors="replace")
        return d


class SearchStats(C.Structure):
    """``aof_search_stats`` (include/aof.h): what the ADAPTIVE search mode of an 8x8 context has done so far."""
    _fields_ = [("pruned_launches", C.c_uint64), ("exhaustive_launches", C.c_uint64), ("reports_read", C.c_uint64),
                ("belief", C.c_int32), ("paying_pct", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class AofError(RuntimeError):
    def __init__(self, code, text):
        super().__init__(f"aof error {code}: {text}")
        self.code = code


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    try:  # share torch's HIP runtime instance when torch is in the process
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the facade
        pass
    lib = C.CDLL(LIB_PATH)
    P, VP, I64 = C.POINTER, C.c_void_p, C.c_int64
    sig = {
        "aof_version": (C.c_int, []),
        "aof_strerror": (C.c_char_p, [C.c_int]),
        "aof_params_default": (C.c_int, [P(Params), C.c_int, C.c_int]),
        "aof_params_px4flow": (C.c_int, [P(Params), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "aof_params_check": (C.c_int, [P(Params)]),
        "aof_grid": (C.c_int, [P(Params), C.c_int] + [P(C.c_int32)] * 6),
        "aof_workspace_layout": (C.c_int, [P(Params), I64, P(WsLayout)]),
        "aof_create": (C.c_int, [P(Params), C.c_int, P(VP)]),
        "aof_destroy": (None, [VP]),
        "aof_last_error": (C.c_char_p, [VP]),
        "aof_get_params": (C.c_int, [VP, P(Params)]),
        "aof_search_variant": (C.c_char_p, [VP]),
        "aof_set_force_generic": (C.c_int, [VP, C.c_int]),
        "aof_set_search_mode": (C.c_int, [VP, C.c_int]),
        "aof_get_search_mode": (C.c_int, [VP]),
        "aof_get_search_stats": (C.c_int, [VP, VP]),
        "aof_set_search_belief": (C.c_int, [VP, C.c_int]),
        "aof_set_split_coarse": (C.c_int, [VP, C.c_int]),
        "aof_set_reduce_fusion": (C.c_int, [VP, C.c_int]),
        "aof_flow_batch_device": (C.c_int, [VP, VP, VP, I64, I64, VP, VP, VP, VP, C.c_size_t, VP]),
        "aof_flow_pair_host": (C.c_int, [VP, VP, VP, VP, VP, VP]),
        "aof_stream_push_host": (C.c_int, [VP, VP, VP]),
        "aof_stream_reset": (C.c_int, [VP]),
        "aof_set_stream_graph": (C.c_int, [VP, C.c_int]),
        "aof_set_stream_resident": (C.c_int, [VP, C.c_int]),
        "aof_stream_get_stats": (C.c_int, [VP, P(StreamStats)]),
        "aof_debug_resident_fault": (C.c_int, [VP, C.c_int, C.c_uint32]),
        "aof_set_vote_deadline_us": (C.c_int, [VP, C.c_uint32]),
        "aof_debug_vote_deadline_ticks": (C.c_int, [VP, C.c_uint32]),
        "aof_debug_tile16_verdicts": (C.c_int, [VP, VP, C.c_int]),
        "aof_ingest_batch_device": (C.c_int, [P(IngestParams), VP, I64, I64, VP, I64, VP, VP]),
        "aof_sequence_layout": (C.c_int, [P(Params), P(SequenceParams), I64, P(SeqLayout)]),
        "aof_sequence_device": (C.c_int, [VP, P(SequenceParams), VP, I64, I64, VP, VP, VP, C.c_size_t, VP]),
        "aof_flow_angle": (C.c_float, [C.c_float, C.c_float]),
        "aof_bank_layout": (C.c_int, [P(Params), P(BankParams), P(BankLayout)]),
        "aof_bank_reset_device": (C.c_int, [VP, P(BankParams), VP, VP, C.c_size_t, VP]),
        "aof_bank_push_device": (C.c_int, [VP, P(BankParams), VP, VP, VP, VP, VP, C.c_size_t, VP, VP, VP, VP]),
        "aof_set_bank_path": (C.c_int, [VP, C.c_int]),
        "aof_bank_last_path": (C.c_int, [VP]),
        "aof_bank_stream_from_params": (C.c_int, [P(BankParams), P(BankStream)]),
        "aof_set_bank_streams": (C.c_int, [VP, VP, C.c_int32]),
        "aof_set_bank_sensors": (C.c_int, [VP, VP, C.c_int32, C.c_uint64]),
        "aof_bank_sensor_from_camera": (C.c_int, [P(Params), P(BankCamera), C.c_int32, P(BankSensor)]),
        "aof_bank_sensor_centred": (C.c_int, [P(Params), C.c_uint64, C.c_int32, C.c_int32, C.c_int32, P(BankSensor)]),
        "aof_bank_sensor_valid": (C.c_int, [P(BankSensor), C.c_int32, C.c_int32, C.c_uint64, C.c_uint64]),
        "aof_ingest_sensors_device": (C.c_int, [C.c_int32, C.c_int32, VP, C.c_uint64, VP, I64, VP, I64, VP, VP, VP]),
        "aof_set_bank_pixel_formats": (C.c_int, [VP, VP, C.c_int32]),
        "aof_bank_sensor_valid_format": (C.c_int, [P(BankSensor), C.c_uint8, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64]),
        "aof_ingest_sensor_formats_device": (C.c_int, [C.c_int32, C.c_int32, VP, C.c_uint64, VP, VP, I64, VP, I64, VP, VP, VP]),
        "aof_set_bank_binning": (C.c_int, [VP, VP, C.c_int32]),
        "aof_bank_sensor_valid_binned": (C.c_int, [P(BankSensor), C.c_uint8, C.c_uint8, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64]),
        "aof_bank_sensor_centred_binned": (C.c_int, [P(Params), C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_uint8, C.c_uint8,
                                                     P(BankSensor)]),
        "aof_ingest_sensors_binned_device": (C.c_int, [C.c_int32, C.c_int32, VP, C.c_uint64, VP, VP, VP, I64, VP, I64, VP, VP, VP]),
        "aof_bank_pixel_row_bytes": (C.c_int, [C.c_uint8, C.c_int32, P(C.c_int64)]),
        "aof_warp_mesh_size": (C.c_int, [P(Params), P(C.c_int32), P(C.c_int32)]),
        "aof_warp_mesh_identity": (C.c_int, [P(Params), C.c_int32, C.c_int32, VP]),
        "aof_warp_mesh_from_lens": (C.c_int, [P(Params), P(Lens), VP]),
        "aof_set_bank_warps": (C.c_int, [VP, VP, C.c_int32]),
        "aof_bank_warp_one_launch": (C.c_int, [P(Params), P(C.c_int64)]),
        "aof_bank_warp_crossover": (C.c_int, []),
        "aof_ingest_warped_device": (C.c_int, [C.c_int32, C.c_int32, VP, C.c_uint64, VP, VP, VP, I64, VP, I64, VP, VP, VP]),
        "aof_warp_host": (C.c_int, [C.c_int32, C.c_int32, VP, C.c_uint64, P(BankSensor), C.c_uint8, VP, VP, VP]),
        "aof_bank_camera_layout": (C.c_int, [P(Params), P(BankParams), P(BankCamera), P(BankLayout), P(C.c_size_t)]),
        "aof_bank_push_camera_device": (C.c_int, [VP, P(BankParams), P(BankCamera), VP, VP, VP, VP, VP, C.c_size_t, VP, VP, VP,
                                                  VP, VP, VP]),
        "aof_bank_push_burst_device": (C.c_int, [VP, P(BankParams), P(BankBurst), VP, VP, VP, VP, VP, C.c_size_t, VP, VP, VP, VP]),
        "aof_bank_push_camera_burst_device": (C.c_int, [VP, P(BankParams), P(BankCamera), P(BankBurst), VP, VP, VP, VP, VP,
                                                        C.c_size_t, VP, VP, VP, VP, VP, VP]),
        "aof_outbox_layout": (C.c_int, [C.c_uint32, C.c_uint32, P(OutboxLayout)]),
        "aof_bank_collect_device": (C.c_int, [VP, C.c_int32, C.c_int32, VP, VP, VP, VP, VP, C.c_uint32, C.c_uint32, VP,
                                              C.c_size_t, C.c_uint64, VP, VP]),
        "aof_outbox_alloc_host": (C.c_int, [C.c_size_t, P(VP)]),
        "aof_outbox_free_host": (C.c_int, [VP]),
        "aof_exposure_control_default": (C.c_int, [P(ExposureControl)]),
        "aof_bank_exposure_reset_device": (C.c_int, [VP, C.c_int32, VP, C.c_uint16, C.c_uint8, VP, VP, VP, VP]),
        "aof_bank_exposure_control_device": (C.c_int, [VP, P(ExposureControl), C.c_int32, C.c_int32, VP, VP, VP, VP]),
        "aof_exposure_control_host": (C.c_int, [P(ExposureControl), C.c_int32, C.c_int32, VP, VP, VP]),
        "aof_bank_imu_reset_device": (C.c_int, [VP, C.c_int32, VP, C.c_uint64, VP, VP]),
        "aof_bank_imu_device": (C.c_int, [VP, P(ImuParams), VP, VP, VP, VP, VP, VP, VP, VP, VP]),
        "aof_bank_imu_host": (C.c_int, [P(ImuParams), VP, VP, VP, VP, VP, VP, VP, VP]),
        "aof_bank_mavlink_rx_reset_device": (C.c_int, [VP, C.c_int32, VP, VP, VP]),
        "aof_bank_mavlink_rx_device": (C.c_int, [VP, P(MavlinkRxParams), VP, VP, VP, VP, VP, VP]),
        "aof_bank_mavlink_rx_host": (C.c_int, [P(MavlinkRxParams), VP, VP, VP, VP, VP]),
        "aof_field_params_default": (C.c_int, [P(FieldParams)]),
        "aof_field_supported": (C.c_int, [P(Params)]),
        "aof_field_batch_device": (C.c_int, [VP, P(FieldParams), VP, VP, VP, I64, VP, VP]),
        "aof_field_host": (C.c_int, [P(Params), P(FieldParams), VP, VP, VP, I64, VP]),
        "aof_derotate_batch_device": (C.c_int, [P(DerotateParams), VP, VP, I64, VP, VP]),
        "aof_exposure_msv": (C.c_float, [VP]),
        "aof_exposure_bin": (C.c_int, [C.c_int]),
        "aof_set_profiling": (C.c_int, [VP, C.c_int]),
        "aof_set_profiling_mask": (C.c_int, [VP, C.c_uint32]),
        "aof_kernel_ms": (C.c_int, [VP, C.c_int, P(C.c_float)]),
        "aof_profile_count": (C.c_int, [VP, C.c_int]),
        "aof_profile_ms": (C.c_int, [VP, C.c_int, C.c_int, P(C.c_float)]),
    }
    for name, (res, args) in sig.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if os.environ.get("AOF_LIB"):   # A/B timing against an older build of the ABI
                continue
            raise
        fn.restype, fn.argtypes = res, args
    return lib, tuple(sig)


lib, EXPORTS = _load()


def default_params(width, height, **overrides) -> Params:
    p = Params()
    lib.aof_params_default(C.byref(p), width, height)
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, int(v))
    return p


def px4flow_params(width, height, search=4, feature_threshold=30, value_threshold=3000,
                   **overrides) -> Params:
    p = Params()
    lib.aof_params_px4flow(C.byref(p), width, height, search, feature_threshold, value_threshold)
    for k, v in overrides.items():
        setattr(p, k, int(v))
    return p


def check_params(p: Params) -> int:
    return lib.aof_params_check(C.byref(p))


def grid(p: Params, level=0):
    """(x0, y0, step_x, step_y, nx, ny) of a pyramid level."""
    v = [C.c_int32() for _ in range(6)]
    rc = lib.aof_grid(C.byref(p), level, *[C.byref(x) for x in v])
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return tuple(x.value for x in v)


def workspace_layout(p: Params, n_pairs: int) -> WsLayout:
    L = WsLayout()
    rc = lib.aof_workspace_layout(C.byref(p), n_pairs, C.byref(L))
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return L


def algorithmic_bytes(p: Params) -> int:
    """Compulsory HBM bytes per frame pair:
    read both frames once, write 4 B per block and the 16 B result."""
    _, _, _, _, nx, ny = grid(p, 0)
    return 2 * p.width * p.height + 4 * nx * ny + 16


def abs_diffs(p: Params) -> int:
    _, _, _, _, nx, ny = grid(p, 0)
    return nx * ny * (2 * p.search + 1) ** 2 * p.tile ** 2


def ingest_batch(camera, crop_w, crop_h, cropped=None, hist=None, want_hist=True):
    """Frame ingest on the device (centre crop + 10-bin exposure histogram; the caller-side
    steps of /root/reference/src/mainloop.cpp:295-298,203-214).  camera: uint8 CUDA tensor
    [n, cam_h, cam_w].  Returns (cropped [n, crop_h, crop_w], hist [n, 10] int32-as-uint32)."""
    import torch
    n, cam_h, cam_w = camera.shape
    p = IngestParams(cam_w, cam_h, crop_w, crop_h)
    if cropped is None:
        cropped = torch.empty((n, crop_h, crop_w), dtype=torch.uint8, device=camera.device)
    if hist is None and want_hist:
        hist = torch.empty((n, 10), dtype=torch.int32, device=camera.device)
    stream = torch.cuda.current_stream(camera.device).cuda_stream
    rc = lib.aof_ingest_batch_device(C.byref(p), camera.data_ptr(), camera.stride(0), n,
                                     cropped.data_ptr(), cropped.stride(0) if n else crop_w * crop_h,
                                     hist.data_ptr() if hist is not None else None, stream)
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return cropped, hist


def derotate_batch(flows, gyro, focal_x, focal_y, max_flow, rate_threshold):
    """Published PX4Flow gyro compensation of a batch of flow records on the device.
    flows: uint8 CUDA tensor [n, 16] (aof_flow records); gyro: float32 CUDA tensor [n, 4]
    (integ_x, integ_y, integ_z, dt_s).  Returns float32 [n, 2]."""
    import torch
    n = flows.shape[0]
    out = torch.empty((n, 2), dtype=torch.float32, device=flows.device)
    p = DerotateParams(focal_x, focal_y, max_flow, rate_threshold)
    rc = lib.aof_derotate_batch_device(C.byref(p), flows.data_ptr(), gyro.data_ptr(), n, out.data_ptr(),
                                       torch.cuda.current_stream(flows.device).cuda_stream)
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return out


def flow_angle(flow_px: float, focal_px: float) -> float:
    """Pixel flow -> angular flow (rad): the fixed-operation atan2 of include/aof_math.h."""
    return float(lib.aof_flow_angle(flow_px, focal_px))


def sequence_params(cam_w, cam_h, crop_w, crop_h, focal_x=216.6677, focal_y=216.2457, output_rate=15,
                    offset_timestamp_usec=0, system_id=1, component_id=100, first_seq=0, derotate=None) -> SequenceParams:
    """``aof_sequence_params``; derotate: None or (max_flow, rate_threshold) of the gyro compensation."""
    sp = SequenceParams()
    sp.ingest = IngestParams(cam_w, cam_h, crop_w, crop_h)
    sp.focal_x, sp.focal_y, sp.output_rate = focal_x, focal_y, output_rate
    sp.offset_timestamp_usec = offset_timestamp_usec
    sp.system_id, sp.component_id, sp.first_seq = system_id, component_id, first_seq & 0xFF
    sp.derotate = 0 if derotate is None else 1
    if derotate is not None:
        sp.derotate_params = DerotateParams(focal_x, focal_y, derotate[0], derotate[1])
    return sp


def sequence_layout(p: Params, sp: SequenceParams, n_frames: int) -> SeqLayout:
    L = SeqLayout()
    rc = lib.aof_sequence_layout(C.byref(p), C.byref(sp), n_frames, C.byref(L))
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return L


def bank_params(n_streams, focal_x=216.6677, focal_y=216.2457, output_rate=15, offset_timestamp_usec=0, system_id=1,
                component_id=100, first_seq=0, frame_stride=0) -> BankParams:
    """``aof_bank_params`` of a bank of ``n_streams`` live streams (frame_stride 0: frames back to back)."""
    bp = BankParams()
    bp.n_streams, bp.frame_stride = n_streams, frame_stride
    bp.focal_x, bp.focal_y, bp.output_rate = focal_x, focal_y, output_rate
    bp.offset_timestamp_usec = offset_timestamp_usec
    bp.system_id, bp.component_id, bp.first_seq = system_id, component_id, first_seq & 0xFF
    return bp


def bank_stream_from_params(bp: BankParams, n=None):
    """aof_bank_stream_from_params: the ``aof_bank_stream`` record the scalars of ``bp`` mean, as a numpy record of
    BANK_STREAM_DTYPE -- or, with ``n``, an array of n copies of it (the start of a per-stream table)."""
    rec = BankStream()
    rc = lib.aof_bank_stream_from_params(C.byref(bp), C.byref(rec))
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    one = np.frombuffer(bytes(rec), dtype=BANK_STREAM_DTYPE)[0]
    return one if n is None else np.full(int(n), one, dtype=BANK_STREAM_DTYPE)


def _sensor_record(rec: BankSensor):
    return np.frombuffer(bytes(rec), dtype=BANK_SENSOR_DTYPE)[0]


def bank_sensor_from_camera(p: Params, cam: BankCamera, stream=None, n=None):
    """aof_bank_sensor_from_camera: the ``aof_bank_sensor`` record the scalars of ``cam`` mean for stream ``stream``, as a
    numpy record of BANK_SENSOR_DTYPE -- or, with ``n``, the array of the records of streams 0..n-1 (binding it changes
    no byte of a camera push)."""
    def one(s):
        rec = BankSensor()
        rc = lib.aof_bank_sensor_from_camera(C.byref(p), C.byref(cam), int(s), C.byref(rec))
        if rc:
            raise AofError(rc, lib.aof_strerror(rc).decode())
        return _sensor_record(rec)
    if n is None:
        return one(stream or 0)
    return np.array([one(s) for s in range(int(n))], dtype=BANK_SENSOR_DTYPE)


def bank_sensor_centred(p: Params, offset, pitch, width, height, format=0, bin=1):
    """aof_bank_sensor_centred / aof_bank_sensor_centred_binned: the record of a frame of width x height, rows ``pitch``
    bytes apart, ``offset`` bytes into the camera buffer, with the crop at the centre (the reference's rule); with a pixel
    format (PIXEL_*) or a bin (1, 2, 4): the footprint of the binned crop at the centre, checked by the kernels' rule."""
    rec = BankSensor()
    if format == 0 and bin == 1:
        rc = lib.aof_bank_sensor_centred(C.byref(p), int(offset), int(pitch), int(width), int(height), C.byref(rec))
    else:
        rc = lib.aof_bank_sensor_centred_binned(C.byref(p), int(offset), int(pitch), int(width), int(height), int(format) & 0xFF,
                                                int(bin) & 0xFF, C.byref(rec))
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return _sensor_record(rec)


def bank_pixel_row_bytes(format, width) -> int:
    """aof_bank_pixel_row_bytes: the bytes of a row of ``width`` pixels of ``format`` (PIXEL_*), (width / G) * Bg.  AofError
    (-EINVAL) for a value that is no format, width < 1 or a width that is not whole groups."""
    out = C.c_int64(0)
    rc = lib.aof_bank_pixel_row_bytes(int(format) & 0xFF, int(width), C.byref(out))
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return int(out.value)


def bank_sensor_valid(rec, crop_w, crop_h, camera_bytes, base=0, format=0, bin=1) -> bool:
    """aof_bank_sensor_valid / _valid_format / _valid_binned: the kernels' validity rule on one BANK_SENSOR_DTYPE record of
    pixel format ``format`` (PIXEL_*) and binning ``bin`` (a byte: 1, 2, 4 are bins), compiled for the host."""
    r = BankSensor.from_buffer_copy(np.asarray(rec, dtype=BANK_SENSOR_DTYPE).tobytes())
    if bin != 1:
        rc = lib.aof_bank_sensor_valid_binned(C.byref(r), int(format) & 0xFF, int(bin) & 0xFF, int(crop_w), int(crop_h), int(base),
                                              int(camera_bytes))
    elif format == 0:
        rc = lib.aof_bank_sensor_valid(C.byref(r), int(crop_w), int(crop_h), int(base), int(camera_bytes))
    else:
        rc = lib.aof_bank_sensor_valid_format(C.byref(r), int(format) & 0xFF, int(crop_w), int(crop_h), int(base), int(camera_bytes))
    if rc < 0:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return bool(rc)


def ingest_sensors(camera, sensors, crop_w, crop_h, camera_bytes=None, cropped=None, hist=None, ok=None, want_cropped=True,
                   want_hist=True, want_ok=True, formats=None, bins=None):
    """aof_ingest_sensors_device: frame ingest on the device for frames that sensor records describe.  camera: uint8 CUDA
    tensor (any shape; the records' offsets count from its first byte); sensors: uint8 CUDA tensor of n * 32 bytes
    (BANK_SENSOR_DTYPE, 16-byte aligned); camera_bytes: bytes of ``camera`` the kernel may read (default: all).
    formats: None, or a uint8 CUDA tensor of n pixel formats (PIXEL_*; aof_ingest_sensor_formats_device).  bins: None, or
    a uint8 CUDA tensor of n bins (1, 2, 4; aof_ingest_sensors_binned_device): crop_w x crop_h is the binned crop.  Returns
    (cropped [n, crop_h, crop_w], hist [n, 10] int32, ok [n] uint8), None where not wanted."""
    import torch
    assert camera.dtype == torch.uint8 and sensors.dtype == torch.uint8 and sensors.is_contiguous() and sensors.numel() % 32 == 0
    n = sensors.numel() // 32
    assert formats is None or (formats.dtype == torch.uint8 and formats.is_contiguous() and formats.numel() == n)
    assert bins is None or (bins.dtype == torch.uint8 and bins.is_contiguous() and bins.numel() == n)
    dev = camera.device
    if cropped is None and want_cropped:
        cropped = torch.empty((n, crop_h, crop_w), dtype=torch.uint8, device=dev)
    if hist is None and want_hist:
        hist = torch.empty((n, 10), dtype=torch.int32, device=dev)
    if ok is None and want_ok:
        ok = torch.empty((n,), dtype=torch.uint8, device=dev)
    opt = lambda t: t.data_ptr() if t is not None else None
    tail = (n, opt(cropped), cropped.stride(0) if cropped is not None and n else crop_w * crop_h, opt(hist), opt(ok),
            torch.cuda.current_stream(dev).cuda_stream)
    head = (int(crop_w), int(crop_h), camera.data_ptr(), camera.numel() if camera_bytes is None else int(camera_bytes), sensors.data_ptr())
    if bins is not None:
        rc = lib.aof_ingest_sensors_binned_device(*head, opt(formats), bins.data_ptr(), *tail)
    elif formats is None:
        rc = lib.aof_ingest_sensors_device(*head, *tail)
    else:
        rc = lib.aof_ingest_sensor_formats_device(*head, formats.data_ptr(), *tail)
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return cropped, hist, ok


def warp_mesh_size(p: Params):
    """aof_warp_mesh_size: (nx, ny), the nodes of the mesh of p.width x p.height -- one every WARP_CELL crop pixels."""
    nx, ny = C.c_int32(0), C.c_int32(0)
    rc = lib.aof_warp_mesh_size(C.byref(p), C.byref(nx), C.byref(ny))
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return int(nx.value), int(ny.value)


def warp_mesh_identity(p: Params, x0, y0) -> np.ndarray:
    """aof_warp_mesh_identity: the mesh [ny, nx] (WARP_POINT_DTYPE) that gives the plain crop at (x0, y0) byte for byte."""
    nx, ny = warp_mesh_size(p)
    out = np.zeros((ny, nx), WARP_POINT_DTYPE)
    rc = lib.aof_warp_mesh_identity(C.byref(p), int(x0), int(y0), out.ctypes.data)
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return out


def warp_mesh_from_lens(p: Params, fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, out_fx=None, out_fy=None, out_cx=None,
                        out_cy=None) -> np.ndarray:
    """aof_warp_mesh_from_lens: the mesh [ny, nx] of a Brown-Conrady lens (fx, fy, cx, cy in plane pixels) seen by the
    virtual pinhole camera out_* of the crop (default: the same focal lengths, the principal point at the crop's
    centre).  The caller binds out_fx, out_fy as the stream's focal lengths."""
    lens = Lens(fx, fy, cx, cy, k1, k2, p1, p2, k3, fx if out_fx is None else out_fx, fy if out_fy is None else out_fy,
                p.width / 2.0 if out_cx is None else out_cx, p.height / 2.0 if out_cy is None else out_cy)
    nx, ny = warp_mesh_size(p)
    out = np.zeros((ny, nx), WARP_POINT_DTYPE)
    rc = lib.aof_warp_mesh_from_lens(C.byref(p), C.byref(lens), out.ctypes.data)
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return out


def bank_warp_one_launch(p: Params):
    """aof_bank_warp_one_launch: (ok, lds_bytes) -- can a camera push of configuration p with warps bound run as one launch
    per round, and the dynamic LDS a workgroup of it would ask for (the one-workgroup plan's bytes plus 8 nx ny)."""
    lds = C.c_int64(0)
    rc = lib.aof_bank_warp_one_launch(C.byref(p), C.byref(lds))
    if rc < 0:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return bool(rc), int(lds.value)


def bank_warp_crossover() -> int:
    """aof_bank_warp_crossover: the largest n_streams at which set_bank_path(0) takes the one-launch kernel with warps
    bound (0: never; path 1 still does)."""
    return int(lib.aof_bank_warp_crossover())


def warp_host(camera, rec, crop_w, crop_h, mesh, format=0, camera_bytes=None):
    """aof_warp_host: one frame in host memory through its mesh, by the header the kernel compiles.  camera: a flat uint8
    array; rec: a BANK_SENSOR_DTYPE record; mesh: [ny, nx] of WARP_POINT_DTYPE.  Returns (crop [crop_h, crop_w] uint8,
    hist [10] uint32), or None where the record is not valid."""
    camera = np.ascontiguousarray(camera, np.uint8).reshape(-1)
    mesh = np.ascontiguousarray(mesh, WARP_POINT_DTYPE)
    r = BankSensor.from_buffer_copy(np.asarray(rec, dtype=BANK_SENSOR_DTYPE).tobytes())
    crop, hist = np.zeros((int(crop_h), int(crop_w)), np.uint8), np.zeros(10, np.uint32)
    rc = lib.aof_warp_host(int(crop_w), int(crop_h), camera.ctypes.data, camera.size if camera_bytes is None else int(camera_bytes),
                           C.byref(r), int(format) & 0xFF, mesh.ctypes.data, crop.ctypes.data, hist.ctypes.data)
    if rc < 0:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return (crop, hist) if rc else None


def ingest_warped(camera, sensors, points, crop_w, crop_h, camera_bytes=None, cropped=None, hist=None, ok=None, want_cropped=True,
                  want_hist=True, want_ok=True, formats=None):
    """aof_ingest_warped_device: ingest_sensors with frame i resampled through mesh i.  points: uint8 CUDA tensor of
    n * ny * nx * 8 bytes (WARP_POINT_DTYPE nodes, 16-byte aligned).  Returns (cropped, hist, ok) as ingest_sensors does."""
    import torch
    assert camera.dtype == torch.uint8 and sensors.dtype == torch.uint8 and sensors.is_contiguous() and sensors.numel() % 32 == 0
    assert points.dtype == torch.uint8 and points.is_contiguous()
    n = sensors.numel() // 32
    assert formats is None or (formats.dtype == torch.uint8 and formats.is_contiguous() and formats.numel() == n)
    nodes = ((int(crop_w) + 7) // 8 + 1) * ((int(crop_h) + 7) // 8 + 1)
    assert points.numel() >= n * nodes * 8
    dev = camera.device
    if cropped is None and want_cropped:
        cropped = torch.empty((n, crop_h, crop_w), dtype=torch.uint8, device=dev)
    if hist is None and want_hist:
        hist = torch.empty((n, 10), dtype=torch.int32, device=dev)
    if ok is None and want_ok:
        ok = torch.empty((n,), dtype=torch.uint8, device=dev)
    opt = lambda t: t.data_ptr() if t is not None else None
    rc = lib.aof_ingest_warped_device(int(crop_w), int(crop_h), camera.data_ptr(), camera.numel() if camera_bytes is None else int(camera_bytes),
                                      sensors.data_ptr(), opt(formats), points.data_ptr(), n, opt(cropped),
                                      cropped.stride(0) if cropped is not None and n else crop_w * crop_h, opt(hist), opt(ok),
                                      torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return cropped, hist, ok


def bank_layout(p: Params, bp: BankParams) -> BankLayout:
    L = BankLayout()
    rc = lib.aof_bank_layout(C.byref(p), C.byref(bp), C.byref(L))
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return L


def bank_camera_params(cam_w, cam_h, crop_w, crop_h, camera_stride=0, exposure_interval_us=200000, derotate=None,
                       focal_x=216.6677, focal_y=216.2457) -> BankCamera:
    """``aof_bank_camera``: sensor size -> centre crop; derotate: None or (max_flow, rate_threshold) of the gyro
    compensation; exposure_interval_us: mainloop.cpp:274 (0 = statistics with every frame)."""
    cam = BankCamera()
    cam.ingest = IngestParams(cam_w, cam_h, crop_w, crop_h)
    cam.camera_stride, cam.exposure_interval_us = camera_stride, exposure_interval_us
    cam.derotate = 0 if derotate is None else 1
    if derotate is not None:
        cam.derotate_params = DerotateParams(focal_x, focal_y, derotate[0], derotate[1])
    return cam


def bank_burst_params(n_rounds, round_stride=0) -> BankBurst:
    """``aof_bank_burst``: K frame rounds per call; round_stride 0: the rounds lie back to back."""
    b = BankBurst()
    b.n_rounds, b.round_stride = int(n_rounds), int(round_stride)
    return b


def bank_camera_layout(p: Params, bp: BankParams, cam: BankCamera):
    """(``BankLayout``, offset of the staging region) of a bank that serves ``bank_push_camera``."""
    L, staging = BankLayout(), C.c_size_t()
    rc = lib.aof_bank_camera_layout(C.byref(p), C.byref(bp), C.byref(cam), C.byref(L), C.byref(staging))
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return L, staging.value


def outbox_layout(capacity_messages, capacity_exposures=0) -> OutboxLayout:
    """``aof_outbox_layout``: byte offsets of the two entry lists behind the 64-byte header, and the outbox's size."""
    L = OutboxLayout()
    rc = lib.aof_outbox_layout(capacity_messages, capacity_exposures, C.byref(L))
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return L


def outbox_view(buffer, capacity_messages=None, capacity_exposures=0):
    """(header, messages, exposures) of an outbox as structured numpy views: the header (OUTBOX_HEADER_DTYPE, a 0-d
    array), its n_messages stored entries (OUTBOX_ENTRY_DTYPE) and its n_exposures stored exposure entries
    (OUTBOX_EXPOSURE_DTYPE).  buffer: a uint8 tensor or array, or a HostOutbox (then a view of the pinned memory itself,
    not a copy).  capacity_messages None: what is left of the buffer beside capacity_exposures exposure entries."""
    if isinstance(buffer, HostOutbox):
        capacity_messages, capacity_exposures, a = buffer.capacity_messages, buffer.capacity_exposures, buffer.array
    else:
        a = buffer.cpu().numpy() if hasattr(buffer, "cpu") else np.asarray(buffer)
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    if capacity_messages is None:
        capacity_messages = (a.size - 64 - 64 * capacity_exposures) // 128
    L = outbox_layout(capacity_messages, capacity_exposures)
    assert a.size >= L.total_bytes, (a.size, L.total_bytes)
    header = a[:64].view(OUTBOX_HEADER_DTYPE).reshape(())
    messages = a[L.messages:L.messages + 128 * capacity_messages].view(OUTBOX_ENTRY_DTYPE)[:int(header["n_messages"])]
    exposures = a[L.exposures:L.exposures + 64 * capacity_exposures].view(OUTBOX_EXPOSURE_DTYPE)[:int(header["n_exposures"])]
    return header, messages, exposures


class HostOutbox:
    """An outbox in pinned, coherent, device-mapped host memory (``aof_outbox_alloc_host``): ``bank_collect`` writes it
    from the device and the host polls its tag, without any stream synchronisation.  ``array`` is a numpy uint8 view of
    the memory itself; ``ptr`` is its address, valid on both sides.  Needs a current HIP device."""

    def __init__(self, capacity_messages, capacity_exposures=0):
        self.capacity_messages, self.capacity_exposures = int(capacity_messages), int(capacity_exposures)
        self.layout = outbox_layout(self.capacity_messages, self.capacity_exposures)
        self.nbytes = self.layout.total_bytes
        p = C.c_void_p()
        rc = lib.aof_outbox_alloc_host(self.nbytes, C.byref(p))
        if rc:
            raise AofError(rc, "aof_outbox_alloc_host failed")
        self.ptr = p.value
        self.array = np.frombuffer((C.c_uint8 * self.nbytes).from_address(self.ptr), dtype=np.uint8)
        self._tag = self.array[:8].view("<u8")

    @property
    def tag(self) -> int:
        """The header's tag as the memory holds it now."""
        return int(self._tag[0])

    def wait(self, tag, timeout_s=2.0) -> bool:
        """Polls for ``tag`` until the deadline; False when it ran out.  Never blocks on the device."""
        import time
        deadline = time.perf_counter() + timeout_s
        tagword, tag = self._tag, int(tag)
        while int(tagword[0]) != tag:
            if time.perf_counter() > deadline:
                return False
        return True

    def close(self):
        """Frees the memory: only once the work that writes it has drained.  The views die with it."""
        if getattr(self, "ptr", None) and lib is not None:
            self.array = self._tag = None
            lib.aof_outbox_free_host(self.ptr)
            self.ptr = None

    __del__ = close


def exposure_control_default() -> ExposureControl:
    """``aof_exposure_control_default``: the reference's constants (mainloop.cpp:53-63)."""
    ec = ExposureControl()
    rc = lib.aof_exposure_control_default(C.byref(ec))
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return ec


def exposure_control_host(records, states, ec: ExposureControl = None):
    """``aof_exposure_control_host``: the controller on host memory, no device.  records: EXPOSURE_DTYPE [S] or [K, S];
    states: EXPOSURE_STATE_DTYPE [S], contiguous, updated IN PLACE.  Returns the commands (EXPOSURE_COMMAND_DTYPE, the
    shape of records)."""
    ec = exposure_control_default() if ec is None else ec
    records = np.ascontiguousarray(records, dtype=EXPOSURE_DTYPE)
    assert records.ndim in (1, 2)
    K, S = (1, records.shape[0]) if records.ndim == 1 else records.shape
    assert states.dtype == EXPOSURE_STATE_DTYPE and states.shape == (S,) and states.flags.c_contiguous and states.flags.writeable
    commands = np.empty(records.shape, EXPOSURE_COMMAND_DTYPE)
    rc = lib.aof_exposure_control_host(C.byref(ec), S, K, records.ctypes.data, states.ctypes.data, commands.ctypes.data)
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return commands


def imu_params(n_streams, n_rounds, max_samples, system_id=1, component_id=100, first_seq=0) -> ImuParams:
    ip = ImuParams()
    ip.n_streams, ip.n_rounds, ip.max_samples = int(n_streams), int(n_rounds), int(max_samples)
    ip.system_id, ip.component_id, ip.first_seq = int(system_id), int(component_id), int(first_seq)
    return ip


def bank_imu_host(samples, counts, times, records, states, system_id=1, component_id=100, first_seq=0, mavlink=True,
                  records_out=None, fill=0):
    """``aof_bank_imu_host``: the IMU call on host memory, no device.  samples: IMU_SAMPLE_DTYPE [K, M, S]; counts:
    uint8 [K, S] or None (M everywhere); times: uint64 [K, S]; records: TICK_DTYPE [K, S], what a push wrote; states:
    IMU_STATE_DTYPE [S], contiguous, updated IN PLACE.  records_out: a TICK_DTYPE [K, S] array to write (`records`
    itself for the in-place form) or None (a new one).  Returns (records_out, frames uint8 [K, S, 56] -- bytes nobody
    wrote keep `fill` --, lengths uint8 [K, S]); frames and lengths are None with mavlink=False."""
    samples = np.ascontiguousarray(samples, dtype=IMU_SAMPLE_DTYPE)
    K, M, S = samples.shape
    times = np.ascontiguousarray(times, dtype=np.uint64)
    assert records.dtype == TICK_DTYPE and records.shape == (K, S) and records.flags.c_contiguous and times.shape == (K, S)
    assert states.dtype == IMU_STATE_DTYPE and states.shape == (S,) and states.flags.c_contiguous and states.flags.writeable
    if counts is not None:
        counts = np.ascontiguousarray(counts, dtype=np.uint8)
        assert counts.shape == (K, S)
    if records_out is None:
        records_out = np.empty((K, S), TICK_DTYPE)
    assert records_out.dtype == TICK_DTYPE and records_out.shape == (K, S) and records_out.flags.c_contiguous
    frames = np.full((K, S, SEQ_FRAME_BYTES), fill, np.uint8) if mavlink else None
    lengths = np.full((K, S), fill, np.uint8) if mavlink else None
    ip = imu_params(S, K, M, system_id, component_id, first_seq)
    rc = lib.aof_bank_imu_host(C.byref(ip), samples.ctypes.data, counts.ctypes.data if counts is not None else None,
                               times.ctypes.data, records.ctypes.data, states.ctypes.data, records_out.ctypes.data,
                               frames.ctypes.data if mavlink else None, lengths.ctypes.data if mavlink else None)
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return records_out, frames, lengths


def imu_states_view(t) -> np.ndarray:
    """uint8 tensor/array [S, 64] of ``aof_imu_state`` -> structured numpy view [S]."""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(IMU_STATE_DTYPE).reshape(a.shape[:-1])


def mavlink_rx_params(n_streams, n_rounds, max_bytes, max_samples) -> MavlinkRxParams:
    rp = MavlinkRxParams()
    rp.n_streams, rp.n_rounds, rp.max_bytes, rp.max_samples = int(n_streams), int(n_rounds), int(max_bytes), int(max_samples)
    return rp


def _aligned_copy(a, align=16):
    """A C-contiguous copy of uint8 array `a` whose first byte lies at a multiple of `align`."""
    raw = np.empty(a.size + align, np.uint8)
    off = -raw.ctypes.data % align
    out = raw[off:off + a.size].reshape(a.shape)
    out[...] = a
    return out


def bank_mavlink_rx_host(data, lengths, states, max_samples, samples=None, counts=None):
    """``aof_bank_mavlink_rx_host``: the MAVLink receive on host memory, no device.  data: uint8 [K, S, B], what stream
    s received for round k in its first lengths[k, s] bytes; lengths: uint16 [K, S] or None (B everywhere); states:
    MAVLINK_RX_STATE_DTYPE [S], contiguous, updated IN PLACE; samples: an IMU_SAMPLE_DTYPE [K, M, S] array to write
    (slots at and behind a count keep what they hold) or None (a new one, zero-filled); counts likewise, uint8 [K, S].
    Returns (samples, counts)."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    K, S, B = data.shape
    M = int(max_samples)
    if data.ctypes.data % 16:
        data = _aligned_copy(data)
    if lengths is not None:
        lengths = np.ascontiguousarray(lengths, dtype=np.uint16)
        assert lengths.shape == (K, S)
    assert states.dtype == MAVLINK_RX_STATE_DTYPE and states.shape == (S,) and states.flags.c_contiguous and states.flags.writeable
    if samples is None:
        samples = np.zeros((K, M, S), IMU_SAMPLE_DTYPE)
    if counts is None:
        counts = np.zeros((K, S), np.uint8)
    assert samples.dtype == IMU_SAMPLE_DTYPE and samples.shape == (K, M, S) and samples.flags.c_contiguous
    assert counts.dtype == np.uint8 and counts.shape == (K, S) and counts.flags.c_contiguous
    rp = mavlink_rx_params(S, K, B, M)
    rc = lib.aof_bank_mavlink_rx_host(C.byref(rp), data.ctypes.data, lengths.ctypes.data if lengths is not None else None,
                                      states.ctypes.data, samples.ctypes.data, counts.ctypes.data)
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return samples, counts


def mavlink_rx_states_view(t) -> np.ndarray:
    """uint8 tensor/array [S, 128] of ``aof_mavlink_rx_state`` -> structured numpy view [S]."""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(MAVLINK_RX_STATE_DTYPE).reshape(a.shape[:-1])


def field_params(min_blocks=None, passes=None, exclude_reach=None, gate_px=None) -> FieldParams:
    """``aof_field_params_default`` (8 blocks, two passes, blocks at reach left out, a gate of 1 px), with overrides."""
    fp = FieldParams()
    lib.aof_field_params_default(C.byref(fp))
    for k, v in (("min_blocks", min_blocks), ("passes", passes), ("exclude_reach", exclude_reach)):
        if v is not None:
            setattr(fp, k, int(v))
    if gate_px is not None:
        fp.gate_px = float(gate_px)
    return fp


def field_supported(p: Params) -> bool:
    """``aof_field_supported``: does the motion-field fit serve the level-0 grid of `p`?"""
    return lib.aof_field_supported(C.byref(p)) == 0


def field_host(p: Params, blocks, flows, subdirs=None, params: FieldParams = None) -> np.ndarray:
    """``aof_field_host``: the motion-field fit on host memory, no device.  blocks: BLOCK_DTYPE (or uint32) [n, nb];
    flows: FLOW_DTYPE [n]; subdirs: uint8 [n, nb] or None.  Returns FIELD_DTYPE [n]."""
    blocks = np.ascontiguousarray(blocks)
    assert blocks.dtype.itemsize == 4 and blocks.ndim == 2
    n, nb = blocks.shape
    flows = np.ascontiguousarray(flows, dtype=FLOW_DTYPE).reshape(n)
    if subdirs is not None:
        subdirs = np.ascontiguousarray(subdirs, dtype=np.uint8)
        assert subdirs.shape == (n, nb)
    g = grid(p, 0)
    assert nb == g[4] * g[5], (nb, g)
    out = np.zeros(n, FIELD_DTYPE)
    fp = params if params is not None else field_params()
    rc = lib.aof_field_host(C.byref(p), C.byref(fp), blocks.ctypes.data, subdirs.ctypes.data if subdirs is not None else None,
                            flows.ctypes.data, n, out.ctypes.data)
    if rc:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return out


def fields_view(t) -> np.ndarray:
    """uint8 tensor/array [n, 64] of ``aof_field`` -> structured numpy view [n]."""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(FIELD_DTYPE).reshape(a.shape[:-1])


def exposure_states_view(t) -> np.ndarray:
    """uint8 tensor/array [S, 16] of ``aof_exposure_state`` -> structured numpy view [S]."""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(EXPOSURE_STATE_DTYPE).reshape(a.shape[:-1])


def exposure_commands_view(t) -> np.ndarray:
    """uint8 tensor/array [.., 16] of ``aof_exposure_command`` -> structured numpy view [..]."""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(EXPOSURE_COMMAND_DTYPE).reshape(a.shape[:-1])


def exposure_view(t) -> np.ndarray:
    """uint8 tensor/array [S, 48] of ``aof_exposure_record`` -> structured numpy view [S]."""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(EXPOSURE_DTYPE).reshape(a.shape[0])


def ticks_view(t) -> np.ndarray:
    """uint8 tensor/array [S, 48] of ``aof_tick_record`` -> structured numpy view [S]."""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(TICK_DTYPE).reshape(a.shape[0])


class Bank:
    """A stream bank in device memory (``FlowEngine.bank_create``): the buffer, its parameters and its layout."""

    def __init__(self, bp: BankParams, layout: BankLayout, buffer, camera: BankCamera = None, staging: int = None):
        self.bp, self.layout, self.buffer = bp, layout, buffer
        self.camera, self.staging = camera, staging     # (a bank made for bank_push_camera: its staging region's offset)

    @property
    def n_streams(self) -> int:
        return self.bp.n_streams

    def frames_bytes(self) -> np.ndarray:
        """Host copy of the bank's ``frames`` region (up to the state records)."""
        return self.buffer[self.layout.frames:self.layout.state].cpu().numpy()

    def state_bytes(self) -> np.ndarray:
        """Host copy of the bank's ``state`` region: [S, 64] bytes."""
        L = self.layout
        return self.buffer[L.state:L.state + BANK_STATE_BYTES * self.n_streams].cpu().numpy().reshape(self.n_streams, BANK_STATE_BYTES)


def exposure_msv(hist) -> float:
    h = np.ascontiguousarray(np.asarray(hist), dtype=np.uint32)
    assert h.shape == (10,)
    return float(lib.aof_exposure_msv(h.ctypes.data))


class FlowEngine:
    """One ``aof_ctx``: the batched, device-resident hot path."""

    def __init__(self, params: Params, device: int = 0):
        self._ctx = C.c_void_p()
        rc = lib.aof_create(C.byref(params), device, C.byref(self._ctx))
        if rc:
            self._ctx = None
            raise AofError(rc, lib.aof_strerror(rc).decode())
        self.params = params
        self.device = device
        self._ws = None

    def close(self):
        if getattr(self, "_ctx", None) and lib is not None:  # lib is None at interpreter shutdown
            lib.aof_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    def _check(self, rc):
        if rc < 0:
            raise AofError(rc, lib.aof_last_error(self._ctx).decode())
        return rc

    @property
    def variant(self) -> str:
        return lib.aof_search_variant(self._ctx).decode()

    def force_generic(self, on=True):
        self._check(lib.aof_set_force_generic(self._ctx, int(on)))

    def set_search_mode(self, mode):
        """SEARCH_ADAPTIVE (the default of every context: exact pruning where it pays -- 16x16 tiles by a probe per
        pair, 8x8 tiles by what the context's previous launches reported), SEARCH_EXHAUSTIVE (every candidate summed
        completely: the data-independent rate) or SEARCH_PRUNED (exact pruning always: rate depends on the images).
        All three write the same records."""
        self._check(lib.aof_set_search_mode(self._ctx, int(mode)))

    @property
    def search_mode(self) -> int:
        return lib.aof_get_search_mode(self._ctx)

    def search_stats(self) -> dict:
        """Launch counters and current verdict of the ADAPTIVE 8x8 search (``aof_search_stats``)."""
        st = SearchStats()
        self._check(lib.aof_get_search_stats(self._ctx, C.byref(st)))
        return st.as_dict()

    def set_search_belief(self, belief):
        """Tell an ADAPTIVE 8x8 context what to assume about its images before it has launched anything:
        1 pruning pays, 0 it does not, -1 forget (``aof_set_search_belief``)."""
        self._check(lib.aof_set_search_belief(self._ctx, int(belief)))

    def set_split_coarse(self, on=True):
        """Two-level batches: run K1 / level-1 search / level-1 reduce as separate kernels (fills the
        workspace's level-1 frames) instead of the fused coarse kernel."""
        self._check(lib.aof_set_split_coarse(self._ctx, int(on)))

    def set_reduce_fusion(self, on=True):
        """8x8 tiles on large grids: on=True reduces inside the search launch (opt-in); the default
        (on=False) launches K3 as a separate kernel behind the search."""
        if not hasattr(lib, "aof_set_reduce_fusion"):
            return   # (AOF_LIB pointing at an older build)
        self._check(lib.aof_set_reduce_fusion(self._ctx, int(on)))

    def set_profiling(self, on=True, kernels=None):
        """Time every kernel (kernels=None) or only the given kernel ids with HIP events."""
        if on and kernels is not None:
            mask = 0
            for k in kernels:
                mask |= 1 << k
            self._check(lib.aof_set_profiling_mask(self._ctx, mask))
        else:
            self._check(lib.aof_set_profiling(self._ctx, int(on)))

    def kernel_ms(self, kernel_id) -> float:
        ms = C.c_float()
        self._check(lib.aof_kernel_ms(self._ctx, kernel_id, C.byref(ms)))
        return ms.value

    def profile_ms(self, kernel_id):
        """Durations (ms) of the launches of one kernel timed since profiling was enabled
        (at most the last AOF_PROFILE_RING); synchronises on their events."""
        n = self._check(lib.aof_profile_count(self._ctx, kernel_id))
        out = []
        ms = C.c_float()
        for i in range(n):
            self._check(lib.aof_profile_ms(self._ctx, kernel_id, i, C.byref(ms)))
            out.append(ms.value)
        return out

    def grid(self, level=0):
        return grid(self.params, level)

    def nblocks(self, level=0):
        g = self.grid(level)
        return g[4] * g[5]

    # -- device-resident batch ------------------------------------------------
    def flow_batch(self, prev, cur, blocks=None, subdirs=None, flows=None, workspace=None,
                   pair_stride=None, n_pairs=None):
        """prev/cur: uint8 CUDA tensors [n, H, W] (or any layout described by
        pair_stride).  Returns (blocks [n, nb] int32-viewed records, flows [n, 16] bytes,
        workspace).  Everything is enqueued on torch's current stream."""
        import torch
        p = self.params
        if n_pairs is None:
            n_pairs = prev.shape[0]
        if pair_stride is None:
            pair_stride = prev.stride(0) if prev.dim() == 3 else p.width * p.height
        dev = prev.device
        nb = self.nblocks(0)
        if blocks is None:
            blocks = torch.empty((n_pairs, nb), dtype=torch.int32, device=dev)
        if flows is None:
            flows = torch.empty((n_pairs, 16), dtype=torch.uint8, device=dev)
        if subdirs is None and p.subpixel:
            subdirs = torch.empty((n_pairs, nb), dtype=torch.uint8, device=dev)
        L = workspace_layout(p, n_pairs)
        if workspace is None:
            if self._ws is None or self._ws.numel() < L.total_bytes or self._ws.device != dev:
                self._ws = torch.empty(L.total_bytes, dtype=torch.uint8, device=dev)
            workspace = self._ws
        stream = torch.cuda.current_stream(dev).cuda_stream
        self._check(lib.aof_flow_batch_device(
            self._ctx, prev.data_ptr(), cur.data_ptr(), pair_stride, n_pairs, blocks.data_ptr(),
            subdirs.data_ptr() if subdirs is not None else None, flows.data_ptr(),
            workspace.data_ptr(), workspace.numel(), stream))
        return blocks, flows, workspace

    def field_batch(self, blocks, flows, subdirs=None, fields=None, params: FieldParams = None, stream=None):
        """aof_field_batch_device behind flow_batch: blocks [n, nb] int32-viewed records, flows [n, 16] bytes, subdirs uint8
        [n, nb] or None, all CUDA tensors as flow_batch returns them.  fields: a uint8 tensor [n, 64] to write or None (a new
        one; read it with fields_view()).  Enqueued on torch's current stream, or on `stream` (a hipStream_t value)."""
        import torch
        n, nb = blocks.shape
        assert blocks.dtype == torch.int32 and blocks.is_contiguous() and nb == self.nblocks(0)
        assert flows.dtype == torch.uint8 and flows.is_contiguous() and flows.numel() == 16 * n
        assert subdirs is None or (subdirs.dtype == torch.uint8 and subdirs.is_contiguous() and tuple(subdirs.shape) == (n, nb))
        if fields is None:
            fields = torch.empty((n, 64), dtype=torch.uint8, device=blocks.device)
        assert fields.dtype == torch.uint8 and fields.is_contiguous() and fields.numel() == 64 * n
        fp = params if params is not None else field_params()
        if stream is None:
            stream = torch.cuda.current_stream(blocks.device).cuda_stream
        self._check(lib.aof_field_batch_device(self._ctx, C.byref(fp), blocks.data_ptr(), subdirs.data_ptr() if subdirs is not None else None,
                                               flows.data_ptr(), n, fields.data_ptr(), stream))
        return fields

    def bind_batch(self, prev, cur, blocks, flows, workspace, subdirs=None, stream=None):
        """flow_batch with every argument resolved once: returns a callable that enqueues the same
        batch on torch's current stream (or on `stream`, a hipStream_t value) with ONE ctypes call (a step of 128 VGA pairs takes 35 us on
        the device; flow_batch's own argument handling takes about as long on the host)."""
        import torch
        p = self.params
        n_pairs = prev.shape[0]
        stride = prev.stride(0) if prev.dim() == 3 else p.width * p.height
        assert workspace.numel() >= workspace_layout(p, n_pairs).total_bytes
        args = (self._ctx, prev.data_ptr(), cur.data_ptr(), stride, n_pairs, blocks.data_ptr(),
                subdirs.data_ptr() if subdirs is not None else None, flows.data_ptr(),
                workspace.data_ptr(), workspace.numel())
        keep = (prev, cur, blocks, flows, workspace, subdirs)
        fn, dev, current_stream = lib.aof_flow_batch_device, prev.device, torch.cuda.current_stream

        if stream is not None:   # a fixed hipStream_t (0 = the default stream)
            def enqueue():
                rc = fn(*args, stream)
                if rc < 0:
                    self._check(rc)
        else:
            def enqueue():
                rc = fn(*args, current_stream(dev).cuda_stream)
                if rc < 0:
                    self._check(rc)
        enqueue.keep = keep
        return enqueue

    # -- a recorded frame sequence as one device pipeline -------------------------------
    def sequence(self, sp: SequenceParams, camera, time_us, gyro=None, workspace=None):
        """aof_sequence_device: camera uint8 CUDA tensor [n, cam_h, cam_w]; time_us int64 CUDA tensor [n]
        (microseconds relative to the first frame); gyro float32 CUDA tensor [n, 4] (integ_x, integ_y,
        integ_z, dt_s of the interval that ends at frame k) or None.  Everything is enqueued on torch's
        current stream.  Returns (workspace, layout): read the outputs with sequence_outputs()."""
        import torch
        n = camera.shape[0]
        L = sequence_layout(self.params, sp, n)
        if workspace is None:
            workspace = torch.empty(L.total_bytes, dtype=torch.uint8, device=camera.device)
        assert time_us.dtype == torch.int64 and time_us.numel() == n
        stream = torch.cuda.current_stream(camera.device).cuda_stream
        self._check(lib.aof_sequence_device(self._ctx, C.byref(sp), camera.data_ptr(), camera.stride(0) if n else 0, n,
                                            time_us.data_ptr(), gyro.data_ptr() if gyro is not None else None,
                                            workspace.data_ptr(), workspace.numel(), stream))
        return workspace, L

    def sequence_outputs(self, sp: SequenceParams, workspace, L: SeqLayout, n: int):
        """Host views of what a (completed) sequence() call left in its workspace."""
        p = self.params
        ws = workspace.cpu().numpy()
        pairs = max(n - 1, 0)
        count = ws[L.count:L.count + 16].view(np.uint32)
        out = {
            "records": ws[L.records:L.records + 32 * int(count[0])].view(SEQ_RECORD_DTYPE),
            "frames_sent": int(count[1]), "status": int(count[2]),
            "cropped": ws[L.cropped:L.cropped + n * p.width * p.height].reshape(n, p.height, p.width),
            "exposure": ws[L.exposure:L.exposure + 40 * n].view(np.uint32).reshape(n, 10),
            "flows": ws[L.flows:L.flows + 16 * pairs].view(FLOW_DTYPE),
            "derotated": ws[L.derotated:L.derotated + 8 * pairs].view(np.float32).reshape(pairs, 2) if sp.derotate else None,
        }
        lens = ws[L.frame_len:L.frame_len + int(count[0])]
        out["mavlink"] = [bytes(ws[L.frames + SEQ_FRAME_BYTES * m:L.frames + SEQ_FRAME_BYTES * m + int(lens[m])])
                          for m in range(int(count[0]))]
        return out

    # -- a bank of live streams: many cameras per tick --------------------------------
    def bank_create(self, bp: BankParams, device=None, camera: BankCamera = None) -> "Bank":
        """Allocates a bank for ``bp.n_streams`` streams as a (zeroed) torch buffer and resets it.  camera: the bank is
        sized by aof_bank_camera_layout and serves bank_push_camera (and bank_push)."""
        import torch
        staging = None
        if camera is None:
            L = bank_layout(self.params, bp)
        else:
            L, staging = bank_camera_layout(self.params, bp, camera)
        dev = torch.device("cuda", self.device) if device is None else device
        bank = Bank(bp, L, torch.zeros(L.total_bytes, dtype=torch.uint8, device=dev), camera, staging)
        self.bank_reset(bank)
        return bank

    def bank_reset(self, bank: "Bank", mask=None):
        """aof_bank_reset_device: mask uint8 CUDA tensor [S] (non-zero = reset) or None (all streams)."""
        import torch
        buf = bank.buffer
        assert mask is None or (mask.dtype == torch.uint8 and mask.numel() == bank.n_streams and mask.is_contiguous())
        self._check(lib.aof_bank_reset_device(self._ctx, C.byref(bank.bp), mask.data_ptr() if mask is not None else None,
                                              buf.data_ptr(), buf.numel(), torch.cuda.current_stream(buf.device).cuda_stream))

    def _bank_push(self, bank, src, times, select, gyro, mavlink, records, out_frames, out_lengths, n_rounds=None,
                   round_stride=0, camera=False, exposure=None, derotated=None, want_exposure=True):
        """The one push behind bank_push, bank_push_camera, bank_push_burst and bank_push_camera_burst: the assertions,
        the outputs (with a leading [K] for a burst: n_rounds is not None) and the one call into the library.  select:
        `active` of a tick, `count` of a burst.  Returns every output tensor (None where not written)."""
        import torch
        S, buf, cam = bank.n_streams, bank.buffer, bank.camera
        burst = n_rounds is not None
        lead = (int(n_rounds), S) if burst else (S,)
        n = int(n_rounds) * S if burst else S
        dev = buf.device
        if camera:
            assert cam is not None, "bank_create(..., camera=...) makes a bank for sensor frames"
        assert src.dtype == torch.uint8 and (camera or src.is_contiguous())
        assert times.dtype == torch.int64 and times.numel() == n and (not burst or times.is_contiguous())
        if burst:
            assert select is None or (select.dtype == torch.uint8 and select.numel() == S)
            assert gyro is None or gyro.numel() == n * 4
        if records is None:
            records = torch.empty(lead + (48,), dtype=torch.uint8, device=dev)
        if camera and exposure is None and want_exposure:
            exposure = torch.empty(lead + (48,), dtype=torch.uint8, device=dev)
        if camera and derotated is None and cam.derotate:
            derotated = torch.empty(lead + (2,), dtype=torch.float32, device=dev)
        if mavlink:
            if out_frames is None:
                out_frames = torch.zeros(lead + (SEQ_FRAME_BYTES,), dtype=torch.uint8, device=dev)
            if out_lengths is None:
                out_lengths = torch.zeros(lead, dtype=torch.uint8, device=dev)
        else:
            out_frames = out_lengths = None
        opt = lambda t: t.data_ptr() if t is not None else None
        fn = getattr(lib, "aof_bank_push" + ("_camera" if camera else "") + ("_burst" if burst else "") + "_device")
        args = [self._ctx, C.byref(bank.bp)]
        if camera:
            args.append(C.byref(cam))
        if burst:
            args.append(C.byref(bank_burst_params(int(n_rounds), round_stride)))
        args += [src.data_ptr(), times.data_ptr(), opt(select), opt(gyro), buf.data_ptr(), buf.numel(), records.data_ptr()]
        if camera:
            args += [opt(exposure), opt(derotated)]
        self._check(fn(*args, opt(out_frames), opt(out_lengths), torch.cuda.current_stream(dev).cuda_stream))
        return dict(records=records, exposure=exposure, derotated=derotated, frames=out_frames, lengths=out_lengths)

    def bank_push(self, bank: "Bank", frames, times, active=None, gyro=None, mavlink=False, records=None, out_frames=None,
                  out_lengths=None):
        """aof_bank_push_device, one tick: frames uint8 CUDA tensor [S, H, W] (stream s at s * frame_stride bytes);
        times int64 CUDA tensor [S] (microseconds); active uint8 [S] or None (all); gyro float32 [S, 4] or None.
        Everything is enqueued on torch's current stream.  Returns the record tensor [S, 48] (read it with
        ticks_view()), and with mavlink=True (records, frames [S, 56], lengths [S])."""
        out = self._bank_push(bank, frames, times, active, gyro, mavlink, records, out_frames, out_lengths)
        return (out["records"], out["frames"], out["lengths"]) if mavlink else out["records"]

    def bank_push_camera(self, bank: "Bank", camera, times, active=None, gyro=None, mavlink=False, records=None,
                         exposure=None, derotated=None, out_frames=None, out_lengths=None, want_exposure=True):
        """aof_bank_push_camera_device, one tick on raw sensor frames: camera uint8 CUDA tensor, stream s's sensor frame
        at s * camera_stride bytes (no alignment needed); the rest as bank_push.  exposure: uint8 [S, 48] (read it with
        exposure_view()), allocated unless want_exposure is False (then no statistics, the gate does not move);
        derotated: float32 [S, 2], allocated when the bank's camera parameters ask for de-rotation.  Returns a dict of
        the output tensors: records, exposure, derotated, frames, lengths (None where not written)."""
        return self._bank_push(bank, camera, times, active, gyro, mavlink, records, out_frames, out_lengths, camera=True,
                               exposure=exposure, derotated=derotated, want_exposure=want_exposure)

    def bank_push_burst(self, bank: "Bank", n_rounds, frames, times, count=None, gyro=None, mavlink=False, records=None,
                        out_frames=None, out_lengths=None, round_stride=0):
        """aof_bank_push_burst_device, K = n_rounds frame rounds in one call: frames uint8 CUDA tensor, stream s's frame
        of round k at k * round_stride + s * frame_stride bytes (round_stride 0: the rounds back to back); times int64
        [K, S]; count uint8 [S] (stream s has frames in rounds 0..count[s]-1) or None (all K); gyro float32 [K, S, 4] or
        None.  Returns the record tensor [K, S, 48] (ticks_view() of round k: records[k]), and with mavlink=True
        (records, frames [K, S, 56], lengths [K, S])."""
        out = self._bank_push(bank, frames, times, count, gyro, mavlink, records, out_frames, out_lengths, n_rounds, round_stride)
        return (out["records"], out["frames"], out["lengths"]) if mavlink else out["records"]

    def bank_push_camera_burst(self, bank: "Bank", n_rounds, camera, times, count=None, gyro=None, mavlink=False,
                               records=None, exposure=None, derotated=None, out_frames=None, out_lengths=None,
                               want_exposure=True, round_stride=0):
        """aof_bank_push_camera_burst_device, K = n_rounds rounds of raw sensor frames in one call: camera uint8 CUDA
        tensor, stream s's sensor frame of round k at k * round_stride + s * camera_stride bytes; the rest as
        bank_push_burst and bank_push_camera, every output with a leading [K].  Returns a dict of the output tensors:
        records, exposure, derotated, frames, lengths (None where not written)."""
        return self._bank_push(bank, camera, times, count, gyro, mavlink, records, out_frames, out_lengths, n_rounds,
                               round_stride, camera=True, exposure=exposure, derotated=derotated, want_exposure=want_exposure)

    def bank_collect(self, records, mavlink=None, lengths=None, exposure=None, derotated=None, capacity_messages=None,
                     capacity_exposures=0, outbox=None, tag=1, tag_tensor=None):
        """aof_bank_collect_device behind a push: records uint8 CUDA tensor [S, 48] (a tick) or [K, S, 48] (a burst);
        mavlink [.., 56] / lengths [..], exposure [.., 48], derotated float32 [.., 2] (or its 8 bytes): the push's other outputs, or None.
        capacity_messages: entries the outbox holds (default: one per record); outbox: a uint8 CUDA tensor of at least
        outbox_layout().total_bytes, a HostOutbox, or None (a new tensor).  tag: non-zero; tag_tensor: int64 CUDA tensor
        [1] the kernel reads the tag from instead (a captured graph: update it between replays).  Enqueued on torch's
        current stream.  Returns the outbox (read it with outbox_view())."""
        import torch
        dev = records.device
        assert records.dtype == torch.uint8 and records.is_contiguous() and records.shape[-1] == 48 and records.dim() in (2, 3)
        K, S = (1, records.shape[0]) if records.dim() == 2 else (records.shape[0], records.shape[1])
        n = K * S
        assert mavlink is None or (mavlink.is_contiguous() and mavlink.numel() == n * SEQ_FRAME_BYTES)
        assert lengths is None or (lengths.is_contiguous() and lengths.numel() == n)
        assert exposure is None or (exposure.is_contiguous() and exposure.numel() == n * 48)
        assert derotated is None or (derotated.is_contiguous() and derotated.numel() * derotated.element_size() == n * 8)
        assert tag_tensor is None or (tag_tensor.dtype == torch.int64 and tag_tensor.numel() == 1)
        if capacity_messages is None:
            capacity_messages = outbox.capacity_messages if isinstance(outbox, HostOutbox) else n
        if outbox is None:
            outbox = torch.empty(outbox_layout(capacity_messages, capacity_exposures).total_bytes, dtype=torch.uint8, device=dev)
        ptr, size = (outbox.ptr, outbox.nbytes) if isinstance(outbox, HostOutbox) else (outbox.data_ptr(), outbox.numel())
        opt = lambda t: t.data_ptr() if t is not None else None
        self._check(lib.aof_bank_collect_device(
            self._ctx, S, K, records.data_ptr(), opt(mavlink), opt(lengths), opt(exposure), opt(derotated),
            capacity_messages, capacity_exposures, ptr, size, int(tag), opt(tag_tensor), torch.cuda.current_stream(dev).cuda_stream))
        return outbox

    def bank_exposure_reset(self, state, mask=None, exposure0=1, gain0=1, exposures=None, gains=None):
        """aof_bank_exposure_reset_device: state uint8 CUDA tensor [S, 16] (``aof_exposure_state``; read it with
        exposure_states_view()); mask uint8 [S] (non-zero = reset) or None (all); the streams start from exposures
        (int16/uint16 [S]) / gains (uint8 [S]) where given, else from the scalars.  Enqueued on torch's current stream."""
        import torch
        S = state.numel() // 16
        assert state.dtype == torch.uint8 and state.is_contiguous() and state.numel() == 16 * S
        assert mask is None or (mask.dtype == torch.uint8 and mask.numel() == S and mask.is_contiguous())
        assert exposures is None or (exposures.element_size() == 2 and exposures.numel() == S and exposures.is_contiguous())
        assert gains is None or (gains.dtype == torch.uint8 and gains.numel() == S and gains.is_contiguous())
        opt = lambda t: t.data_ptr() if t is not None else None
        self._check(lib.aof_bank_exposure_reset_device(self._ctx, S, opt(mask), int(exposure0), int(gain0), opt(exposures),
                                                       opt(gains), state.data_ptr(), torch.cuda.current_stream(state.device).cuda_stream))

    def bank_exposure_control(self, exposure, state, commands=None, ec: ExposureControl = None):
        """aof_bank_exposure_control_device behind a camera push: exposure uint8 CUDA tensor [S, 48] (a tick) or
        [K, S, 48] (a burst), what the push wrote; state uint8 [S, 16], stepped in place; commands: uint8 CUDA tensor
        [.., 16], a numpy uint8 array over device-mapped host memory (a HostOutbox's ``array``), or None (a new tensor).
        Enqueued on torch's current stream.  Returns the commands (read them with exposure_commands_view())."""
        import torch
        dev = exposure.device
        assert exposure.dtype == torch.uint8 and exposure.is_contiguous() and exposure.shape[-1] == 48 and exposure.dim() in (2, 3)
        K, S = (1, exposure.shape[0]) if exposure.dim() == 2 else (exposure.shape[0], exposure.shape[1])
        assert state.dtype == torch.uint8 and state.is_contiguous() and state.numel() == 16 * S
        if commands is None:
            commands = torch.empty(tuple(exposure.shape[:-1]) + (16,), dtype=torch.uint8, device=dev)
        if isinstance(commands, np.ndarray):
            assert commands.dtype == np.uint8 and commands.size == 16 * K * S and commands.flags.c_contiguous
            ptr = commands.ctypes.data
        else:
            assert commands.dtype == torch.uint8 and commands.is_contiguous() and commands.numel() == 16 * K * S
            ptr = commands.data_ptr()
        ec = exposure_control_default() if ec is None else ec
        self._check(lib.aof_bank_exposure_control_device(self._ctx, C.byref(ec), S, K, exposure.data_ptr(), state.data_ptr(), ptr,
                                                         torch.cuda.current_stream(dev).cuda_stream))
        return commands

    def bank_imu_reset(self, state, mask=None, offset0=0):
        """aof_bank_imu_reset_device: state uint8 CUDA tensor [S, 64] (``aof_imu_state``; read it with imu_states_view());
        mask uint8 [S] (non-zero = reset) or None (all); offset0: the streams' vehicle-time offset, 0 = learned from the
        first sample.  Enqueued on torch's current stream."""
        import torch
        S = state.numel() // 64
        assert state.dtype == torch.uint8 and state.is_contiguous() and state.numel() == 64 * S
        assert mask is None or (mask.dtype == torch.uint8 and mask.numel() == S and mask.is_contiguous())
        self._check(lib.aof_bank_imu_reset_device(self._ctx, S, mask.data_ptr() if mask is not None else None, int(offset0),
                                                  state.data_ptr(), torch.cuda.current_stream(state.device).cuda_stream))

    def bank_imu(self, samples, times, records, state, counts=None, mavlink=True, records_out=None, out_frames=None,
                 out_lengths=None, system_id=1, component_id=100, first_seq=0):
        """aof_bank_imu_device behind a records-only push: samples uint8 CUDA tensor [K, M, S, 24] (or [M, S, 24] for a
        tick); times int64 [K, S] / [S], what the push was given; records uint8 [K, S, 48] / [S, 48], what it wrote;
        state uint8 [S, 64], stepped in place; counts uint8 [K, S] / [S] or None (M everywhere).  records_out: `records`
        itself (in place), another tensor of its shape, or None (a new one); out_frames [.., 56] / out_lengths [..]:
        tensors, numpy uint8 arrays over device-mapped host memory, or None (new tensors, zero-filled).  Enqueued on
        torch's current stream.  Returns (records_out, frames, lengths); the last two are None with mavlink=False."""
        import torch
        dev = records.device
        assert records.dtype == torch.uint8 and records.is_contiguous() and records.shape[-1] == 48 and records.dim() in (2, 3)
        K, S = (1, records.shape[0]) if records.dim() == 2 else (records.shape[0], records.shape[1])
        lead = tuple(records.shape[:-1])
        assert samples.dtype == torch.uint8 and samples.is_contiguous() and samples.shape[-1] == 24 and samples.numel() % (24 * K * S) == 0
        M = samples.numel() // (24 * K * S)
        assert times.dtype == torch.int64 and times.is_contiguous() and times.numel() == K * S
        assert state.dtype == torch.uint8 and state.is_contiguous() and state.numel() == 64 * S
        assert counts is None or (counts.dtype == torch.uint8 and counts.is_contiguous() and counts.numel() == K * S)
        if records_out is None:
            records_out = torch.empty_like(records)
        assert records_out.dtype == torch.uint8 and records_out.is_contiguous() and records_out.shape == records.shape
        ptr = lambda t: None if t is None else t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr()
        if mavlink:
            if out_frames is None:
                out_frames = torch.zeros(lead + (SEQ_FRAME_BYTES,), dtype=torch.uint8, device=dev)
            if out_lengths is None:
                out_lengths = torch.zeros(lead, dtype=torch.uint8, device=dev)
            for t, n in ((out_frames, K * S * SEQ_FRAME_BYTES), (out_lengths, K * S)):
                if isinstance(t, np.ndarray):
                    assert t.dtype == np.uint8 and t.size == n and t.flags.c_contiguous
                else:
                    assert t.dtype == torch.uint8 and t.is_contiguous() and t.numel() == n
        else:
            out_frames = out_lengths = None
        ip = imu_params(S, K, M, system_id, component_id, first_seq)
        self._check(lib.aof_bank_imu_device(self._ctx, C.byref(ip), samples.data_ptr(), ptr(counts), times.data_ptr(),
                                            records.data_ptr(), state.data_ptr(), records_out.data_ptr(), ptr(out_frames),
                                            ptr(out_lengths), torch.cuda.current_stream(dev).cuda_stream))
        return records_out, out_frames, out_lengths

    def bank_mavlink_rx_reset(self, state, mask=None):
        """aof_bank_mavlink_rx_reset_device: state uint8 CUDA tensor [S, 128] (``aof_mavlink_rx_state``; read it with
        mavlink_rx_states_view()); mask uint8 [S] (non-zero = reset) or None (all).  Enqueued on torch's current stream."""
        import torch
        S = state.numel() // 128
        assert state.dtype == torch.uint8 and state.is_contiguous() and state.numel() == 128 * S
        assert mask is None or (mask.dtype == torch.uint8 and mask.numel() == S and mask.is_contiguous())
        self._check(lib.aof_bank_mavlink_rx_reset_device(self._ctx, S, mask.data_ptr() if mask is not None else None,
                                                         state.data_ptr(), torch.cuda.current_stream(state.device).cuda_stream))

    def bank_mavlink_rx(self, data, state, max_samples, lengths=None, samples=None, counts=None):
        """aof_bank_mavlink_rx_device in front of bank_imu(): data uint8 CUDA tensor [K, S, B] (or [S, B] for a tick), what
        each stream received; lengths: a tensor of K * S 16-bit elements (the received byte counts) or None (B everywhere);
        state uint8 [S, 128], stepped in place; samples uint8 [K, M, S, 24] / [M, S, 24] and counts uint8 [K, S] / [S]:
        tensors to write or None (new ones, zero-filled) -- what bank_imu() takes.  Enqueued on torch's current stream.
        Returns (samples, counts)."""
        import torch
        dev = data.device
        assert data.dtype == torch.uint8 and data.is_contiguous() and data.dim() in (2, 3)
        K, S, B = (1,) + tuple(data.shape) if data.dim() == 2 else tuple(data.shape)
        M = int(max_samples)
        assert state.dtype == torch.uint8 and state.is_contiguous() and state.numel() == 128 * S
        assert lengths is None or (lengths.element_size() == 2 and lengths.is_contiguous() and lengths.numel() == K * S)
        if samples is None:
            samples = torch.zeros(((K,) if data.dim() == 3 else ()) + (M, S, 24), dtype=torch.uint8, device=dev)
        if counts is None:
            counts = torch.zeros(tuple(data.shape[:-1]), dtype=torch.uint8, device=dev)
        assert samples.dtype == torch.uint8 and samples.is_contiguous() and samples.numel() == K * M * S * 24
        assert counts.dtype == torch.uint8 and counts.is_contiguous() and counts.numel() == K * S
        rp = mavlink_rx_params(S, K, B, M)
        self._check(lib.aof_bank_mavlink_rx_device(self._ctx, C.byref(rp), data.data_ptr(),
                                                   lengths.data_ptr() if lengths is not None else None, state.data_ptr(),
                                                   samples.data_ptr(), counts.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        return samples, counts

    def _bind_bank_table(self, setter, keep, tensor, n_streams, item, *extra):
        """The one body of the four set_bank_* methods: `setter` of the library on `tensor` (None: unbind) for n_streams
        streams (None: as many as the tensor holds), `item` bytes per stream -- records (item > 1) come in whole records and
        for at least one stream, byte arrays only have to hold n_streams --; `extra`: further arguments of the setter (zeros
        when unbinding).  The tensor is kept alive in attribute `keep` for as long as it is bound."""
        if tensor is None:
            self._check(setter(self._ctx, None, 0, *(0 for _ in extra)))
            setattr(self, keep, None)
            return
        import torch
        assert tensor.dtype == torch.uint8 and tensor.is_contiguous() and tensor.numel() % item == 0
        n = tensor.numel() // item if n_streams is None else int(n_streams)
        assert (item == 1 or 1 <= n) and n <= tensor.numel() // item
        self._check(setter(self._ctx, tensor.data_ptr(), n, *extra))
        setattr(self, keep, tensor)

    def set_bank_streams(self, streams=None, n_streams=None):
        """aof_set_bank_streams: binds a uint8 CUDA tensor of S * 32 bytes (``aof_bank_stream`` records, BANK_STREAM_DTYPE;
        16-byte aligned) to the context, or with None unbinds.  n_streams: S, where the tensor holds more than S records.  While it is bound every push and IMU call of S streams
        takes focal lengths, output rate, time offset and MAVLink identity of stream s from record s; the kernels read
        it when they run, so the tensor must stay alive and may be rewritten between ticks.  Enqueues nothing."""
        self._bind_bank_table(lib.aof_set_bank_streams, "_bank_streams", streams, n_streams, 32)

    def set_bank_sensors(self, sensors=None, n_streams=None, camera_bytes=0):
        """aof_set_bank_sensors: binds a uint8 CUDA tensor of S * 32 bytes (``aof_bank_sensor`` records, BANK_SENSOR_DTYPE;
        16-byte aligned) to the context, or with None unbinds.  n_streams: S, where the tensor holds more than S records;
        camera_bytes: the bytes readable from the camera tensor of the pushes.  While it is bound every camera push of S
        streams takes the place, row pitch, size and crop origin of stream s's sensor frame from record s; the kernels
        read it when they run, so the tensor must stay alive and may be rewritten between ticks.  Enqueues nothing."""
        self._bind_bank_table(lib.aof_set_bank_sensors, "_bank_sensors", sensors, n_streams, 32, int(camera_bytes))

    def set_bank_pixel_formats(self, formats=None, n_streams=None):
        """aof_set_bank_pixel_formats: binds a uint8 CUDA tensor of S pixel formats (PIXEL_GREY8 .. PIXEL_Y12P;
        any alignment) to the context, or with None unbinds.  n_streams: S, where the tensor holds more.
        Used by the camera pushes next to bound sensor records (set_bank_sensors): stream s's crop then comes from pixels
        of one or two bytes.  The kernels read it when they run: keep it alive; it may be rewritten between ticks."""
        self._bind_bank_table(lib.aof_set_bank_pixel_formats, "_bank_formats", formats, n_streams, 1)

    def set_bank_binning(self, bins=None, n_streams=None):
        """aof_set_bank_binning: binds a uint8 CUDA tensor of S bins (1, 2 or 4; any alignment) to the context, or with None
        unbinds.  n_streams: S, where the tensor holds more.  Used by the camera pushes next to bound sensor records
        (set_bank_sensors): a pixel of stream s's crop is then the rounded mean of bin x bin sensor pixels.  The focal
        length stays the caller's (focal / bin through set_bank_streams).  The kernels read it when they run: keep it alive;
        it may be rewritten between ticks."""
        self._bind_bank_table(lib.aof_set_bank_binning, "_bank_bins", bins, n_streams, 1)

    def set_bank_warps(self, points=None, n_streams=None):
        """aof_set_bank_warps: binds a uint8 CUDA tensor of S meshes (S * ny * nx nodes of WARP_POINT_DTYPE, 16-byte
        aligned; warp_mesh_size) to the context, or with None unbinds.  n_streams: S, where the tensor holds more.  While it
        is bound every camera push of S streams resamples stream s's crop through mesh s (a first node with x == WARP_NONE:
        the plain crop); set_bank_path applies as ever -- the one-launch form is the tick kernel with the warp inside it
        (bank_warp_one_launch says whether the configuration has one; last_bank_path says what a push took).  The kernels
        read it when they run: keep it alive; it may be rewritten between ticks."""
        nx, ny = warp_mesh_size(self.params)
        self._bind_bank_table(lib.aof_set_bank_warps, "_bank_warps", points, n_streams, nx * ny * 8)

    def ingest_warped(self, camera, sensors, points, **kw):
        """ingest_warped for the context's crop size."""
        return ingest_warped(camera, sensors, points, self.params.width, self.params.height, **kw)

    def warp_host(self, camera, rec, mesh, format=0, camera_bytes=None):
        """warp_host for the context's crop size."""
        return warp_host(camera, rec, self.params.width, self.params.height, mesh, format, camera_bytes)

    def set_bank_path(self, path=0):
        """0: the library chooses between the one-launch tick kernel and the composed path, 1: the tick kernel where
        the configuration allows it, 2: always the composed path.  Same bytes either way."""
        self._check(lib.aof_set_bank_path(self._ctx, int(path)))

    def last_bank_path(self) -> int:
        """aof_bank_last_path: 0 no push yet, 1 the most recent accepted push ran one-launch kernel(s), 2 the composed
        launches.  A refused push leaves it as it was."""
        rc = lib.aof_bank_last_path(self._ctx)
        if rc < 0:
            raise AofError(rc, lib.aof_strerror(rc).decode())
        return int(rc)

    # -- host buffers -----------------------------------------------------------
    def flow_pair_host(self, prev: np.ndarray, cur: np.ndarray):
        p = self.params
        prev = np.ascontiguousarray(prev, dtype=np.uint8)
        cur = np.ascontiguousarray(cur, dtype=np.uint8)
        assert prev.shape == cur.shape == (p.height, p.width)
        nb = self.nblocks(0)
        blocks = np.zeros(nb, dtype=BLOCK_DTYPE)
        subdirs = np.zeros(nb, dtype=np.uint8)
        flow = np.zeros(1, dtype=FLOW_DTYPE)
        self._check(lib.aof_flow_pair_host(self._ctx, prev.ctypes.data, cur.ctypes.data,
                                           blocks.ctypes.data, subdirs.ctypes.data,
                                           flow.ctypes.data))
        return blocks, subdirs, flow[0]

    def stream_push(self, frame: np.ndarray):
        """Returns None for the first frame, else the flow record vs the previous frame."""
        p = self.params
        frame = np.ascontiguousarray(frame, dtype=np.uint8)
        assert frame.shape == (p.height, p.width)
        flow = np.zeros(1, dtype=FLOW_DTYPE)
        rc = self._check(lib.aof_stream_push_host(self._ctx, frame.ctypes.data, flow.ctypes.data))
        return None if rc == 1 else flow[0]

    def set_stream_graph(self, on=True):
        """Streaming entry point: replay a captured hipGraph per frame (default) or launch eagerly."""
        self._check(lib.aof_set_stream_graph(self._ctx, int(on)))

    def set_stream_resident(self, on=True):
        """Streaming entry point for small frames: a resident one-workgroup kernel serves the calls
        through a mailbox in pinned memory instead of one launch per frame."""
        self._check(lib.aof_set_stream_resident(self._ctx, int(on)))

    def stream_resident_running(self) -> bool:
        return lib.aof_set_stream_resident(self._ctx, -1) == 1

    def stream_stats(self) -> dict:
        """Counters of the streaming entry point (``aof_stream_stats``)."""
        st = StreamStats()
        self._check(lib.aof_stream_get_stats(self._ctx, C.byref(st)))
        return st.as_dict()

    def debug_resident_fault(self, deaf=True, stop_wait_us=0):
        """Fault injection: resident kernels ignore the request to leave; the library's wait for them is shortened."""
        self._check(lib.aof_debug_resident_fault(self._ctx, int(deaf), int(stop_wait_us)))

    def set_vote_deadline_us(self, microseconds):
        """Deadline of the finaliser waves of the in-launch reduction (at least 100 us)."""
        self._check(lib.aof_set_vote_deadline_us(self._ctx, int(microseconds)))

    def debug_vote_deadline_ticks(self, ticks):
        """Fault injection: that deadline in 10 ns ticks, unchecked (0: every finaliser gives up at once)."""
        self._check(lib.aof_debug_vote_deadline_ticks(self._ctx, int(ticks)))

    def debug_tile16_verdicts(self, verdicts=()):
        """Test hook of the 16x16 adaptive search: pair i gets verdicts[i % len(verdicts)] (0..4, as in the workspace's
        hints) instead of the probe's; an empty sequence gives the decision back to the probe."""
        v = [int(x) for x in verdicts]
        self._check(lib.aof_debug_tile16_verdicts(self._ctx, (C.c_uint8 * max(len(v), 1))(*v), len(v)))

    def stream_graph_active(self) -> bool:
        return lib.aof_set_stream_graph(self._ctx, -1) == 1

    def stream_reset(self):
        self._check(lib.aof_stream_reset(self._ctx))


def blocks_view(t) -> np.ndarray:
    """int32 tensor/array of packed records -> structured numpy view."""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(BLOCK_DTYPE).reshape(a.shape)


def flows_view(t) -> np.ndarray:
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(FLOW_DTYPE).reshape(a.shape[0])


# ---- the C++ facade (facade/libOpticalFlow.so) through its plain-C handles -------

FACADE_PATH = os.path.join(_HERE, "facade", "libOpticalFlow.so")
_facade = None


def facade_lib():
    """facade/libOpticalFlow.so: the drop-in classes OpticalFlowPX4 / OpticalFlowOpenCV."""
    global _facade
    if _facade is None:
        if not os.path.exists(FACADE_PATH):
            raise ImportError(f"{FACADE_PATH} is missing: run __graft_entry__.build()")
        f = C.CDLL(FACADE_PATH)
        f.aof_facade_px4_create.restype = C.c_void_p
        f.aof_facade_px4_create.argtypes = [C.c_float, C.c_float] + [C.c_int] * 6
        f.aof_facade_opencv_create.restype = C.c_void_p
        f.aof_facade_opencv_create.argtypes = [C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
        f.aof_facade_destroy.argtypes = [C.c_void_p]
        f.aof_facade_calc_flow.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_int),
                                           C.POINTER(C.c_float), C.POINTER(C.c_float)]
        f.aof_facade_px4_track_features.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        f.aof_facade_pack_optical_flow_rad.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_float, C.c_float,
                                                       C.c_double, C.c_double, C.c_double, C.c_int, C.c_uint8,
                                                       C.c_void_p]
        f.aof_facade_mavlink_crc.restype = C.c_uint
        f.aof_facade_mavlink_crc.argtypes = [C.c_void_p, C.c_int]
        f.aof_facade_image_width.argtypes = [C.c_void_p]
        f.aof_facade_set_search_pyramid.argtypes = [C.c_void_p, C.c_int, C.c_int]
        f.aof_facade_pyramid_levels.argtypes = [C.c_void_p]
        f.aof_facade_set_resident.argtypes = [C.c_void_p, C.c_int]
        f.aof_facade_image_height.argtypes = [C.c_void_p]
        f.aof_facade_last_error.restype = C.c_char_p
        f.aof_facade_last_error.argtypes = [C.c_void_p]
        f.aof_facade_bank_create.restype = C.c_void_p
        f.aof_facade_bank_create.argtypes = [C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int]
        f.aof_facade_bank_destroy.argtypes = [C.c_void_p]
        f.aof_facade_bank_set_timestamp_offset.argtypes = [C.c_void_p, C.c_uint64]
        f.aof_facade_bank_set_stream_focal_length.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float]
        f.aof_facade_bank_set_stream_output_rate.argtypes = [C.c_void_p, C.c_int, C.c_int]
        f.aof_facade_bank_set_stream_identity.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        f.aof_facade_bank_set_stream_timestamp_offset.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
        f.aof_facade_bank_set_stream_sensor.argtypes = [C.c_void_p, C.c_int, C.c_uint64] + [C.c_int] * 5
        f.aof_facade_bank_set_stream_pixel_format.argtypes = [C.c_void_p, C.c_int, C.c_int]
        f.aof_facade_bank_set_stream_binning.argtypes = [C.c_void_p, C.c_int, C.c_int]
        f.aof_facade_bank_set_stream_warp.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        f.aof_facade_bank_set_stream_lens.argtypes = [C.c_void_p, C.c_int] + [C.c_double] * 9
        f.aof_facade_bank_enable_camera_packed.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32]
        f.aof_facade_bank_push.argtypes = [C.c_void_p] * 5
        f.aof_facade_bank_enable_camera.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32]
        f.aof_facade_bank_push_camera.argtypes = [C.c_void_p] * 5
        f.aof_facade_bank_enable_imu.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
        f.aof_facade_bank_push_imu.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_float, C.c_float, C.c_float]
        f.aof_facade_bank_enable_mavlink_rx.argtypes = [C.c_void_p, C.c_int]
        f.aof_facade_bank_push_mavlink.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        f.aof_facade_bank_exposure_commands.restype = C.c_void_p
        f.aof_facade_bank_exposure_commands.argtypes = [C.c_void_p]
        f.aof_facade_bank_published.restype = C.c_void_p
        f.aof_facade_bank_published.argtypes = [C.c_void_p]
        f.aof_facade_bank_reset.argtypes = [C.c_void_p, C.c_void_p]
        f.aof_facade_bank_pyramid_levels.argtypes = [C.c_void_p]
        f.aof_facade_bank_last_push_path.argtypes = [C.c_void_p]
        f.aof_facade_bank_ok.argtypes = [C.c_void_p]
        f.aof_facade_bank_last_error.restype = C.c_char_p
        f.aof_facade_bank_last_error.argtypes = [C.c_void_p]
        _facade = f
    return _facade


def pack_optical_flow_rad(offset_ts, img_time_us, dt_us, flow_x, flow_y, gyro=(0.0, 0.0, 0.0), quality=0,
                          seq=0) -> bytes:
    """The OPTICAL_FLOW_RAD MAVLink 2 frame the reference would send for these calcFlow
    outputs (/root/reference/src/mainloop.cpp:359-373, src/mavlink_tcp.cpp:142-162)."""
    buf = (C.c_uint8 * 56)()
    n = facade_lib().aof_facade_pack_optical_flow_rad(offset_ts, img_time_us, dt_us, flow_x, flow_y, gyro[0],
                                                      gyro[1], gyro[2], quality, seq, buf)
    return bytes(buf[:n])


DEFAULT_OUTPUT_RATE = 15
DEFAULT_IMAGE_WIDTH = 64
DEFAULT_IMAGE_HEIGHT = 64
DEFAULT_SEARCH_SIZE = 4
DEFAULT_FLOW_FEATURE_THRESHOLD = 30
DEFAULT_FLOW_VALUE_THRESHOLD = 3000


class _FacadeFlow:
    """Handle on one C++ facade object.  ``calcFlow`` keeps the reference's
    convention (/root/reference/src/mainloop.cpp:322-331): the return value is
    negative while the engine integrates towards its output rate, else the
    quality 0..255 with dt_us and the angular flow (rad)."""
    _h = None

    def getImageWidth(self):
        return facade_lib().aof_facade_image_width(self._h)

    def getImageHeight(self):
        return facade_lib().aof_facade_image_height(self._h)

    def lastError(self):
        return facade_lib().aof_facade_last_error(self._h).decode()

    def setSearchPyramid(self, levels, mean_subtract):
        return bool(facade_lib().aof_facade_set_search_pyramid(self._h, int(levels), int(bool(mean_subtract))))

    def getPyramidLevels(self):
        return facade_lib().aof_facade_pyramid_levels(self._h)

    def setResidentKernel(self, on=True):
        """Serve calcFlow() from a kernel that stays on the device (mailbox in pinned memory)."""
        return bool(facade_lib().aof_facade_set_resident(self._h, int(bool(on))))

    def calcFlow(self, img, img_time_us):
        """Returns (quality, dt_us, flow_x_rad, flow_y_rad); the C++ out-parameters keep
        their previous values (0 here) when the call does not publish."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        assert img.size == self.getImageWidth() * self.getImageHeight()
        dt, fx, fy = C.c_int(0), C.c_float(0), C.c_float(0)
        q = facade_lib().aof_facade_calc_flow(self._h, img.ctypes.data, int(img_time_us) & 0xFFFFFFFF,
                                              C.byref(dt), C.byref(fx), C.byref(fy))
        return q, dt.value, fx.value, fy.value

    def close(self):
        if self._h:
            facade_lib().aof_facade_destroy(self._h)
            self._h = None

    __del__ = close


class OpticalFlowPX4(_FacadeFlow):
    """facade/include/flow_px4.hpp"""

    def __init__(self, f_length_x, f_length_y, output_rate=DEFAULT_OUTPUT_RATE,
                 img_width=DEFAULT_IMAGE_WIDTH, img_height=DEFAULT_IMAGE_HEIGHT,
                 search_size=DEFAULT_SEARCH_SIZE,
                 flow_feature_threshold=DEFAULT_FLOW_FEATURE_THRESHOLD,
                 flow_value_threshold=DEFAULT_FLOW_VALUE_THRESHOLD):
        self._h = facade_lib().aof_facade_px4_create(f_length_x, f_length_y, output_rate, img_width,
                                                      img_height, search_size,
                                                      flow_feature_threshold, flow_value_threshold)


    def trackFeatures(self, img_prev, img_current, capacity=4096):
        """Rows of (prev_x, prev_y, cur_x, cur_y, sad, accepted) per grid tile."""
        a = np.ascontiguousarray(img_prev, dtype=np.uint8)
        b = np.ascontiguousarray(img_current, dtype=np.uint8)
        out = np.zeros((capacity, 6), dtype=np.float32)
        n = facade_lib().aof_facade_px4_track_features(self._h, a.ctypes.data, b.ctypes.data,
                                                       out.ctypes.data, capacity)
        if n < 0:
            raise AofError(n, self.lastError())
        return out[:min(n, capacity)]


class OpticalFlowOpenCV(_FacadeFlow):
    """facade/include/flow_opencv.hpp -- the class /root/reference/src/mainloop.cpp:423 creates."""

    def __init__(self, f_length_x, f_length_y, output_rate=DEFAULT_OUTPUT_RATE,
                 img_width=DEFAULT_IMAGE_WIDTH, img_height=DEFAULT_IMAGE_HEIGHT):
        self._h = facade_lib().aof_facade_opencv_create(f_length_x, f_length_y, output_rate,
                                                         img_width, img_height)


class OpticalFlowBank:
    """facade/include/flow_bank.hpp -- the many-camera counterpart of OpticalFlowOpenCV: one C++ object for
    ``n_streams`` cameras of one frame size, a push() per tick."""

    def __init__(self, f_length_x, f_length_y, output_rate=DEFAULT_OUTPUT_RATE, img_width=DEFAULT_IMAGE_WIDTH,
                 img_height=DEFAULT_IMAGE_HEIGHT, n_streams=1):
        self.n_streams, self.width, self.height = int(n_streams), int(img_width), int(img_height)
        self._h = facade_lib().aof_facade_bank_create(f_length_x, f_length_y, output_rate, img_width, img_height, n_streams)

    def setTimestampOffset(self, offset_usec):
        facade_lib().aof_facade_bank_set_timestamp_offset(self._h, int(offset_usec))

    def setStreamFocalLength(self, s, fx, fy):
        """Stream s's own focal lengths (px), from the next push on.  0, or -EINVAL (bad index or focal length)."""
        return facade_lib().aof_facade_bank_set_stream_focal_length(self._h, int(s), float(fx), float(fy))

    def setStreamOutputRate(self, s, hz):
        """Stream s's own output rate (<= 0: every frame), from the next push on.  0, or -EINVAL for a bad index."""
        return facade_lib().aof_facade_bank_set_stream_output_rate(self._h, int(s), int(hz))

    def setStreamIdentity(self, s, system_id, component_id, first_seq):
        """The MAVLink system id, component id and first sequence number of stream s's frames.  0, or -EINVAL."""
        return facade_lib().aof_facade_bank_set_stream_identity(self._h, int(s), int(system_id) & 0xFF, int(component_id) & 0xFF,
                                                                int(first_seq) & 0xFF)

    def setStreamTimestampOffset(self, s, usec):
        """Stream s's own MAVLink time offset (0: no frame for it); ignored once enableImu() is on.  0, or -EINVAL."""
        return facade_lib().aof_facade_bank_set_stream_timestamp_offset(self._h, int(s), int(usec))

    def setStreamSensor(self, s, offset, pitch, width, height, x0, y0):
        """Stream s's own sensor layout inside the bytes pushCamera() takes: the frame's offset, row pitch, size and the
        crop's origin.  After enableCamera(), from the next pushCamera() on.  0, or -EINVAL (bad index, no
        enableCamera(), a record outside the staging buffer)."""
        return facade_lib().aof_facade_bank_set_stream_sensor(self._h, int(s), int(offset), int(pitch), int(width), int(height),
                                                              int(x0), int(y0))

    def getPyramidLevels(self):
        return facade_lib().aof_facade_bank_pyramid_levels(self._h)

    def lastPushPath(self):
        """How the engine ran the last accepted push: 0 none yet, 1 one launch per tick, 2 the composed launches."""
        return facade_lib().aof_facade_bank_last_push_path(self._h)

    def engineOk(self):
        return bool(facade_lib().aof_facade_bank_ok(self._h))

    def lastError(self):
        return facade_lib().aof_facade_bank_last_error(self._h).decode()

    def _push(self, call, frames, frame_bytes, img_time_us, active, gyro):
        """One tick through `call` (the plain or the sensor-frame delegate): (n, a copy of the n published entries)."""
        S = self.n_streams
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        times = np.ascontiguousarray(img_time_us, dtype=np.uint64)
        assert frames.size == S * frame_bytes and times.size == S
        active = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
        gyro = None if gyro is None else np.ascontiguousarray(gyro, dtype=np.float32)
        assert active is None or active.size == S
        assert gyro is None or gyro.size == 4 * S
        n = call(self._h, frames.ctypes.data, times.ctypes.data, active.ctypes.data if active is not None else None,
                 gyro.ctypes.data if gyro is not None else None)
        if n <= 0:
            return n, np.zeros(0, OUTBOX_ENTRY_DTYPE)
        p = facade_lib().aof_facade_bank_published(self._h)
        return n, np.frombuffer((C.c_uint8 * (128 * n)).from_address(p), dtype=OUTBOX_ENTRY_DTYPE).copy()

    def push(self, frames, img_time_us, active=None, gyro=None):
        """frames uint8 [S, h, w]; img_time_us [S]; active uint8 [S] or None (all); gyro float32 [S, 4] or None.
        Returns (n, entries): the return value of the C++ push() and a copy of its n published entries
        (OUTBOX_ENTRY_DTYPE; empty when n <= 0)."""
        return self._push(facade_lib().aof_facade_bank_push, frames, self.width * self.height, img_time_us, active, gyro)

    def enableCamera(self, camera_width, camera_height, exposure0=1, gain0=1, exposure_interval_us=200000):
        """The sensor-frame form: pushCamera() takes camera_width x camera_height frames, and every stream's
        auto-exposure controller starts from exposure0 / gain0.  Returns 0 or a negative value."""
        rc = facade_lib().aof_facade_bank_enable_camera(self._h, int(camera_width), int(camera_height), int(exposure0), int(gain0),
                                                        int(exposure_interval_us))
        if rc == 0:
            self._sensor = int(camera_width) * int(camera_height)
        return rc

    def enableCameraPacked(self, camera_width, camera_height, format, exposure0=1, gain0=1, exposure_interval_us=200000):
        """enableCamera() for cameras that all deliver pixel format ``format`` (PIXEL_*): pushCamera() then takes
        camera_height rows of bank_pixel_row_bytes(format, camera_width) bytes per stream.  Returns 0 or a negative value
        (-EINVAL also for a value that is no format and a camera_width that is not whole groups of the format)."""
        rc = facade_lib().aof_facade_bank_enable_camera_packed(self._h, int(camera_width), int(camera_height), int(format),
                                                               int(exposure0), int(gain0), int(exposure_interval_us))
        if rc == 0:
            self._sensor = int(camera_height) * bank_pixel_row_bytes(format, camera_width)
        return rc

    def setStreamPixelFormat(self, s, format):
        """Stream s's own pixel format (PIXEL_*) inside the bytes pushCamera() takes, from the next pushCamera() on.  0, or
        -EINVAL (bad index, a value that is no format, before enableCamera(), a record that no longer fits those bytes)."""
        return facade_lib().aof_facade_bank_set_stream_pixel_format(self._h, int(s), int(format))

    def setStreamBinning(self, s, bin):
        """Stream s's binning (1, 2 or 4) inside the bytes pushCamera() takes, from the next pushCamera() on.  0, or -EINVAL
        (bad index, another bin, before enableCamera(), a footprint that no longer fits the stream's sensor frame)."""
        return facade_lib().aof_facade_bank_set_stream_binning(self._h, int(s), int(bin))

    def setStreamWarp(self, s, mesh=None):
        """Stream s's warp mesh ([ny, nx] of WARP_POINT_DTYPE for the image size: warp_mesh_size) from the next pushCamera()
        on; None: the stream's plain crop again.  0, or -EINVAL (bad index, not enabled, an object that bins a stream)."""
        if mesh is None:
            return facade_lib().aof_facade_bank_set_stream_warp(self._h, int(s), None)
        mesh = np.ascontiguousarray(mesh, WARP_POINT_DTYPE)
        nx, ny = (self.width + 7) // 8 + 1, (self.height + 7) // 8 + 1
        assert mesh.shape == (ny, nx), (mesh.shape, (ny, nx))
        return facade_lib().aof_facade_bank_set_stream_warp(self._h, int(s), mesh.ctypes.data)

    def setStreamLens(self, s, fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
        """Stream s's lens: the sensor camera (plane pixels) and its Brown-Conrady coefficients; the image is that of a
        pinhole camera of the same focal lengths with the principal point at the image centre.  0, or -EINVAL as setStreamWarp."""
        return facade_lib().aof_facade_bank_set_stream_lens(self._h, int(s), *(float(v) for v in (fx, fy, cx, cy, k1, k2, p1, p2, k3)))

    def pushCamera(self, sensor_frames, img_time_us, active=None, gyro=None):
        """sensor_frames uint8 [S, camera_height, camera_width] (enableCameraPacked(): [S, camera_height, row_bytes], see
        bank_pixel_row_bytes()); the rest and the return value as push()."""
        assert getattr(self, "_sensor", None), "pushCamera() needs enableCamera()"
        return self._push(facade_lib().aof_facade_bank_push_camera, sensor_frames, self._sensor, img_time_us, active, gyro)

    def enableImu(self, max_samples, offset0=0):
        """The IMU form: pushImu() queues raw gyro samples, push() / pushCamera() ignore their gyro argument, and the
        entries are what the reference would have sent (stale-gyro and no-offset records dropped).  Returns 0 or a
        negative value."""
        return facade_lib().aof_facade_bank_enable_imu(self._h, int(max_samples), int(offset0))

    def pushImu(self, stream, time_usec, xgyro, ygyro, zgyro):
        """One HIGHRES_IMU sample for the stream's next tick: 0, -ENOBUFS (the stream's queue is full), -EINVAL."""
        return facade_lib().aof_facade_bank_push_imu(self._h, int(stream), int(time_usec), float(xgyro), float(ygyro), float(zgyro))

    def enableMavlinkRx(self, max_bytes):
        """The receive path behind enableImu(): pushMavlink() queues the bytes a stream's connection received, and the
        device parses them into the samples of the stream's next tick; pushImu() then answers -EINVAL.  max_bytes: a
        stream's bytes per tick, 16..4096 and a multiple of 16.  Returns 0 or a negative value."""
        return facade_lib().aof_facade_bank_enable_mavlink_rx(self._h, int(max_bytes))

    def pushMavlink(self, stream, data):
        """Appends received bytes to the stream's slot for its next tick: 0, -ENOBUFS (they do not fit: nothing is
        taken), -EINVAL."""
        data = np.frombuffer(bytes(data), np.uint8)
        return facade_lib().aof_facade_bank_push_mavlink(self._h, int(stream), data.ctypes.data if data.size else None, int(data.size))

    def exposureCommands(self):
        """A copy of the last pushCamera()'s commands (EXPOSURE_COMMAND_DTYPE [n_streams]); None without enableCamera()."""
        p = facade_lib().aof_facade_bank_exposure_commands(self._h)
        if not p:
            return None
        return np.frombuffer((C.c_uint8 * (16 * self.n_streams)).from_address(p), dtype=EXPOSURE_COMMAND_DTYPE).copy()

    def reset(self, mask=None):
        mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        return facade_lib().aof_facade_bank_reset(self._h, mask.ctypes.data if mask is not None else None)

    def close(self):
        if self._h:
            facade_lib().aof_facade_bank_destroy(self._h)
            self._h = None

    __del__ = close
