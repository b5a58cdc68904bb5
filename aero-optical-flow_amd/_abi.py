"""include/aof.h restated for ``ctypes`` and numpy: the constants, the records (a ``Structure`` where the library takes
a pointer to one, a dtype where it fills arrays of them), ``AofError``, and ``lib`` -- ``csrc/libaof.so`` loaded once,
with the signature of every export.  A new entry point of the header is bound here, and here alone."""
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


class BankSensor(C.Structure):
    """``aof_bank_sensor`` (include/aof.h): where one camera's frame lies in the camera buffer, and its crop."""
    _fields_ = [("offset", C.c_uint64), ("pitch", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("x0", C.c_int32), ("y0", C.c_int32), ("reserved", C.c_uint32)]


# the two records that go both ways -- by pointer and in tables the kernels read -- are written once: numpy takes the fields
BANK_STREAM_DTYPE, BANK_SENSOR_DTYPE = np.dtype(BankStream), np.dtype(BankSensor)
assert BANK_STREAM_DTYPE.itemsize == 32 and BANK_SENSOR_DTYPE.itemsize == 32


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
