"""The C++ facade (facade/libOpticalFlow.so) through its plain-C handles: the drop-in classes ``OpticalFlowPX4`` and
``OpticalFlowOpenCV``, their many-camera counterpart ``OpticalFlowBank``, and the OPTICAL_FLOW_RAD packer.  The library
is loaded by the first ``facade_lib()``; nothing here needs it before that."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._abi import _HERE, EXPOSURE_COMMAND_DTYPE, OUTBOX_ENTRY_DTYPE, WARP_POINT_DTYPE, AofError
from .bank import bank_pixel_row_bytes

FACADE_PATH = os.path.join(_HERE, "facade", "libOpticalFlow.so")
_facade = None


def facade_lib():
    """facade/libOpticalFlow.so: the drop-in classes OpticalFlowPX4 / OpticalFlowOpenCV."""
    global _facade
    if _facade is None:
        if not os.path.exists(FACADE_PATH):
            raise ImportError(f"{FACADE_PATH} is missing: run __graft_entry__.build()")
        f = C.CDLL(FACADE_PATH)
        VP, I, F, D, U64 = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_uint64
        sig = {   # (result, arguments)
            "aof_facade_px4_create": (VP, [F, F] + [I] * 6),
            "aof_facade_opencv_create": (VP, [F, F, I, I, I]),
            "aof_facade_destroy": (I, [VP]),
            "aof_facade_calc_flow": (I, [VP, VP, C.c_uint32, C.POINTER(I), C.POINTER(F), C.POINTER(F)]),
            "aof_facade_px4_track_features": (I, [VP, VP, VP, VP, I]),
            "aof_facade_pack_optical_flow_rad": (I, [U64, U64, I, F, F, D, D, D, I, C.c_uint8, VP]),
            "aof_facade_mavlink_crc": (C.c_uint, [VP, I]),
            "aof_facade_image_width": (I, [VP]),
            "aof_facade_set_search_pyramid": (I, [VP, I, I]),
            "aof_facade_pyramid_levels": (I, [VP]),
            "aof_facade_set_resident": (I, [VP, I]),
            "aof_facade_image_height": (I, [VP]),
            "aof_facade_last_error": (C.c_char_p, [VP]),
            "aof_facade_bank_create": (VP, [F, F, I, I, I, I]),
            "aof_facade_bank_destroy": (I, [VP]),
            "aof_facade_bank_set_timestamp_offset": (I, [VP, U64]),
            "aof_facade_bank_set_stream_focal_length": (I, [VP, I, F, F]),
            "aof_facade_bank_set_stream_output_rate": (I, [VP, I, I]),
            "aof_facade_bank_set_stream_identity": (I, [VP, I, I, I, I]),
            "aof_facade_bank_set_stream_timestamp_offset": (I, [VP, I, U64]),
            "aof_facade_bank_set_stream_sensor": (I, [VP, I, U64] + [I] * 5),
            "aof_facade_bank_set_stream_pixel_format": (I, [VP, I, I]),
            "aof_facade_bank_set_stream_binning": (I, [VP, I, I]),
            "aof_facade_bank_set_stream_warp": (I, [VP, I, VP]),
            "aof_facade_bank_set_stream_lens": (I, [VP, I] + [D] * 9),
            "aof_facade_bank_enable_camera_packed": (I, [VP, I, I, I, I, I, C.c_uint32]),
            "aof_facade_bank_push": (I, [VP] * 5),
            "aof_facade_bank_enable_camera": (I, [VP, I, I, I, I, C.c_uint32]),
            "aof_facade_bank_push_camera": (I, [VP] * 5),
            "aof_facade_bank_enable_imu": (I, [VP, I, U64]),
            "aof_facade_bank_push_imu": (I, [VP, I, U64, F, F, F]),
            "aof_facade_bank_enable_mavlink_rx": (I, [VP, I]),
            "aof_facade_bank_push_mavlink": (I, [VP, I, VP, I]),
            "aof_facade_bank_exposure_commands": (VP, [VP]),
            "aof_facade_bank_published": (VP, [VP]),
            "aof_facade_bank_reset": (I, [VP, VP]),
            "aof_facade_bank_pyramid_levels": (I, [VP]),
            "aof_facade_bank_last_push_path": (I, [VP]),
            "aof_facade_bank_ok": (I, [VP]),
            "aof_facade_bank_last_error": (C.c_char_p, [VP]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(f, name)
            fn.restype, fn.argtypes = res, args
        _facade = f
    return _facade


def pack_optical_flow_rad(offset_ts, img_time_us, dt_us, flow_x, flow_y, gyro=(0.0, 0.0, 0.0), quality=0, seq=0) -> bytes:
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

    def __init__(self, f_length_x, f_length_y, output_rate=DEFAULT_OUTPUT_RATE, img_width=DEFAULT_IMAGE_WIDTH,
                 img_height=DEFAULT_IMAGE_HEIGHT, search_size=DEFAULT_SEARCH_SIZE,
                 flow_feature_threshold=DEFAULT_FLOW_FEATURE_THRESHOLD, flow_value_threshold=DEFAULT_FLOW_VALUE_THRESHOLD):
        self._h = facade_lib().aof_facade_px4_create(f_length_x, f_length_y, output_rate, img_width, img_height, search_size,
                                                      flow_feature_threshold, flow_value_threshold)

    def trackFeatures(self, img_prev, img_current, capacity=4096):
        """Rows of (prev_x, prev_y, cur_x, cur_y, sad, accepted) per grid tile."""
        a = np.ascontiguousarray(img_prev, dtype=np.uint8)
        b = np.ascontiguousarray(img_current, dtype=np.uint8)
        out = np.zeros((capacity, 6), dtype=np.float32)
        n = facade_lib().aof_facade_px4_track_features(self._h, a.ctypes.data, b.ctypes.data, out.ctypes.data, capacity)
        if n < 0:
            raise AofError(n, self.lastError())
        return out[:min(n, capacity)]


class OpticalFlowOpenCV(_FacadeFlow):
    """facade/include/flow_opencv.hpp -- the class /root/reference/src/mainloop.cpp:423 creates."""

    def __init__(self, f_length_x, f_length_y, output_rate=DEFAULT_OUTPUT_RATE, img_width=DEFAULT_IMAGE_WIDTH,
                 img_height=DEFAULT_IMAGE_HEIGHT):
        self._h = facade_lib().aof_facade_opencv_create(f_length_x, f_length_y, output_rate, img_width, img_height)


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
