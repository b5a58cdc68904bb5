"""The stream bank (many live cameras per tick): its parameters, layouts, sensor records, pixel formats and warp
meshes; ``Bank`` and the outbox; the host twins of the controller, the IMU call and the MAVLink receive; the views of
its records; and ``BankCalls``, the bank methods of ``FlowEngine``."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import *   # noqa: F403 -- the header: lib, the records (BankParams ...), the dtypes and constants (UPPER_CASE)
from ._util import assert_mask, check, mavlink_outputs, ptr, records_view, rounds_of


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
    check(lib.aof_bank_stream_from_params(C.byref(bp), C.byref(rec)))
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
        check(lib.aof_bank_sensor_from_camera(C.byref(p), C.byref(cam), int(s), C.byref(rec)))
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
    check(rc)
    return _sensor_record(rec)


def bank_pixel_row_bytes(format, width) -> int:
    """aof_bank_pixel_row_bytes: the bytes of a row of ``width`` pixels of ``format`` (PIXEL_*), (width / G) * Bg.  AofError
    (-EINVAL) for a value that is no format, width < 1 or a width that is not whole groups."""
    out = C.c_int64(0)
    check(lib.aof_bank_pixel_row_bytes(int(format) & 0xFF, int(width), C.byref(out)))
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
    return bool(check(rc))


def ingest_sensors(camera, sensors, crop_w, crop_h, camera_bytes=None, cropped=None, hist=None, ok=None, want_cropped=True,
                   want_hist=True, want_ok=True, formats=None, bins=None):
    """aof_ingest_sensors_device: frame ingest on the device for frames that sensor records describe.  camera: uint8 CUDA
    tensor (any shape; the records' offsets count from its first byte); sensors: uint8 CUDA tensor of n * 32 bytes
    (BANK_SENSOR_DTYPE, 16-byte aligned); camera_bytes: bytes of ``camera`` the kernel may read (default: all).
    formats: None, or a uint8 CUDA tensor of n pixel formats (PIXEL_*; aof_ingest_sensor_formats_device).  bins: None, or
    a uint8 CUDA tensor of n bins (1, 2, 4; aof_ingest_sensors_binned_device): crop_w x crop_h is the binned crop.  Returns
    (cropped [n, crop_h, crop_w], hist [n, 10] int32, ok [n] uint8), None where not wanted."""
    return _ingest(camera, sensors, crop_w, crop_h, None, bins, camera_bytes=camera_bytes, cropped=cropped, hist=hist, ok=ok,
                   want_cropped=want_cropped, want_hist=want_hist, want_ok=want_ok, formats=formats)


def _ingest(camera, sensors, crop_w, crop_h, points, bins, *, camera_bytes, cropped, hist, ok, want_cropped, want_hist, want_ok,
            formats):
    """The one body of ingest_sensors and ingest_warped (points: the meshes): the assertions, the outputs, the one call."""
    import torch
    assert camera.dtype == torch.uint8 and sensors.dtype == torch.uint8 and sensors.is_contiguous() and sensors.numel() % 32 == 0
    assert points is None or (points.dtype == torch.uint8 and points.is_contiguous())
    n = sensors.numel() // 32
    assert formats is None or (formats.dtype == torch.uint8 and formats.is_contiguous() and formats.numel() == n)
    assert bins is None or (bins.dtype == torch.uint8 and bins.is_contiguous() and bins.numel() == n)
    nodes = ((int(crop_w) + 7) // 8 + 1) * ((int(crop_h) + 7) // 8 + 1)
    assert points is None or points.numel() >= n * nodes * 8
    dev = camera.device
    if cropped is None and want_cropped:
        cropped = torch.empty((n, crop_h, crop_w), dtype=torch.uint8, device=dev)
    if hist is None and want_hist:
        hist = torch.empty((n, 10), dtype=torch.int32, device=dev)
    if ok is None and want_ok:
        ok = torch.empty((n,), dtype=torch.uint8, device=dev)
    tail = (n, ptr(cropped), cropped.stride(0) if cropped is not None and n else crop_w * crop_h, ptr(hist), ptr(ok),
            torch.cuda.current_stream(dev).cuda_stream)
    head = (int(crop_w), int(crop_h), camera.data_ptr(), camera.numel() if camera_bytes is None else int(camera_bytes), sensors.data_ptr())
    if points is not None:
        rc = lib.aof_ingest_warped_device(*head, ptr(formats), points.data_ptr(), *tail)
    elif bins is not None:
        rc = lib.aof_ingest_sensors_binned_device(*head, ptr(formats), bins.data_ptr(), *tail)
    elif formats is None:
        rc = lib.aof_ingest_sensors_device(*head, *tail)
    else:
        rc = lib.aof_ingest_sensor_formats_device(*head, formats.data_ptr(), *tail)
    check(rc)
    return cropped, hist, ok


def warp_mesh_size(p: Params):
    """aof_warp_mesh_size: (nx, ny), the nodes of the mesh of p.width x p.height -- one every WARP_CELL crop pixels."""
    nx, ny = C.c_int32(0), C.c_int32(0)
    check(lib.aof_warp_mesh_size(C.byref(p), C.byref(nx), C.byref(ny)))
    return int(nx.value), int(ny.value)


def warp_mesh_identity(p: Params, x0, y0) -> np.ndarray:
    """aof_warp_mesh_identity: the mesh [ny, nx] (WARP_POINT_DTYPE) that gives the plain crop at (x0, y0) byte for byte."""
    nx, ny = warp_mesh_size(p)
    out = np.zeros((ny, nx), WARP_POINT_DTYPE)
    check(lib.aof_warp_mesh_identity(C.byref(p), int(x0), int(y0), out.ctypes.data))
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
    check(lib.aof_warp_mesh_from_lens(C.byref(p), C.byref(lens), out.ctypes.data))
    return out


def bank_warp_one_launch(p: Params):
    """aof_bank_warp_one_launch: (ok, lds_bytes) -- can a camera push of configuration p with warps bound run as one launch
    per round, and the dynamic LDS a workgroup of it would ask for (the one-workgroup plan's bytes plus 8 nx ny)."""
    lds = C.c_int64(0)
    rc = check(lib.aof_bank_warp_one_launch(C.byref(p), C.byref(lds)))
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
    rc = check(lib.aof_warp_host(int(crop_w), int(crop_h), camera.ctypes.data, camera.size if camera_bytes is None else int(camera_bytes),
                                 C.byref(r), int(format) & 0xFF, mesh.ctypes.data, crop.ctypes.data, hist.ctypes.data))
    return (crop, hist) if rc else None


def ingest_warped(camera, sensors, points, crop_w, crop_h, camera_bytes=None, cropped=None, hist=None, ok=None, want_cropped=True,
                  want_hist=True, want_ok=True, formats=None):
    """aof_ingest_warped_device: ingest_sensors with frame i resampled through mesh i.  points: uint8 CUDA tensor of
    n * ny * nx * 8 bytes (WARP_POINT_DTYPE nodes, 16-byte aligned).  Returns (cropped, hist, ok) as ingest_sensors does."""
    assert points is not None
    return _ingest(camera, sensors, crop_w, crop_h, points, None, camera_bytes=camera_bytes, cropped=cropped, hist=hist, ok=ok,
                   want_cropped=want_cropped, want_hist=want_hist, want_ok=want_ok, formats=formats)


def bank_layout(p: Params, bp: BankParams) -> BankLayout:
    L = BankLayout()
    check(lib.aof_bank_layout(C.byref(p), C.byref(bp), C.byref(L)))
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
    check(lib.aof_bank_camera_layout(C.byref(p), C.byref(bp), C.byref(cam), C.byref(L), C.byref(staging)))
    return L, staging.value


def outbox_layout(capacity_messages, capacity_exposures=0) -> OutboxLayout:
    """``aof_outbox_layout``: byte offsets of the two entry lists behind the 64-byte header, and the outbox's size."""
    L = OutboxLayout()
    check(lib.aof_outbox_layout(capacity_messages, capacity_exposures, C.byref(L)))
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
    check(lib.aof_exposure_control_default(C.byref(ec)))
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
    check(lib.aof_exposure_control_host(C.byref(ec), S, K, records.ctypes.data, states.ctypes.data, commands.ctypes.data))
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
    check(lib.aof_bank_imu_host(C.byref(ip), samples.ctypes.data, ptr(counts), times.ctypes.data, records.ctypes.data,
                                states.ctypes.data, records_out.ctypes.data, ptr(frames), ptr(lengths)))
    return records_out, frames, lengths


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
    check(lib.aof_bank_mavlink_rx_host(C.byref(rp), data.ctypes.data, ptr(lengths), states.ctypes.data, samples.ctypes.data,
                                       counts.ctypes.data))
    return samples, counts


def imu_states_view(t) -> np.ndarray:
    """uint8 tensor/array [S, 64] of ``aof_imu_state`` -> structured numpy view [S]."""
    return records_view(t, IMU_STATE_DTYPE)


def mavlink_rx_states_view(t) -> np.ndarray:
    """uint8 tensor/array [S, 128] of ``aof_mavlink_rx_state`` -> structured numpy view [S]."""
    return records_view(t, MAVLINK_RX_STATE_DTYPE)


def exposure_states_view(t) -> np.ndarray:
    """uint8 tensor/array [S, 16] of ``aof_exposure_state`` -> structured numpy view [S]."""
    return records_view(t, EXPOSURE_STATE_DTYPE)


def exposure_commands_view(t) -> np.ndarray:
    """uint8 tensor/array [.., 16] of ``aof_exposure_command`` -> structured numpy view [..]."""
    return records_view(t, EXPOSURE_COMMAND_DTYPE)


def exposure_view(t) -> np.ndarray:
    """uint8 tensor/array [S, 48] of ``aof_exposure_record`` -> structured numpy view [S]."""
    return records_view(t, EXPOSURE_DTYPE)


def ticks_view(t) -> np.ndarray:
    """uint8 tensor/array [S, 48] of ``aof_tick_record`` -> structured numpy view [S]."""
    return records_view(t, TICK_DTYPE)


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


class BankCalls:
    """The stream-bank methods of ``FlowEngine``, which supplies ``_ctx``, ``_check``, ``params`` and ``device``."""

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
        assert_mask(mask, bank.n_streams)
        self._check(lib.aof_bank_reset_device(self._ctx, C.byref(bank.bp), ptr(mask), buf.data_ptr(), buf.numel(),
                                              torch.cuda.current_stream(buf.device).cuda_stream))

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
        out_frames, out_lengths = mavlink_outputs(mavlink, out_frames, out_lengths, lead, dev)
        fn = getattr(lib, "aof_bank_push" + ("_camera" if camera else "") + ("_burst" if burst else "") + "_device")
        args = [self._ctx, C.byref(bank.bp)]
        if camera:
            args.append(C.byref(cam))
        if burst:
            args.append(C.byref(bank_burst_params(int(n_rounds), round_stride)))
        args += [src.data_ptr(), times.data_ptr(), ptr(select), ptr(gyro), buf.data_ptr(), buf.numel(), records.data_ptr()]
        if camera:
            args += [ptr(exposure), ptr(derotated)]
        self._check(fn(*args, ptr(out_frames), ptr(out_lengths), torch.cuda.current_stream(dev).cuda_stream))
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
        K, S, _ = rounds_of(records)
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
        box, size = (outbox.ptr, outbox.nbytes) if isinstance(outbox, HostOutbox) else (outbox.data_ptr(), outbox.numel())
        self._check(lib.aof_bank_collect_device(
            self._ctx, S, K, records.data_ptr(), ptr(mavlink), ptr(lengths), ptr(exposure), ptr(derotated),
            capacity_messages, capacity_exposures, box, size, int(tag), ptr(tag_tensor), torch.cuda.current_stream(dev).cuda_stream))
        return outbox

    def bank_exposure_reset(self, state, mask=None, exposure0=1, gain0=1, exposures=None, gains=None):
        """aof_bank_exposure_reset_device: state uint8 CUDA tensor [S, 16] (``aof_exposure_state``; read it with
        exposure_states_view()); mask uint8 [S] (non-zero = reset) or None (all); the streams start from exposures
        (int16/uint16 [S]) / gains (uint8 [S]) where given, else from the scalars.  Enqueued on torch's current stream."""
        import torch
        S = state.numel() // 16
        assert state.dtype == torch.uint8 and state.is_contiguous() and state.numel() == 16 * S
        assert_mask(mask, S)
        assert exposures is None or (exposures.element_size() == 2 and exposures.numel() == S and exposures.is_contiguous())
        assert gains is None or (gains.dtype == torch.uint8 and gains.numel() == S and gains.is_contiguous())
        self._check(lib.aof_bank_exposure_reset_device(self._ctx, S, ptr(mask), int(exposure0), int(gain0), ptr(exposures),
                                                       ptr(gains), state.data_ptr(), torch.cuda.current_stream(state.device).cuda_stream))

    def bank_exposure_control(self, exposure, state, commands=None, ec: ExposureControl = None):
        """aof_bank_exposure_control_device behind a camera push: exposure uint8 CUDA tensor [S, 48] (a tick) or
        [K, S, 48] (a burst), what the push wrote; state uint8 [S, 16], stepped in place; commands: uint8 CUDA tensor
        [.., 16], a numpy uint8 array over device-mapped host memory (a HostOutbox's ``array``), or None (a new tensor).
        Enqueued on torch's current stream.  Returns the commands (read them with exposure_commands_view())."""
        import torch
        dev = exposure.device
        assert exposure.dtype == torch.uint8 and exposure.is_contiguous() and exposure.shape[-1] == 48 and exposure.dim() in (2, 3)
        K, S, lead = rounds_of(exposure)
        assert state.dtype == torch.uint8 and state.is_contiguous() and state.numel() == 16 * S
        if commands is None:
            commands = torch.empty(lead + (16,), dtype=torch.uint8, device=dev)
        if isinstance(commands, np.ndarray):
            assert commands.dtype == np.uint8 and commands.size == 16 * K * S and commands.flags.c_contiguous
        else:
            assert commands.dtype == torch.uint8 and commands.is_contiguous() and commands.numel() == 16 * K * S
        ec = exposure_control_default() if ec is None else ec
        self._check(lib.aof_bank_exposure_control_device(self._ctx, C.byref(ec), S, K, exposure.data_ptr(), state.data_ptr(),
                                                         ptr(commands), torch.cuda.current_stream(dev).cuda_stream))
        return commands

    def bank_imu_reset(self, state, mask=None, offset0=0):
        """aof_bank_imu_reset_device: state uint8 CUDA tensor [S, 64] (``aof_imu_state``; read it with imu_states_view());
        mask uint8 [S] (non-zero = reset) or None (all); offset0: the streams' vehicle-time offset, 0 = learned from the
        first sample.  Enqueued on torch's current stream."""
        import torch
        S = state.numel() // 64
        assert state.dtype == torch.uint8 and state.is_contiguous() and state.numel() == 64 * S
        assert_mask(mask, S)
        self._check(lib.aof_bank_imu_reset_device(self._ctx, S, ptr(mask), int(offset0), state.data_ptr(),
                                                  torch.cuda.current_stream(state.device).cuda_stream))

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
        K, S, lead = rounds_of(records)
        assert samples.dtype == torch.uint8 and samples.is_contiguous() and samples.shape[-1] == 24 and samples.numel() % (24 * K * S) == 0
        M = samples.numel() // (24 * K * S)
        assert times.dtype == torch.int64 and times.is_contiguous() and times.numel() == K * S
        assert state.dtype == torch.uint8 and state.is_contiguous() and state.numel() == 64 * S
        assert counts is None or (counts.dtype == torch.uint8 and counts.is_contiguous() and counts.numel() == K * S)
        if records_out is None:
            records_out = torch.empty_like(records)
        assert records_out.dtype == torch.uint8 and records_out.is_contiguous() and records_out.shape == records.shape
        out_frames, out_lengths = mavlink_outputs(mavlink, out_frames, out_lengths, lead, dev, K * S)
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
        assert_mask(mask, S)
        self._check(lib.aof_bank_mavlink_rx_reset_device(self._ctx, S, ptr(mask), state.data_ptr(),
                                                         torch.cuda.current_stream(state.device).cuda_stream))

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
        self._check(lib.aof_bank_mavlink_rx_device(self._ctx, C.byref(rp), data.data_ptr(), ptr(lengths), state.data_ptr(),
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
        return int(check(lib.aof_bank_last_path(self._ctx)))
