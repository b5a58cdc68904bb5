"""Parameters, grids and layouts; frame ingest, de-rotation and the motion-field fit beside a batch; and
``FlowEngine``, one ``aof_ctx``: the batched device-resident hot path, a recorded sequence as one pipeline, the
per-call host paths, profiling and the debug knobs.  Its stream-bank methods come from ``bank.BankCalls``."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import *   # noqa: F403 -- the header: lib, the records (Params ...), the dtypes and constants (UPPER_CASE)
from ._util import check, ptr, records_view
from .bank import BankCalls


def default_params(width, height, **overrides) -> Params:
    p = Params()
    lib.aof_params_default(C.byref(p), width, height)
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, int(v))
    return p


def px4flow_params(width, height, search=4, feature_threshold=30, value_threshold=3000, **overrides) -> Params:
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
    check(lib.aof_grid(C.byref(p), level, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def workspace_layout(p: Params, n_pairs: int) -> WsLayout:
    L = WsLayout()
    check(lib.aof_workspace_layout(C.byref(p), n_pairs, C.byref(L)))
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
    check(lib.aof_ingest_batch_device(C.byref(p), camera.data_ptr(), camera.stride(0), n,
                                      cropped.data_ptr(), cropped.stride(0) if n else crop_w * crop_h, ptr(hist), stream))
    return cropped, hist


def exposure_msv(hist) -> float:
    h = np.ascontiguousarray(np.asarray(hist), dtype=np.uint32)
    assert h.shape == (10,)
    return float(lib.aof_exposure_msv(h.ctypes.data))


def derotate_batch(flows, gyro, focal_x, focal_y, max_flow, rate_threshold):
    """Published PX4Flow gyro compensation of a batch of flow records on the device.
    flows: uint8 CUDA tensor [n, 16] (aof_flow records); gyro: float32 CUDA tensor [n, 4]
    (integ_x, integ_y, integ_z, dt_s).  Returns float32 [n, 2]."""
    import torch
    n = flows.shape[0]
    out = torch.empty((n, 2), dtype=torch.float32, device=flows.device)
    p = DerotateParams(focal_x, focal_y, max_flow, rate_threshold)
    check(lib.aof_derotate_batch_device(C.byref(p), flows.data_ptr(), gyro.data_ptr(), n, out.data_ptr(),
                                        torch.cuda.current_stream(flows.device).cuda_stream))
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
    check(lib.aof_sequence_layout(C.byref(p), C.byref(sp), n_frames, C.byref(L)))
    return L


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
    check(lib.aof_field_host(C.byref(p), C.byref(fp), blocks.ctypes.data, ptr(subdirs), flows.ctypes.data, n, out.ctypes.data))
    return out


def fields_view(t) -> np.ndarray:
    """uint8 tensor/array [n, 64] of ``aof_field`` -> structured numpy view [n]."""
    return records_view(t, FIELD_DTYPE)


def blocks_view(t) -> np.ndarray:
    """int32 tensor/array of packed records -> structured numpy view."""
    return records_view(t, BLOCK_DTYPE, drop=0)


def flows_view(t) -> np.ndarray:
    return records_view(t, FLOW_DTYPE)


class FlowEngine(BankCalls):
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
    def flow_batch(self, prev, cur, blocks=None, subdirs=None, flows=None, workspace=None, pair_stride=None, n_pairs=None):
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
            subdirs.data_ptr() if subdirs is not None else None, flows.data_ptr(), workspace.data_ptr(), workspace.numel(), stream))
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
        self._check(lib.aof_field_batch_device(self._ctx, C.byref(fp), blocks.data_ptr(), ptr(subdirs), flows.data_ptr(), n,
                                               fields.data_ptr(), stream))
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
                subdirs.data_ptr() if subdirs is not None else None, flows.data_ptr(), workspace.data_ptr(), workspace.numel())
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
                                            time_us.data_ptr(), ptr(gyro), workspace.data_ptr(), workspace.numel(), stream))
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
        self._check(lib.aof_flow_pair_host(self._ctx, prev.ctypes.data, cur.ctypes.data, blocks.ctypes.data, subdirs.ctypes.data,
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
