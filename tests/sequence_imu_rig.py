"""The sequence pipeline's IMU call (include/aof_sequence_imu.h) for the tests and tools that drive it: the ctypes record and
prototypes of the two entry points of libaof, written ONCE and here -- the package's surface (tests/golden/binding_surface.json)
does not carry them --, and thin callers over torch tensors and numpy arrays.  The functions are bound on the package's own
handle (aof.lib)."""
import ctypes as C

import numpy as np

EINVAL, ENOSPC = -22, -28
FRAME_BYTES = 56
SYMBOLS = ("aof_sequence_imu_device", "aof_sequence_imu_host")


class SeqImuParams(C.Structure):    # aof_seq_imu_params
    _fields_ = [("n_samples", C.c_int64), ("offset0", C.c_uint64), ("system_id", C.c_uint8), ("component_id", C.c_uint8),
                ("first_seq", C.c_uint8)]


def params(n_samples, offset0=0, system_id=1, component_id=100, first_seq=0):
    return SeqImuParams(int(n_samples), int(offset0), int(system_id), int(component_id), int(first_seq) & 0xFF)


def bind(aof):
    """aof.lib with the prototypes of the two calls set (idempotent)."""
    VP, P = C.c_void_p, C.POINTER
    lib = aof.lib
    sig = {
        "aof_sequence_imu_device": (C.c_int, [VP, P(aof.SequenceParams), P(SeqImuParams), C.c_int64, VP, VP, VP, VP, C.c_size_t, VP, VP]),
        "aof_sequence_imu_host": (C.c_int, [P(SeqImuParams), C.c_int64, VP, VP, VP, VP, VP, VP, VP, VP]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def _ptr(t):
    return None if t is None else t.data_ptr()


def device(aof, eng, sp, ip, n_frames, time_us, samples, sample_end, workspace, state=None, workspace_bytes=None):
    """aof_sequence_imu_device on torch's current stream.  time_us: int64 CUDA tensor [n]; samples: uint8 CUDA tensor [T, 24] or
    None; sample_end: int32 CUDA tensor [n] holding the u32 bits; workspace: the sequence call's uint8 tensor; state: uint8 CUDA
    tensor [64] or None.  Returns the call's code."""
    import torch
    stream = torch.cuda.current_stream(workspace.device).cuda_stream
    return bind(aof).aof_sequence_imu_device(eng._ctx, C.byref(sp), C.byref(ip), int(n_frames), time_us.data_ptr(), _ptr(samples),
                                             sample_end.data_ptr(), workspace.data_ptr(),
                                             workspace.numel() if workspace_bytes is None else workspace_bytes, _ptr(state), stream)


def host(aof, ip, n_frames, time_us, samples, sample_end, records, count, frames, frame_len, state=None):
    """aof_sequence_imu_host on numpy arrays, all changed in place: time_us uint64 [n]; samples the 24-byte sample records [T];
    sample_end uint32 [n]; records the 32-byte sequence records [n]; count uint32 [4]; frames uint8 [n, 56]; frame_len uint8 [n];
    state the 64-byte state record [1] or None.  Returns the call's code."""
    at = lambda a: None if a is None else a.ctypes.data
    for a in (time_us, samples, sample_end, records, count, frames, frame_len, state):
        assert a is None or a.flags.c_contiguous
    return bind(aof).aof_sequence_imu_host(None if ip is None else C.byref(ip), int(n_frames), at(time_us), at(samples), at(sample_end),
                                           at(records), at(count), at(frames), at(frame_len), at(state))


def limiter_slot_bytes(n_frames):
    """Bytes of each of the four limiter buffers at the start of aof_seq_layout.scratch, which the device call uses as its own."""
    return ((n_frames + 1) * 4 + 255) // 256 * 256


def up(torch, a, device):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(device)
