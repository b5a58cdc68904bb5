"""The sequence pipeline's MAVLink receive (include/aof_sequence_mavlink_rx.h) for the tests and tools that drive it: the ctypes
record and prototypes of the three entry points of libaof, written ONCE and here -- the package's surface
(tests/golden/binding_surface.json) does not carry them --, and thin callers over torch tensors and numpy arrays.  The
functions are bound on the package's own handle (aof.lib)."""
import ctypes as C

import numpy as np

EINVAL, ENOSPC, ENOMEM = -22, -28, -12
SYMBOLS = ("aof_sequence_mavlink_rx_scratch_bytes", "aof_sequence_mavlink_rx_device", "aof_sequence_mavlink_rx_host")


class SeqRxParams(C.Structure):    # aof_seq_rx_params
    _fields_ = [("n_bytes", C.c_int64), ("max_samples", C.c_int64)]


def params(n_bytes, max_samples):
    return SeqRxParams(int(n_bytes), int(max_samples))


def bind(aof):
    """aof.lib with the prototypes of the three calls set (idempotent)."""
    VP, P = C.c_void_p, C.POINTER
    lib = aof.lib
    sig = {
        "aof_sequence_mavlink_rx_scratch_bytes": (C.c_size_t, [C.c_int64]),
        "aof_sequence_mavlink_rx_device": (C.c_int, [VP, P(SeqRxParams), C.c_int64, VP, VP, VP, VP, VP, VP, C.c_size_t, VP]),
        "aof_sequence_mavlink_rx_host": (C.c_int, [P(SeqRxParams), C.c_int64, VP, VP, VP, VP, VP]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def scratch_bytes(aof, n_bytes):
    return int(bind(aof).aof_sequence_mavlink_rx_scratch_bytes(int(n_bytes)))


def _ptr(t):
    return None if t is None else t.data_ptr()


def device(aof, eng, rp, n_frames, log, byte_end, samples, sample_end, state, scratch, scratch_size=None):
    """aof_sequence_mavlink_rx_device on torch's current stream.  log: uint8 CUDA tensor (16-byte aligned) or None; byte_end,
    sample_end: int32 CUDA tensors [n] holding the u32 bits, or None; samples: uint8 CUDA tensor [max_samples, 24]; state: uint8
    CUDA tensor [128] or None; scratch: uint8 CUDA tensor, 256-byte aligned.  Returns the call's code."""
    import torch
    stream = torch.cuda.current_stream(scratch.device).cuda_stream
    return bind(aof).aof_sequence_mavlink_rx_device(eng._ctx, C.byref(rp), int(n_frames), _ptr(log), _ptr(byte_end), _ptr(samples),
                                                    _ptr(sample_end), _ptr(state), scratch.data_ptr(),
                                                    scratch.numel() if scratch_size is None else scratch_size, stream)


def host(aof, rp, n_frames, log, byte_end, samples, sample_end, state=None):
    """aof_sequence_mavlink_rx_host on numpy arrays: log uint8 [N]; byte_end, sample_end uint32 [n] or None; samples the 24-byte
    records [max_samples], written in place; state the 128-byte record [1] or None.  Returns the call's code."""
    at = lambda a: None if a is None else a.ctypes.data
    for a in (log, byte_end, samples, sample_end, state):
        assert a is None or a.flags.c_contiguous
    return bind(aof).aof_sequence_mavlink_rx_host(None if rp is None else C.byref(rp), int(n_frames), at(log), at(byte_end), at(samples),
                                                  at(sample_end), at(state))


def run_host(aof, log, byte_end, max_samples, fill, slots=None):
    """The host function on a case -> (samples as bytes [slots, 24] pre-filled with `fill`, sample_end uint32 [n], state bytes
    [128]); slots: the sample array's size (default max_samples)."""
    n = len(byte_end)
    samples = np.full((max_samples if slots is None else slots, 24), fill, np.uint8)
    sample_end = np.full(n, fill * 0x01010101, np.uint32)
    state = np.full(128, fill, np.uint8)
    rc = host(aof, params(len(log), max_samples), n, np.ascontiguousarray(log), np.ascontiguousarray(byte_end, np.uint32) if n else None,
              samples, sample_end if n else None, state)
    assert rc == 0, rc
    return samples, sample_end, state


def up(torch, a, device):
    if isinstance(a, (bytes, bytearray)):
        a = np.frombuffer(a, np.uint8)
    return torch.from_numpy(np.require(a, requirements="CW").view(np.uint8).reshape(-1)).to(device)
