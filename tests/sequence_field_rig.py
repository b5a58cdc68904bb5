"""The sequence pipeline's motion field (include/aof_sequence_field.h) for the tests and tools that drive it: the ctypes
prototypes of the two entry points of libaof, written ONCE and here -- the package's surface
(tests/golden/binding_surface.json) does not carry them --, thin callers over torch tensors and numpy arrays, and where a
sequence workspace keeps every pair's block records.  The functions are bound on the package's own handle (aof.lib)."""
import ctypes as C

import numpy as np

from bank_field_rig import RECORD_DTYPE, STATE_DTYPE   # noqa: F401  (aof_bank_field_record, aof_bank_field_state)

EINVAL, ENOSPC = -22, -28
SYMBOLS = ("aof_sequence_field_device", "aof_sequence_field_host")


def bind(aof):
    """aof.lib with the prototypes of the two calls set (idempotent)."""
    VP, P = C.c_void_p, C.POINTER
    lib = aof.lib
    sig = {
        "aof_sequence_field_device": (C.c_int, [VP, P(aof.SequenceParams), P(aof.FieldParams), C.c_int64, VP, C.c_size_t, VP, VP, VP, VP]),
        "aof_sequence_field_host": (C.c_int, [P(aof.Params), P(aof.SequenceParams), P(aof.FieldParams), C.c_int64, VP, VP, VP, VP,
                                              C.c_uint32, VP, VP, VP]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def _ptr(t):
    return None if t is None else t.data_ptr()


def device(aof, eng, sp, n_frames, workspace, fields, out, state=None, fp=None, workspace_bytes=None):
    """aof_sequence_field_device on torch's current stream.  workspace: the sequence call's uint8 tensor; fields: uint8 CUDA
    tensor [n - 1, 64] or None; out: uint8 CUDA tensor [n, 48]; state: uint8 CUDA tensor [64] or None.  Returns the call's
    code."""
    import torch
    fp = fp or aof.field_params()
    stream = torch.cuda.current_stream(workspace.device).cuda_stream
    return bind(aof).aof_sequence_field_device(eng._ctx, C.byref(sp), C.byref(fp), int(n_frames), workspace.data_ptr(),
                                               workspace.numel() if workspace_bytes is None else workspace_bytes, _ptr(fields),
                                               out.data_ptr(), _ptr(state), stream)


def host(aof, p, sp, n_frames, blocks, subdirs, flows, records, fp=None, want_state=True, fill=0):
    """aof_sequence_field_host on numpy arrays: blocks BLOCK_DTYPE [n - 1, nb], subdirs uint8 [n - 1, nb] or None, flows
    FLOW_DTYPE [n - 1], records the 32-byte sequence records [M] -> (code, fields [n - 1], out [M], state [1] or None), the
    outputs filled with `fill` beforehand."""
    at = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    pairs, M = max(int(n_frames) - 1, 0), len(records)
    blocks, flows, records = (None if a is None else np.ascontiguousarray(a) for a in (blocks, flows, records))
    subdirs = None if subdirs is None else np.ascontiguousarray(subdirs)
    fields = np.full(pairs * 64, fill, np.uint8).view(aof.FIELD_DTYPE)
    out = np.full(M * 48, fill, np.uint8).view(RECORD_DTYPE)
    state = np.full(64, fill, np.uint8).view(STATE_DTYPE) if want_state else None
    fp = fp or aof.field_params()
    rc = bind(aof).aof_sequence_field_host(C.byref(p), C.byref(sp), C.byref(fp), int(n_frames), at(blocks), at(subdirs), at(flows),
                                           at(records), M, at(fields), out.ctypes.data, None if state is None else state.ctypes.data)
    return rc, fields, out, state


def limiter_slot_bytes(n_frames):
    return ((n_frames + 1) * 4 + 255) // 256 * 256


def flow_workspace_offset(n_frames):
    """Offset, inside aof_seq_layout.scratch, of the flow engine's workspace for the n - 1 pairs: behind the limiter's four
    buffers, its rank words and its reached bytes."""
    return 5 * limiter_slot_bytes(n_frames) + (n_frames + 1 + 255) // 256 * 256


def block_offsets(aof, p, L, n_frames):
    """(blocks, subdirs): byte offsets, inside a sequence workspace of layout L, of the pairs' level-0 records [n - 1][nb] and
    sub-directions."""
    W = aof.workspace_layout(p, max(n_frames - 1, 0))
    at = L.scratch + flow_workspace_offset(n_frames)
    return at + W.l0_blocks, at + W.l0_subdirs


def up(torch, a, device):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(device)
