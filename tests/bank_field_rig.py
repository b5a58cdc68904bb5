"""The stream bank's motion field (include/aof.h, "the stream bank's motion field") for the tests and tools that drive it: the
ctypes records and prototypes of the three entry points of libaof and of the facade library's three shims, written ONCE
and here -- the package's surface (tests/golden/binding_surface.json) does not carry them yet --, thin callers over torch
tensors and numpy arrays, and where a bank keeps a tick's block records.  libaof's functions are bound on the package's own
handle (aof.lib); the facade's on a handle of this module's own."""
import ctypes as C

import numpy as np

STATE_DTYPE = np.dtype([("sum_zoom", "<f8"), ("sum_rotation", "<f8"), ("sum_centre_x", "<f8"), ("sum_centre_y", "<f8"),
                        ("pairs", "<u4"), ("fits", "<u4"), ("used", "<u4"), ("published", "<u4"), ("reserved", "u1", (16,))])   # aof_bank_field_state
RECORD_DTYPE = np.dtype([("status", "<i4"), ("dt_us", "<i4"), ("zoom", "<f4"), ("rotation", "<f4"), ("centre_x", "<f4"),
                         ("centre_y", "<f4"), ("flow_x", "<f4"), ("flow_y", "<f4"), ("pairs", "<u4"), ("fits", "<u4"),
                         ("used", "<u4"), ("frame", "<u4")])                                                                     # aof_bank_field_record
assert STATE_DTYPE.itemsize == 64 and RECORD_DTYPE.itemsize == 48
HELD, IDLE, STALE_GYRO, NO_OFFSET, BAD_SENSOR = -1, -2, -3, -4, -5
EINVAL, ENOSPC = -22, -28
SYMBOLS = ("aof_bank_field_reset_device", "aof_bank_field_device", "aof_bank_field_host")
FACADE_SYMBOLS = ("aof_facade_bank_enable_field", "aof_facade_bank_field_records", "aof_facade_bank_fields")

_facade = None


def bind(aof):
    """aof.lib with the prototypes of the three calls set (idempotent)."""
    VP, P = C.c_void_p, C.POINTER
    lib = aof.lib
    sig = {
        "aof_bank_field_reset_device": (C.c_int, [VP, C.c_int32, VP, VP, VP]),
        "aof_bank_field_device": (C.c_int, [VP, P(aof.BankParams), P(aof.FieldParams), VP, C.c_size_t, VP, VP, VP, VP, VP]),
        "aof_bank_field_host": (C.c_int, [P(aof.Params), P(aof.BankParams), VP, P(aof.FieldParams), VP, VP, VP, VP, VP, VP]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def facade(aof):
    """A handle of this module's own on the facade library, with the three shims' prototypes."""
    global _facade
    if _facade is None:
        f = C.CDLL(aof.FACADE_PATH)
        f.aof_facade_bank_enable_field.restype, f.aof_facade_bank_enable_field.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
        f.aof_facade_bank_field_records.restype, f.aof_facade_bank_field_records.argtypes = C.c_void_p, [C.c_void_p]
        f.aof_facade_bank_fields.restype, f.aof_facade_bank_fields.argtypes = C.c_void_p, [C.c_void_p]
        _facade = f
    return _facade


# ---- the facade's three methods on a Python OpticalFlowBank object (its handle) ---------------------------------------------
def enable_field(aof, bank, fp=None):
    return facade(aof).aof_facade_bank_enable_field(bank._h, C.addressof(fp) if fp is not None else None)


def _pinned(p, n, dtype):
    return None if not p else np.frombuffer((C.c_uint8 * (dtype.itemsize * n)).from_address(p), dtype=dtype).copy()


def field_records(aof, bank):
    """A copy of the last push's aof_bank_field_record [S], or None without enableField()."""
    return _pinned(facade(aof).aof_facade_bank_field_records(bank._h), bank.n_streams, RECORD_DTYPE)


def fields(aof, bank):
    """A copy of the last push's aof_field [S], or None without enableField()."""
    return _pinned(facade(aof).aof_facade_bank_fields(bank._h), bank.n_streams, aof.FIELD_DTYPE)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream(t):
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream


def reset(aof, eng, state, mask=None):
    """aof_bank_field_reset_device on torch's current stream: state uint8 CUDA tensor [S, 64]; returns the call's code."""
    return bind(aof).aof_bank_field_reset_device(eng._ctx, state.numel() // 64, _ptr(mask), state.data_ptr(), _stream(state))


def device(aof, eng, bp, buffer, records, state, out, fields=None, fp=None, bank_bytes=None):
    """aof_bank_field_device on torch's current stream: buffer the bank's uint8 tensor, records [S, 48], state [S, 64], out
    [S, 48], fields [S, 64] or None; returns the call's code."""
    fp = fp or aof.field_params()
    return bind(aof).aof_bank_field_device(eng._ctx, C.byref(bp), C.byref(fp), buffer.data_ptr(), buffer.numel() if bank_bytes is None else bank_bytes,
                                           records.data_ptr(), state.data_ptr(), _ptr(fields), out.data_ptr(), _stream(buffer))


def host(aof, p, bp, blocks, subdirs, records, state, streams=None, fp=None, want_fields=True):
    """aof_bank_field_host: blocks BLOCK_DTYPE [S, nb], subdirs uint8 [S, nb] or None, records TICK_DTYPE [S], state
    STATE_DTYPE [S] (stepped in place), streams BANK_STREAM records [S] or None -> (code, fields or None, out)."""
    S = bp.n_streams
    blocks, records = np.ascontiguousarray(blocks), np.ascontiguousarray(records)
    subdirs = None if subdirs is None else np.ascontiguousarray(subdirs)
    streams = None if streams is None else np.ascontiguousarray(streams)
    assert state.flags.c_contiguous and state.dtype == STATE_DTYPE
    fp = fp or aof.field_params()
    out, fld = np.zeros(S, RECORD_DTYPE), (np.zeros(S, aof.FIELD_DTYPE) if want_fields else None)
    at = lambda a: None if a is None else a.ctypes.data
    rc = bind(aof).aof_bank_field_host(C.byref(p), C.byref(bp), at(streams), C.byref(fp), at(blocks), at(subdirs), at(records), at(state),
                                       at(fld), at(out))
    return rc, fld, out


def scratch_offsets(aof, p, layout, n_streams):
    """(blocks, subdirs): byte offsets, inside a bank of `layout`, of the tick's level-0 records [S][nb] and sub-directions."""
    W = aof.workspace_layout(p, n_streams)
    return layout.scratch + W.l0_blocks, layout.scratch + W.l0_subdirs
