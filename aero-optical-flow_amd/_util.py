"""What every wrapper of the binding does the same way, written once."""
from __future__ import annotations

import numpy as np

from ._abi import SEQ_FRAME_BYTES, AofError, lib


def check(rc):
    """The result of a library call that has no context: AofError for a negative one, else the value itself."""
    if rc < 0:
        raise AofError(rc, lib.aof_strerror(rc).decode())
    return rc


def ptr(t):
    """The address of a tensor's or a numpy array's memory; None for None."""
    return None if t is None else t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr()


def records_view(t, dtype, drop=1):
    """A tensor or array whose last axis holds one record each -> a structured numpy view without that axis (drop=0:
    the elements are the records themselves)."""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(dtype).reshape(a.shape[:a.ndim - drop])


def rounds_of(t):
    """(K, S, lead) of a record tensor [S, n] (a tick: K = 1) or [K, S, n] (a burst); lead: its shape without n."""
    K, S = (1, t.shape[0]) if t.dim() == 2 else (t.shape[0], t.shape[1])
    return K, S, tuple(t.shape[:-1])


def assert_mask(mask, S):
    """A reset's mask: None (all streams) or S contiguous bytes."""
    import torch
    assert mask is None or (mask.dtype == torch.uint8 and mask.numel() == S and mask.is_contiguous())


def mavlink_outputs(mavlink, frames, lengths, lead, dev, n=None):
    """The frames [lead, 56] / lengths [lead] outputs of a call that packs MAVLink frames: (None, None) unless `mavlink`;
    new zero-filled tensors where None is given; with n, what was given must hold n records (tensors, or numpy uint8
    arrays over device-mapped host memory)."""
    import torch
    if not mavlink:
        return None, None
    if frames is None:
        frames = torch.zeros(lead + (SEQ_FRAME_BYTES,), dtype=torch.uint8, device=dev)
    if lengths is None:
        lengths = torch.zeros(lead, dtype=torch.uint8, device=dev)
    if n is not None:
        for t, size in ((frames, n * SEQ_FRAME_BYTES), (lengths, n)):
            if isinstance(t, np.ndarray):
                assert t.dtype == np.uint8 and t.size == size and t.flags.c_contiguous
            else:
                assert t.dtype == torch.uint8 and t.is_contiguous() and t.numel() == size
    return frames, lengths
