"""The reference's per-frame loop around a calcFlow implementation, over one recording: what the sequence pipeline's
tests (tests/test_gpu_sequence.py, tests/tail_ref.py) expect.  Nothing here touches the GPU."""
import numpy as np


def crop_of(frames, cw, ch):
    n, H, W = frames.shape
    x0, y0 = W // 2 - cw // 2, H // 2 - ch // 2            # mainloop.cpp:295-297
    return np.ascontiguousarray(frames[:, y0:y0 + ch, x0:x0 + cw])


def replay(calc_flow, cropped, times, gyro, offset, first_seq, pack):
    """mainloop.cpp:322-373 around a calcFlow implementation: the negative-return gate, the gyro taken and
    zeroed with every published flow, the field mapping and the frame."""
    recs, wire = [], []
    g = np.zeros(3, np.float64)
    seq = first_seq
    for k in range(len(times)):
        g += gyro[k, :3].astype(np.float64)                 # integrated since the last message (:383-405)
        q, dt, ax, ay = calc_flow(cropped[k], int(times[k]) & 0xFFFFFFFF)
        if q < 0:                                           # :327-331
            continue
        taken, g = g.copy(), np.zeros(3, np.float64)        # :333-334
        recs.append((k, q, dt, np.float32(ax), np.float32(ay), np.float32(taken[0]), np.float32(taken[1]), np.float32(taken[2])))
        if offset:                                          # :353-357
            wire.append(pack(offset, int(times[k]), dt, float(np.float32(ax)), float(np.float32(ay)),
                             tuple(float(v) for v in taken), q, seq & 0xFF))
            seq += 1
    return recs, wire
