"""The stream bank's motion field on the host (aof_bank_field_host, csrc/aof_bank_field.cpp over csrc/aof_bank_field_step.hpp)
against the numpy model (tests/bank_field_ref.py), byte for byte: a window of three pairs worked by hand, randomised runs
that mix every quality code, first frames, valid and invalid fits and per-stream focal lengths, the state of a stream
without a frame, and every refusal.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import bank_field_ref as bf
import bank_field_rig as rig
import field_ref as fr


def angle_of(aof):
    return lambda px, focal: np.float32(aof.lib.aof_flow_angle(px, focal))


def similarity_blocks(p, a, b, t):
    """Block records that hold the field U = t0 + a X - b Y, V = t1 + b X + a Y exactly (integers by choice of a, b, t)."""
    X, Y = fr.coordinates(p)
    U, V = t[0] + a * X - b * Y, t[1] + b * X + a * Y
    assert (U == np.rint(U)).all() and (V == np.rint(V)).all()
    return fr.records_of(U.astype(np.int64), V.astype(np.int64), 100)[0]


def test_a_window_of_three_pairs_by_hand(aof):
    """Dense 64 x 64 without half-pixels: 7 x 7 blocks at X, Y = -48 .. 48 in steps of 16 half-pixels, U and V even.  Three
    exact similarities: a zoom a = 1/8 (U = X/8, V = Y/8), a rotation b = -1/8 (U = Y/8, V = -X/8) and a shift of (6, 2)
    half-pixels.  Held, held, published at 66 667 us: the record carries the sums -- zoom 0.125, rotation -0.125, centre
    (3, 1) pixels, three fits of 49 blocks -- and the window starts over."""
    p = aof.default_params(64, 64)
    bp = aof.bank_params(1, focal_x=100.0, focal_y=50.0)
    state = np.zeros(1, rig.STATE_DTYPE)
    designs = [(1 / 8, 0.0, (0, 0)), (0.0, -1 / 8, (0, 0)), (0.0, 0.0, (6, 2))]
    qualities = [(bf.HELD, 0), (bf.HELD, 0), (180, 66667)]
    outs, flds = [], []
    for k, ((a, b, t), (q, dt)) in enumerate(zip(designs, qualities)):
        rec = np.zeros(1, bf.TICK_DTYPE)
        rec["quality"], rec["dt_us"], rec["frame"] = q, dt, k + 2
        rc, fld, out = rig.host(aof, p, bp, similarity_blocks(p, a, b, t)[None], None, rec, state)
        assert rc == 0
        outs.append(out[0])
        flds.append(fld[0])
        if k < 2:
            assert state["pairs"][0] == k + 1 and state["fits"][0] == k + 1 and state["used"][0] == 49 * (k + 1) and state["published"][0] == 0
    assert [float(f["zoom"]) for f in flds] == [0.125, 0.0, 0.0] and [float(f["rotation"]) for f in flds] == [0.0, -0.125, 0.0]
    assert [(float(f["centre_x"]), float(f["centre_y"])) for f in flds] == [(0.0, 0.0), (0.0, 0.0), (3.0, 1.0)]
    assert all(int(f["flags"]) == (fr.VALID | fr.REFIT) and int(f["used"]) == 49 for f in flds)
    for k in range(2):
        held = np.zeros((), rig.RECORD_DTYPE)
        held["status"], held["frame"] = bf.HELD, k + 2
        assert outs[k].tobytes() == held.tobytes()
    o = outs[2]
    assert (int(o["status"]), int(o["dt_us"]), int(o["pairs"]), int(o["fits"]), int(o["used"]), int(o["frame"])) == (3, 66667, 3, 3, 147, 4)
    assert (float(o["zoom"]), float(o["rotation"]), float(o["centre_x"]), float(o["centre_y"])) == (0.125, -0.125, 3.0, 1.0)
    assert o["flow_x"] == np.float32(aof.lib.aof_flow_angle(3.0, 100.0)) and o["flow_y"] == np.float32(aof.lib.aof_flow_angle(1.0, 50.0))
    assert abs(float(o["flow_x"]) - np.arctan2(3.0, 100.0)) < 1e-7 and abs(float(o["flow_y"]) - np.arctan2(1.0, 50.0)) < 1e-7
    want = np.zeros(1, rig.STATE_DTYPE)
    want["published"] = 1
    assert state.tobytes() == want.tobytes()


CONFIGS = {
    "dense-64": lambda aof: aof.default_params(64, 64),
    "px4-64": lambda aof: aof.px4flow_params(64, 64),                                        # sub-pixel: sub-directions reach the fit
    "opencv-128": lambda aof: aof.px4flow_params(128, 128, pyramid_levels=2, mean_subtract=1),
    "dense-144x136-subpixel": lambda aof: aof.default_params(144, 136, subpixel=1),
}


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("bound", [False, True], ids=["scalars", "stream-table"])
def test_host_equals_model_on_randomised_runs(aof, cfg, bound):
    p = CONFIGS[cfg](aof)
    S, T = 13, 14
    blocks, subdirs, records = bf.designed_run(p, S, T, seed=len(cfg))
    bp = aof.bank_params(S, focal_x=216.5, focal_y=180.25)
    focals = bf.focal_table(S, 3) if bound else np.tile(np.array([bp.focal_x, bp.focal_y], np.float32), (S, 1))
    streams = None
    if bound:
        streams = aof.bank_stream_from_params(bp, S)
        streams["focal_x"], streams["focal_y"] = focals[:, 0], focals[:, 1]
    angle = angle_of(aof)
    got_state, want_state = np.zeros(S, rig.STATE_DTYPE), np.zeros(S, rig.STATE_DTYPE)
    got_state["reserved"] = want_state["reserved"] = 0xA5        # (passes through: the step keeps what it does not own)
    seen_q, seen_flags, first_frames, windows = set(), set(), 0, set()
    for t in range(T):
        before = got_state.copy()
        rc, fld, out = rig.host(aof, p, bp, blocks[t], subdirs[t], records[t], got_state, streams=streams)
        assert rc == 0
        wf, wo = bf.step(p, focals, blocks[t], subdirs[t], records[t], want_state, angle)
        assert fld.tobytes() == wf.tobytes(), (t, [(s, fld[s], wf[s]) for s in range(S) if fld[s] != wf[s]][:2])
        assert out.tobytes() == wo.tobytes(), (t, [(s, out[s], wo[s]) for s in range(S) if out[s] != wo[s]][:2])
        assert got_state.tobytes() == want_state.tobytes(), t
        for s in range(S):
            q = int(records[t, s]["quality"])
            seen_q.add(min(q, 0) if q < 0 else 1)
            if bf.no_frame(q):
                assert got_state[s].tobytes() == before[s].tobytes() and not np.frombuffer(fld[s].tobytes(), np.uint8).any()
            elif bf.ran_pair(records[t, s]):
                seen_flags.add(int(fld[s]["flags"]) & fr.VALID)
            else:
                first_frames += 1
            if int(out[s]["status"]) >= 0:
                windows.add(int(out[s]["pairs"]))
        # fields = NULL: records and state the same
        again = before.copy()
        rc, none, out2 = rig.host(aof, p, bp, blocks[t], subdirs[t], records[t], again, streams=streams, want_fields=False)
        assert rc == 0 and none is None and out2.tobytes() == out.tobytes() and again.tobytes() == got_state.tobytes()
    assert seen_q == {1, bf.HELD, bf.IDLE, bf.STALE_GYRO, bf.NO_OFFSET, bf.BAD_SENSOR}
    assert seen_flags == {0, fr.VALID} and first_frames >= S and {0, 1, 2} <= windows, (seen_flags, first_frames, windows)


def test_subdirs_are_ignored_without_a_subpixel_context(aof):
    p = aof.default_params(64, 64)
    assert not p.subpixel
    blocks, subdirs, records = bf.designed_run(p, 4, 3, seed=1)
    bp = aof.bank_params(4)
    a, b = np.zeros(4, rig.STATE_DTYPE), np.zeros(4, rig.STATE_DTYPE)
    for t in range(3):
        _, f1, o1 = rig.host(aof, p, bp, blocks[t], subdirs[t], records[t], a)
        _, f2, o2 = rig.host(aof, p, bp, blocks[t], None, records[t], b)
        assert f1.tobytes() == f2.tobytes() and o1.tobytes() == o2.tobytes()


def test_every_refusal(aof):
    p = aof.default_params(64, 64)
    bp, fp = aof.bank_params(2), aof.field_params()
    blocks, subdirs, records = bf.designed_run(p, 2, 1)
    state, out, fld = np.full(2, 0, rig.STATE_DTYPE), np.zeros(2, rig.RECORD_DTYPE), np.zeros(2, aof.FIELD_DTYPE)
    for a in (state, out, fld):
        a.view(np.uint8)[:] = 0xEE
    lib = rig.bind(aof)
    good = [C.byref(p), C.byref(bp), None, C.byref(fp), blocks[0].ctypes.data, subdirs[0].ctypes.data, records[0].ctypes.data,
            state.ctypes.data, fld.ctypes.data, out.ctypes.data]
    bad = []
    for i in (0, 1, 3, 4, 6, 7, 9):                                     # NULL p, bp, fp, blocks, records, state, out
        a = list(good)
        a[i] = None
        bad.append(a)
    bad.append(good[:1] + [C.byref(aof.bank_params(0))] + good[2:])
    bad.append(good[:1] + [C.byref(aof.bank_params(-3))] + good[2:])
    for kw in (dict(min_blocks=2), dict(passes=3), dict(passes=0), dict(exclude_reach=2), dict(gate_px=0.0), dict(gate_px=float("nan")),
               dict(gate_px=float("inf"))):
        bad.append(good[:3] + [C.byref(aof.field_params(**kw))] + good[4:])
    wide = aof.default_params(8192, 2048)                               # a grid beyond the fit's integer range
    assert aof.check_params(wide) == 0 and not aof.field_supported(wide)
    bad.append([C.byref(wide)] + good[1:])
    broken = aof.default_params(64, 64)
    broken.tile = 5
    bad.append([C.byref(broken)] + good[1:])
    for a in bad:
        assert lib.aof_bank_field_host(*a) == rig.EINVAL, a
    assert all((a.view(np.uint8) == 0xEE).all() for a in (state, out, fld))
    # without a context the device calls answer -EINVAL whatever else is passed
    assert lib.aof_bank_field_device(None, C.byref(bp), C.byref(fp), state.ctypes.data, 64, state.ctypes.data, state.ctypes.data, None,
                                     out.ctypes.data, None) == rig.EINVAL
    assert lib.aof_bank_field_reset_device(None, 2, None, state.ctypes.data, None) == rig.EINVAL
    assert all((a.view(np.uint8) == 0xEE).all() for a in (state, out, fld))
    state.view(np.uint8)[:] = 0
    assert lib.aof_bank_field_host(*good) == 0
