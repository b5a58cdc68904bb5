"""aof_sequence_field_host (include/aof_sequence_field.h) against the sequential model of tests/sequence_field_ref.py, byte for
byte; the model against the closed form the kernels compute and against a window worked by hand; the host function against
aof_bank_field_host driven as one stream, a tick per frame, on the ORACLE's blocks of a climbing and yawing recording; every
refusal; and the conditions the GPU end-to-end cases (tests/test_gpu_sequence_field.py) rest on.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import bank_field_ref as bf
import bank_field_rig as bank_rig
import field_ref as fr
import sequence_field_ref as ref
import sequence_field_rig as rig
from bank_ref import FX, FY, oracle_chain
from sequence_ref import crop_of

FILL = 0xEE
FOCAL = np.array([FX, FY], np.float32)


def similarity_blocks(p, a, b, t):
    """Block records that hold the field U = t0 + a X - b Y, V = t1 + b X + a Y exactly (integers by choice of a, b, t)."""
    X, Y = fr.coordinates(p)
    U, V = t[0] + a * X - b * Y, t[1] + b * X + a * Y
    assert (U == np.rint(U)).all() and (V == np.rint(V)).all()
    return fr.records_of(U.astype(np.int64), V.astype(np.int64), 100)[0]


def angle_of(aof):
    return lambda px, focal: np.float32(aof.lib.aof_flow_angle(px, focal))


def differing(got, want):
    return [(i, got[i], want[i]) for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()][:2]


# ---- the model against itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [0, 1, 5000], ids=["no-tail", "tail-1", "tail-5000"])
def test_the_closed_form_equals_the_sequential_model(aof, tail):
    """Every window length of the list among short random windows, fits without AOF_FIELD_VALID interleaved, two windows with
    no valid fit at all."""
    angle = angle_of(aof)
    records_seen, lengths = 0, set()
    for seed in range(3):
        rng = np.random.default_rng([seed, tail])
        windows = list(ref.WINDOW_LENGTHS if seed == 0 else ref.WINDOW_LENGTHS[:-1]) + ref.random_windows(rng, 40 + 30 * seed)
        rng.shuffle(windows)
        records, n = ref.record_list(windows, tail, seed)
        fields = ref.random_fields(n - 1, seed)
        ref.invalidate(fields, records, [3, 17])
        a_out, a_state = ref.integrate(fields, records, n, FOCAL, angle)
        b_out, b_state = ref.closed_form(fields, records, n, FOCAL, angle)
        assert a_out.tobytes() == b_out.tobytes(), (seed, differing(a_out, b_out))
        assert a_state.tobytes() == b_state.tobytes(), (seed, a_state, b_state)
        assert int(a_state["pairs"][0]) == tail and int(a_state["published"][0]) == len(records)
        assert [int(a_out[m]["status"]) for m in (3, 17)] == [0, 0] and (a_out["pairs"][1:] == np.array(windows)).all()
        assert (a_out["fits"] < a_out["pairs"]).any() and (a_out["fits"] > 0).any()
        records_seen += len(records)
        lengths |= set(windows)
    assert set(ref.WINDOW_LENGTHS) <= lengths and records_seen > 150


def test_records_of_every_frame_have_windows_of_one_pair(aof):
    """output_rate <= 0: a record per frame."""
    records, n = ref.record_list([1] * 30, 0)
    fields = ref.random_fields(n - 1, 4)
    out, state = ref.integrate(fields, records, n, FOCAL, angle_of(aof))
    assert (out["pairs"][1:] == 1).all() and out["pairs"][0] == 0 and int(out[0]["status"]) == 0
    valid = (fields["flags"] & fr.VALID) != 0
    assert out["zoom"][1:][valid].tobytes() == fields["zoom"][valid].tobytes() and not out["zoom"][1:][~valid].any()
    assert out["frame"].tolist() == list(range(31)) and not state["pairs"][0]


# ---- a window by hand -------------------------------------------------------------------------------------------------------------
def hand_recording(aof):
    """Dense 64 x 64 without half-pixels (7 x 7 blocks, X and Y multiples of 16 half-pixels).  Six frames, five pairs: a zoom
    a = 1/8, a pair nobody accepts, a rotation b = -1/8, a shift of (6, 2) half-pixels -- the window of the record at frame 4
    --, then another zoom of 1/8 behind it: the tail."""
    p = aof.default_params(64, 64)
    designs = [(1 / 8, 0.0, (0, 0)), None, (0.0, -1 / 8, (0, 0)), (0.0, 0.0, (6, 2)), (1 / 8, 0.0, (0, 0))]
    blocks = np.zeros((5, 49), fr.BLOCK_DTYPE)
    for k, d in enumerate(designs):
        if d is None:
            blocks[k]["sad"] = fr.SKIPPED
        else:
            blocks[k] = similarity_blocks(p, *d)
    records = np.zeros(2, ref.SEQ_RECORD_DTYPE)
    records["frame"], records["quality"], records["dt_us"] = [0, 4], [0, bf.STALE_GYRO], [0, 53333]
    return p, blocks, np.zeros(5, fr.FLOW_DTYPE), records


def test_a_window_of_four_pairs_by_hand(aof):
    p, blocks, flows, records = hand_recording(aof)
    sp = aof.sequence_params(64, 64, 64, 64, 100.0, 50.0, 15)
    focal = np.array([100.0, 50.0], np.float32)
    for fields, out, state in (ref.run(p, blocks, None, flows, records, 6, focal, angle_of(aof)),
                               rig.host(aof, p, sp, 6, blocks, None, flows, records)[1:]):
        assert [int(f["flags"]) & fr.VALID for f in fields] == [1, 0, 1, 1, 1]
        first = np.zeros((), rig.RECORD_DTYPE)
        assert out[0].tobytes() == first.tobytes(), "frame 0: an empty window, published, all zero"
        o = out[1]
        assert (int(o["status"]), int(o["dt_us"]), int(o["pairs"]), int(o["fits"]), int(o["used"]), int(o["frame"])) == (3, 53333, 4, 3, 147, 4)
        assert (float(o["zoom"]), float(o["rotation"]), float(o["centre_x"]), float(o["centre_y"])) == (0.125, -0.125, 3.0, 1.0)
        assert o["flow_x"] == np.float32(aof.lib.aof_flow_angle(3.0, 100.0)) and o["flow_y"] == np.float32(aof.lib.aof_flow_angle(1.0, 50.0))
        s = state[0]
        assert (float(s["sum_zoom"]), float(s["sum_rotation"]), float(s["sum_centre_x"]), float(s["sum_centre_y"])) == (0.125, 0.0, 0.0, 0.0)
        assert (int(s["pairs"]), int(s["fits"]), int(s["used"]), int(s["published"])) == (1, 1, 49, 2) and not s["reserved"].any()


# ---- the host function against the model ---------------------------------------------------------------------------------------------
CONFIGS = {
    "px4-64": lambda aof: aof.px4flow_params(64, 64),                                        # 25 blocks, sub-pixel
    "dense-64": lambda aof: aof.default_params(64, 64),                                      # no sub-directions
    "opencv-128": lambda aof: aof.px4flow_params(128, 128, pyramid_levels=2, mean_subtract=1),
}


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_the_host_function_equals_the_model(aof, cfg):
    p = CONFIGS[cfg](aof)
    sp = aof.sequence_params(p.width, p.height, p.width, p.height, FX, FY, 15)
    rng = np.random.default_rng(len(cfg))
    windows = [5, 1, 64, 2, 65, 63] + ref.random_windows(rng, 20)
    for tail in (0, 7):
        records, n = ref.record_list(windows, tail, seed=tail)
        F = records["frame"]
        blocks, subdirs, flows = ref.designed_pairs(p, n - 1, seed=tail, invalid_spans=[(int(F[2]), int(F[3])), (int(F[8]), int(F[9]))])
        w_fields, w_out, w_state = ref.run(p, blocks, subdirs, flows, records, n, FOCAL, angle_of(aof))
        rc, fields, out, state = rig.host(aof, p, sp, n, blocks, subdirs, flows, records, fill=FILL)
        assert rc == 0
        assert fields.tobytes() == w_fields.tobytes(), differing(fields, w_fields)
        assert out.tobytes() == w_out.tobytes(), differing(out, w_out)
        assert state.tobytes() == w_state.tobytes(), (state, w_state)
        assert int(out[3]["status"]) == 0 and int(out[3]["pairs"]) == 64 and int(out[9]["status"]) == 0
        assert (out["status"] > 0).sum() > len(out) // 2 and {0, fr.VALID} == set((fields["flags"] & fr.VALID).tolist())
        # without a state, and with the sub-directions a configuration without sub-pixel search must not look at
        rc, f2, o2, none = rig.host(aof, p, sp, n, blocks, subdirs if p.subpixel else None, flows, records, want_state=False)
        assert rc == 0 and none is None and f2.tobytes() == fields.tobytes() and o2.tobytes() == out.tobytes()


def test_one_frame_and_no_frames(aof):
    p = aof.px4flow_params(64, 64)
    sp = aof.sequence_params(64, 64, 64, 64, FX, FY, 15)
    records, n = ref.record_list([], 0)
    assert n == 1
    rc, fields, out, state = rig.host(aof, p, sp, 1, None, None, None, records, fill=FILL)
    want = np.zeros(1, rig.STATE_DTYPE)
    want["published"] = 1
    first = np.zeros(1, rig.RECORD_DTYPE)
    first["dt_us"] = records["dt_us"]
    assert rc == 0 and fields.size == 0 and out.tobytes() == first.tobytes() and state.tobytes() == want.tobytes()
    rc, _, out, state = rig.host(aof, p, sp, 0, None, None, None, records[:0], fill=FILL)
    assert rc == 0 and (state.view(np.uint8) == FILL).all(), "no frames: nothing to do"
    rc, _, out, state = rig.host(aof, p, sp, 1, None, None, None, records[:0], fill=FILL)
    assert rc == 0 and not state.view(np.uint8).any(), "a frame nobody published: a zero state"


# ---- against the stream bank's host function, a tick per frame, on the oracle's blocks ------------------------------------------------
_oracle_runs = {}


def oracle_run(aof, orc, synth, name):
    """The recording of an end-to-end case through the oracle: (p, n, blocks, subdirs, flows, ticks TICK_DTYPE [n], records)."""
    if name not in _oracle_runs:
        case = ref.E2E[name]
        p = ref.e2e_params(aof, case)
        frames, times = ref.e2e_recording(synth, case)
        cropped = crop_of(frames, *case["crop"])
        n, nb = case["n"], fr.coordinates(p)[0].size
        po = orc.params_from(p)
        chain = oracle_chain(aof, orc, p, case["rate"], 0, 0, use_gyro=False)
        blocks, subdirs = np.zeros((n - 1, nb), fr.BLOCK_DTYPE), np.zeros((n - 1, nb), np.uint8)
        ticks = np.zeros(n, aof.TICK_DTYPE)
        for j in range(n):
            if j:
                r = orc.flow_pair(po, cropped[j - 1], cropped[j])
                blocks[j - 1], subdirs[j - 1] = r["blocks"], r["subdirs"]
            ticks[j], _ = chain.push(cropped[j], times[j], np.zeros(4, np.float32))
        published = np.flatnonzero(ticks["quality"] >= 0)
        records = np.zeros(len(published), ref.SEQ_RECORD_DTYPE)
        records["frame"] = published
        for f in ("quality", "dt_us", "flow_x", "flow_y"):
            records[f] = ticks[f][published]
        _oracle_runs[name] = (p, n, blocks, subdirs, ticks["pixel"][1:].copy(), ticks, records)
    return _oracle_runs[name]


@pytest.mark.parametrize("name", ["px4-64-rate15", "opencv-128-two-levels"])
def test_the_host_function_equals_the_bank_host_function_driven_frame_by_frame(aof, orc, synth, name):
    p, n, blocks, subdirs, flows, ticks, records = oracle_run(aof, orc, synth, name)
    sp = aof.sequence_params(p.width, p.height, p.width, p.height, FX, FY, ref.E2E[name]["rate"])
    rc, fields, out, state = rig.host(aof, p, sp, n, blocks, subdirs, flows, records)
    assert rc == 0
    bp = aof.bank_params(1, FX, FY, ref.E2E[name]["rate"], 0, 1, 100, 0)
    bank_state = np.zeros(1, bank_rig.STATE_DTYPE)
    m = 0
    zero = np.zeros((1, blocks.shape[1]), fr.BLOCK_DTYPE)
    for j in range(n):
        rc, f, o = bank_rig.host(aof, p, bp, blocks[j - 1:j] if j else zero, subdirs[j - 1:j] if j else None, ticks[j:j + 1], bank_state)
        assert rc == 0 and int(o[0]["frame"]) == j + 1
        if j:
            assert f[0].tobytes() == fields[j - 1].tobytes(), (j, "the pair's fit")
        if int(o[0]["status"]) >= 0:
            want = o[0].copy()
            want["frame"] = j                     # the sequence counts frames from 0, the bank from 1
            assert out[m].tobytes() == want.tobytes(), (m, out[m], want)
            m += 1
    assert m == len(records) >= 3 and state.tobytes() == bank_state.tobytes()
    if p.pyramid_levels == 2:
        assert (subdirs < 8).any() and ((flows["pred_x"] != 0) | (flows["pred_y"] != 0)).any(), "sub-directions and predictors reach the fit"


@pytest.mark.parametrize("name", list(ref.E2E))
def test_the_end_to_end_cases_do_not_pass_on_zeros(aof, orc, synth, name):
    """What the GPU cases rest on: most published records carry a fit, and a zoom or rotation that is not zero."""
    p, n, blocks, subdirs, flows, ticks, records = oracle_run(aof, orc, synth, name)
    sp = aof.sequence_params(p.width, p.height, p.width, p.height, FX, FY, ref.E2E[name]["rate"])
    rc, fields, out, state = rig.host(aof, p, sp, n, blocks, subdirs, flows, records)
    assert rc == 0 and len(out) >= 3
    assert 2 * int((out["status"] >= 1).sum()) >= len(out), out["status"]
    assert (out["zoom"] != 0).any() or (out["rotation"] != 0).any()
    if ref.E2E[name]["rate"] > 0:
        assert int(out["pairs"].max()) >= 3, "windows of several pairs"
    else:
        assert len(out) == n


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_host_function_writes_nothing(aof):
    p = aof.px4flow_params(64, 64)
    sp, fp = aof.sequence_params(64, 64, 64, 64, FX, FY, 15), aof.field_params()
    records, n = ref.record_list([2, 3, 1], 2)
    blocks, subdirs, flows = ref.designed_pairs(p, n - 1)
    blocks, subdirs = np.ascontiguousarray(blocks), np.ascontiguousarray(subdirs)
    fields, out, state = np.zeros(n - 1, aof.FIELD_DTYPE), np.zeros(len(records), rig.RECORD_DTYPE), np.zeros(1, rig.STATE_DTYPE)
    for a in (fields, out, state):
        a.view(np.uint8)[:] = FILL
    lib = rig.bind(aof)
    good = [C.byref(p), C.byref(sp), C.byref(fp), n, blocks.ctypes.data, subdirs.ctypes.data, flows.ctypes.data, records.ctypes.data,
            len(records), fields.ctypes.data, out.ctypes.data, state.ctypes.data]
    bad = []
    for i in (0, 1, 2, 4, 6, 7, 9, 10):                                  # NULL p, sp, fp, blocks, flows, records, fields, out
        a = list(good)
        a[i] = None
        bad.append(a)
    for count in (-1, 0x7FFFFFF0, len(records) - 1):                     # frames: negative, too many, fewer than records
        bad.append(good[:3] + [count] + good[4:])
    for kw in (dict(min_blocks=2), dict(passes=3), dict(exclude_reach=2), dict(gate_px=0.0), dict(gate_px=float("nan"))):
        bad.append(good[:2] + [C.byref(aof.field_params(**kw))] + good[3:])
    wide = aof.default_params(8192, 2048)                                # a grid beyond the fit's integer range
    bad.append([C.byref(wide)] + good[1:])
    bad.append(good[:1] + [C.byref(aof.sequence_params(64, 64, 64, 64, 0.0, FY, 15))] + good[2:])
    for frames in ([0, 2, 2, 6], [0, 5, 3, 6], [0, 2, 5, n]):            # a frame twice, out of order, behind the recording
        r2 = records.copy()
        r2["frame"] = frames
        bad.append((good[:7] + [r2.ctypes.data] + good[8:], r2))
    for a in bad:
        a = a[0] if isinstance(a, tuple) else a
        assert lib.aof_sequence_field_host(*a) == rig.EINVAL, a
    assert all((a.view(np.uint8) == FILL).all() for a in (fields, out, state))
    # without a context the device call answers -EINVAL whatever else is passed
    assert lib.aof_sequence_field_device(None, C.byref(sp), C.byref(fp), n, state.ctypes.data, 1 << 20, fields.ctypes.data, out.ctypes.data,
                                         state.ctypes.data, None) == rig.EINVAL
    assert all((a.view(np.uint8) == FILL).all() for a in (fields, out, state))
    assert lib.aof_sequence_field_host(*good) == 0 and int(state["published"][0]) == len(records)
