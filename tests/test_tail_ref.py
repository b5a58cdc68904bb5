"""The CPU side of the tail matrix (tests/tail_ref.py): the restated branch structure of aof_atan2f on its boundaries, the
steady frames, and -- on the ORACLE's records of every case, as the sequence pipeline and as the stream bank are fed
them -- the conditions that make tests/test_gpu_tail_matrix.py mean something: every branch is reached, with both
signs, behind windows of 75 frames and more.  On the exact (sum, focal) values the matrix publishes the host build of
aof_atan2f (aof.flow_angle) equals the oracle's restatement bit for bit and math.atan2 within the one float ulp
include/aof_math.h states for itself."""
import math
from collections import Counter

import numpy as np
import pytest

import tail_ref as tr
from npref import ulp_distance

F32 = np.float32


def test_angle_class_on_each_boundary():
    # t against tan(pi/8) = 0.41421356237...: the two floats around it (tests/test_math.py's pair)
    assert float(F32(0.41421354)) < tr.TAN_PI_8 < float(F32(0.4142136))
    for sign in (1, -1):
        assert tr.angle_class(sign * 0.41421354, 1.0) == ("direct", sign)
        assert tr.angle_class(sign * 0.4142136, 1.0) == ("reduced", sign)
    # px == focal, also where the focal length is no float: both are rounded to float first
    for focal in (1.0, 2.0, 216.6677, 216.2457):
        for sign in (1, -1):
            assert tr.angle_class(sign * float(F32(focal)), focal) == ("equal", sign)
            assert tr.angle_class(sign * float(np.nextafter(F32(focal), F32(0))), focal) == ("reduced", sign)
            assert tr.angle_class(sign * float(np.nextafter(F32(focal), F32(1e9))), focal) == ("swapped_reduced", sign)
    # |px| = focal / tan(pi/8) = (1 + sqrt 2) focal: the floats on both sides
    for focal in (1.0, 3.0, 0.25):
        edge = (1.0 + math.sqrt(2.0)) * focal
        below = F32(edge) if float(F32(edge)) < edge else np.nextafter(F32(edge), F32(0))
        above = np.nextafter(below, F32(1e9))
        assert float(below) < edge < float(above)
        for sign in (1, -1):
            assert tr.angle_class(sign * float(below), focal) == ("swapped_reduced", sign)
            assert tr.angle_class(sign * float(above), focal) == ("swapped_direct", sign)
    assert tr.angle_class(0.0, 2.0) == ("direct", 0) and tr.angle_class(-0.0, 0.5) == ("direct", 0)
    assert tr.angle_class(1e-30, 4000.0) == ("direct", 1) and tr.angle_class(-3.0, 0.25) == ("swapped_direct", -1)


@pytest.mark.parametrize("velocity", [(2, -2), (4, -3), (-1, 0)])
def test_steady_sequence_moves_by_whole_pixels_and_the_oracle_sees_them(aof, orc, velocity):
    vx, vy = velocity
    n, w, h = 6, 64, 64
    frames = tr.steady_sequence(w, h, n, velocity, 11)
    assert frames.shape == (n, h, w) and frames.dtype == np.uint8
    ys, xs = slice(max(0, -vy), h - max(0, vy)), slice(max(0, -vx), w - max(0, vx))
    yd, xd = slice(max(0, vy), h - max(0, -vy)), slice(max(0, vx), w - max(0, -vx))
    po = orc.params_from(aof.px4flow_params(w, h))
    flows = set()
    for k in range(n - 1):
        assert np.array_equal(frames[k + 1][ys, xs], frames[k][yd, xd]), k       # the window moved by (vx, vy)
        f = orc.flow_pair(po, frames[k], frames[k + 1])["flow"]
        assert f["quality"] > 0
        flows.add((float(f["flow_x"]), float(f["flow_y"])))
    assert len(flows) == 1 and all(v == int(v) for v in flows.pop()), "one whole-pixel flow for every pair"


def both(aof, orc, synth, case):
    return (("sequence", tr.oracle_of_sequence(aof, orc, synth, case)), ("bank", tr.oracle_of_bank(aof, orc, synth, case)))


@pytest.mark.parametrize("case", tr.CASES, ids=lambda c: c["id"])
def test_every_case_reaches_the_classes_its_row_names(aof, orc, synth, case):
    """(census() itself asserts that orc.angle of the recomputed float32 sums is the chain's angle, bit for bit.)"""
    for what, o in both(aof, orc, synth, case):
        assert len(o["sums"]) >= 3, what
        tr.check_reaches(case, o["counts"], o["sums"])


def test_the_matrix_reaches_every_class_with_both_signs(aof, orc, synth):
    for what in ("sequence", "bank"):
        seen, zero_behind_a_first_frame = Counter(), 0
        for case in tr.CASES:
            o = dict(both(aof, orc, synth, case))[what]
            seen.update(tr.by_class(o["counts"]))
            zero_behind_a_first_frame += sum(1 for m in o["sums"] if m[0] >= 1 and (float(m[1]) == 0.0 or float(m[2]) == 0.0))
        for cls in tr.CLASSES:
            for sign in (-1, 1):
                assert seen[(cls, sign)] >= 3, (what, cls, sign, dict(seen))
        assert seen[("equal", -1)] + seen[("equal", 1)] >= 10, (what, dict(seen))
        assert zero_behind_a_first_frame >= 1 and seen[("direct", 0)] >= 1, what


def test_the_slow_rate_windows_are_long(aof, orc, synth):
    case = tr.BY_ID["slow-rate"]
    for what, o in both(aof, orc, synth, case):
        long = [m for m in o["sums"] if m[3] >= 75 and abs(float(m[1])) > float(F32(case["fx"]))]
        assert len(long) >= 2, (what, o["sums"])


def test_the_host_build_equals_the_oracle_on_what_the_matrix_publishes(aof, orc, synth):
    pairs = set()
    for case in tr.CASES:
        for _, o in both(aof, orc, synth, case):
            for _, sx, sy, _ in o["sums"]:
                pairs.add((float(sx), float(F32(case["fx"]))))
                pairs.add((float(sy), float(F32(case["fy"]))))
    assert len(pairs) > 60 and {tr.angle_class(*p)[0] for p in pairs} == set(tr.CLASSES)
    for px, focal in sorted(pairs):
        got = F32(aof.flow_angle(px, focal))
        assert got.tobytes() == F32(orc.angle(px, focal)).tobytes(), (px, focal)
        assert ulp_distance(got, F32(math.atan2(px, focal))) <= 1, (px, focal, got)


def test_burst_run_keeps_every_streams_frames_in_order(aof, orc, synth):
    case = tr.BY_ID["short-focal"]
    run = tr.oracle_of_bank(aof, orc, synth, case)["run"]
    b, counts, given = tr.burst_run(run)
    K = tr.K_BURST
    assert (given > K).sum() == 1 and (np.minimum(given, K) == counts).all()
    for s in range(run.S):
        a0, a1 = run.active[:, s] == 1, b.active[:, s] == 1
        assert np.array_equal(run.frames[a0, s], b.frames[a1, s]) and np.array_equal(run.times[a0, s], b.times[a1, s])
        assert np.array_equal(run.gyro[a0, s], b.gyro[a1, s])
        for j in range(b.T // K):
            assert b.active[j * K:(j + 1) * K, s].tolist() == [1] * counts[j, s] + [0] * (K - counts[j, s])
    assert (counts == 0).any() and (counts == K).any() and b.T % K == 0
