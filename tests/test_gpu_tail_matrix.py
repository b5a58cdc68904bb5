"""Every device tail -- k_sequence_emit (aof_sequence_device) and bank_tail_step under the tick, the burst and their camera
forms, one-launch and composed -- on the cases of tests/tail_ref.py: focal lengths, output rates and motions that take
aof_atan2f (include/aof_math.h) through its argument reduction, its lo == hi case and its swap with both signs, and the
limiter through windows of 75 frames and more.  Records and MAVLink frames byte for byte against the CPU oracle's chain
with the independent serializer of tests/mavlink_model.py, for two cases also against the C++ facade driven frame by frame;
the de-rotated flows against orc.derotate at the case's focal lengths.  Every case first asserts, on the oracle's
records and before the device runs, that its input reaches the branches it is there for."""
import numpy as np
import pytest

import bank_camera_ref as cref
import tail_ref as tr
from bank_cases import Case, run_camera_case, run_case
from bank_rig import time_limit   # (this module's fixture too: every test under a limit of its own)
from sequence_ref import replay

pytestmark = pytest.mark.gpu

DEROTATE = (4.5, 0.01)          # the sequence pipeline's, as tests/test_gpu_sequence.py sets it
SENSOR, SKEW = (160, 120), 1    # the camera forms: the crop origin 28 * 160 + 48 (+ 1) is an odd byte of the allocation
CAMERA_CASES = [c for c in tr.CASES if c.get("camera")]
ids = lambda c: c["id"]


def bits(values):
    return b"".join(np.float32(v).tobytes() for v in values)


@pytest.mark.parametrize("case", tr.CASES, ids=ids)
def test_sequence_pipeline(aof, orc, synth, gpu_device, case):
    import torch
    o = tr.oracle_of_sequence(aof, orc, synth, case)
    tr.check_reaches(case, o["counts"], o["sums"])                      # on the oracle, before the device
    fx, fy, rate, n = case["fx"], case["fy"], case["rate"], case["n"]
    frames, times, gyro, cropped = o["frames"], o["times"], o["gyro"], o["cropped"]
    p = tr.params_of(aof, case["cfg"])
    cam_w, cam_h = tr.sensor_of(case["cfg"])
    first_seq = 250
    eng = aof.FlowEngine(p, 0)
    sp = aof.sequence_params(cam_w, cam_h, p.width, p.height, fx, fy, rate, tr.OFFSET, 1, 100, first_seq, derotate=DEROTATE)
    ws, L = eng.sequence(sp, torch.from_numpy(frames).to(gpu_device), torch.from_numpy(times).to(gpu_device),
                         torch.from_numpy(gyro).to(gpu_device))
    torch.cuda.synchronize()
    out = eng.sequence_outputs(sp, ws, L, n)
    assert out["status"] == 0
    assert np.array_equal(out["cropped"], cropped)

    refs = [(o["recs"], o["wire"], "oracle")]
    if case.get("facade"):
        cls = aof.OpticalFlowPX4 if p.pyramid_levels == 1 else aof.OpticalFlowOpenCV
        fac = cls(fx, fy, rate, p.width, p.height)
        refs.append(replay(fac.calcFlow, cropped, times, gyro, tr.OFFSET, first_seq, aof.pack_optical_flow_rad) + ("facade",))
        fac.close()
    got = out["records"]
    for recs, wire, name in refs:
        assert len(got) == len(recs) >= 4, name
        for m, r in enumerate(recs):
            g = got[m]
            assert (int(g["frame"]), int(g["quality"]), int(g["dt_us"])) == r[:3], (name, m, g, r)
            assert bits(g[f] for f in ("flow_x", "flow_y", "gyro_x", "gyro_y", "gyro_z")) == bits(r[3:]), (name, m, g, r)
        assert out["frames_sent"] == len(wire) and out["mavlink"] == wire, f"device frames differ from the {name}'s"

    po = orc.params_from(p)
    for k in range(n - 1):
        f = out["flows"][k]
        assert f.tobytes() == orc.flow_pair(po, cropped[k], cropped[k + 1])["flow"].tobytes(), k
        want = orc.derotate(float(f["flow_x"]), float(f["flow_y"]), float(gyro[k + 1, 0]), float(gyro[k + 1, 1]),
                            float(gyro[k + 1, 3]), fx, fy, *DEROTATE)
        assert np.asarray(want, np.float32).tobytes() == out["derotated"][k].tobytes(), k
    moved = out["derotated"] != np.stack([out["flows"]["flow_x"], out["flows"]["flow_y"]], -1)
    assert moved.any(), "some pair is compensated"
    eng.close()


def bank_oracle(aof, orc, synth, case):
    o = tr.oracle_of_bank(aof, orc, synth, case)
    tr.check_reaches(case, o["counts"], o["sums"])                      # on the oracle, before the device
    return o


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("case", tr.CASES, ids=ids)
def test_bank_tick(aof, orc, synth, gpu_device, case, path):
    """aof_bank_push_device, one launch (path 1) and composed (path 2): S streams that join at different ticks, synchronised
    once per tick; on path 1 the facade cases also against one facade object per stream."""
    o = bank_oracle(aof, orc, synth, case)
    p = tr.params_of(aof, case["cfg"])
    want = run_case(aof, orc, synth, gpu_device, case["cfg"], case["S"], case["T"], case["seed"], rate=case["rate"], path=path,
                    facade=case["S"] if case.get("facade") and path == 1 else 0, fx=case["fx"], fy=case["fy"],
                    source=tr.stream_source(case, p.width, p.height))
    assert want.tobytes() == o["want"].tobytes(), "the run that was compared is the run of the census"


def burst_case(aof, orc, synth, case, o, path, camera):
    run = o["run"]
    b, counts, given = tr.burst_run(run)
    c = Case(aof, orc, synth, case["cfg"], tr.K_BURST, S=run.S, B=b.T // tr.K_BURST, seed=case["seed"], camera=camera,
             rate=case["rate"], path=path, fx=case["fx"], fy=case["fy"], burst_run=(b, counts, given),
             sensor=SENSOR if camera else None, skew=SKEW if camera else 0,
             needs=("first-frame-then-more", "count0") + (("crop-origin-on-an-odd-byte",) if camera else ()))
    for s in range(run.S):      # stream by stream the chain saw what the census saw, and left the same records
        assert c.want[b.active[:, s] == 1, s].tobytes() == o["want"][run.active[:, s] == 1, s].tobytes(), s
    return c


def run_bursts(c, orc, gpu_device):
    eng = c.engine()
    dev = c.burst_device(eng, gpu_device)
    for j in range(c.B):
        got = dev.push(j, c.given, c.sensors(j))
        c.check_against_oracle(j, got, orc)
        if c.camera:
            assert dev.gate_bytes().tolist() == c.after[(j + 1) * c.K - 1].tolist(), ("gate", j)
    eng.close()


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("case", tr.CASES, ids=ids)
def test_bank_burst(aof, orc, synth, gpu_device, case, path):
    """aof_bank_push_burst_device with K = 5 over the same streams, in its one-launch and its composed form."""
    o = bank_oracle(aof, orc, synth, case)
    run_bursts(burst_case(aof, orc, synth, case, o, path, camera=False), orc, gpu_device)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("case", CAMERA_CASES, ids=ids)
def test_camera_tick(aof, orc, synth, gpu_device, case, path):
    """aof_bank_push_camera_device on 160 x 120 sensor frames: records, frames, exposure records and the de-rotated pairs
    (orc.derotate at the case's focal lengths) against the oracle chain, tick by tick."""
    o = bank_oracle(aof, orc, synth, case)
    p = tr.params_of(aof, case["cfg"])
    x0, y0 = cref.crop_origin(SENSOR[0], SENSOR[1], p.width, p.height)
    assert (y0 * SENSOR[0] + x0 + SKEW) % 2 == 1
    want, _ = run_camera_case(aof, orc, synth, gpu_device, case["cfg"], case["S"], case["T"], case["seed"], sensor=SENSOR,
                              rate=case["rate"], path=path, skew=SKEW, fx=case["fx"], fy=case["fy"],
                              source=tr.stream_source(case, p.width, p.height), patches=False)
    assert want.tobytes() == o["want"].tobytes(), "the run that was compared is the run of the census"


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("case", CAMERA_CASES, ids=ids)
def test_camera_burst(aof, orc, synth, gpu_device, case, path):
    o = bank_oracle(aof, orc, synth, case)
    c = burst_case(aof, orc, synth, case, o, path, camera=True)
    assert (c.derot != 0).any()
    run_bursts(c, orc, gpu_device)
