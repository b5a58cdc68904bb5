"""The one-launch tick with the lens inside it at every edge of its plan (csrc/k_bank_tick_warp.hip, csrc/aof_small_plan.hpp:
small_warp_plan_make): the cases of tests/warp_plan_ref.py (TICK_CASES: idle waves, a partly filled last trip, a second trip of
the node loop, a partial last cell row, two levels off a partly filled buffer, the exposure mask off the crop's corner, the
dynamic-LDS attribute set by the nodes alone, the last height that fits LDS and the first that does not), each on a bank of
mixed meshes under aof_set_bank_path(1).  The references are independent of the kernels: per tick and stream the stored frame
is the numpy model's warped crop (tests/bank_warp_ref.py) byte for byte, the record and the wire bytes are those of an oracle
chain of its own fed the model's crops, a due frame's histogram is the model's and its MSV bit-exact
(tests/bank_warp_tick_cases.py works all of it out on the host, and asserts that no case passes vacuously, before the device
runs).  A twin on path 2 must then hold the same bytes.  Where the model says the nodes do not fit, the push under path 1
reports the composed path and the references hold all the same."""
import numpy as np
import pytest

import bank_warp_tick_cases as tc
import crop_source_ref as csr
import warp_plan_ref as wplan
from bank_rig import time_limit   # (this module's fixture too: every test under a limit of its own)
from bank_sensor_rig import same_rigs, table_tensor
from bank_warp_rig import WarpRig

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
RUNS = tc.every_run()


def break_refused_stream(rig, dev, fmt):
    """The refused stream's record one byte beyond camera_bytes (inside the allocation's slack): AOF_TICK_BAD_SENSOR."""
    bad = rig.recs[tc.REFUSED].copy()
    bad["offset"] = rig.camera_bytes - csr.extent(bad, fmt) + 1
    assert not csr.valid(bad, fmt, 1, rig.shape.W, rig.shape.H, rig.camera_bytes) and rig.alloc.numel() - 1 - rig.camera_bytes >= 64
    rig.recs = rig.recs.copy()
    rig.recs[tc.REFUSED] = bad
    rig.table = table_tensor(dev, rig.recs)


def fill_staging(bank):
    bank.buffer[bank.staging:].fill_(SENTINEL)


def staging_untouched(bank):
    return bool((bank.buffer[bank.staging:] == SENTINEL).all().item())


def rig_of(aof, eng, q, dev, **kw):
    rig = WarpRig(aof, eng, q.run, q.bp, dev, q.cam, fmt=q.fmt, rows=q.rows, shape=q.shape, **kw)
    assert rig.layout_bytes == q.nbytes
    rig.give_meshes(q.meshes)
    break_refused_stream(rig, dev, q.fmt)
    rig.bind()
    return rig


def check_step(aof, q, i, got, what):
    """One tick or one round of the burst against the references of step i."""
    for s, (kind, rec, wire, crop, hist) in enumerate(q.want[i]):
        at = what + ("stream", s)
        if kind == tc.BAD:
            idle = np.zeros((), got.recs.dtype)
            idle["quality"] = aof.TICK_BAD_SENSOR
            assert got.recs[s].tobytes() == idle.tobytes() and got.wire[s] == b"", at
            assert not got.exposure[s].tobytes().strip(b"\0"), at
        elif kind == tc.IDLE:
            assert got.recs[s]["quality"] == aof.TICK_IDLE and got.wire[s] == b"", at
        else:
            assert got.recs[s].tobytes() == rec.tobytes(), at + (got.recs[s], rec)
            assert got.wire[s] == wire, at
            assert int(got.exposure[s]["due"]) == int(q.due[i, s]), at
            if q.due[i, s]:
                assert got.exposure[s]["hist"].tolist() == hist.tolist(), at
                assert got.exposure[s]["msv"].tobytes() == np.float32(aof.exposure_msv(hist)).tobytes(), at


def stored(rig):
    n, w, h = rig.shape.S, rig.shape.W, rig.shape.H
    return rig.bank.frames_bytes()[:n * w * h].reshape(n, h, w)


def unbound_tick_first(aof, q, dev):
    """One tick of an engine with nothing warped bound, on the same configuration: the unwarped one-launch tick, whose plan
    does not set the dynamic-LDS attribute, runs in this process before the warped one, whose nodes set it."""
    eng = aof.FlowEngine(q.params, 0)
    eng.set_bank_path(1)
    rig = WarpRig(aof, eng, q.run, q.bp, dev, q.cam, fmt=q.fmt, rows=q.rows, shape=q.shape)
    rig.bind()
    rig.push(0)
    assert eng.last_bank_path() == 1
    buf = rig.frames[:rig.layout_bytes].cpu().numpy()
    for s in range(q.shape.S):   # (not an identity mesh's: at a height off the cell its last node row lies below a plane's last row)
        assert np.array_equal(stored(rig)[s], csr.crop(buf, rig.recs[s], q.fmt, 1, q.shape.W, q.shape.H)), ("nothing bound: the plain crop", s)
    eng.close()


@pytest.mark.parametrize("case,sub,fmt,burst", RUNS, ids=[tc.run_id(*r) for r in RUNS])
def test_the_warped_tick_is_the_model_and_the_oracle_chain_at_the_edges_of_its_plan(aof, orc, synth, gpu_device, case, sub, fmt, burst):
    q = tc.prepare(aof, orc, synth, case, sub, fmt, burst)
    plan, reach = wplan.case_tick_plan(case), wplan.tick_reach(case)
    assert set(case["tags"]) <= reach, sorted(set(case["tags"]) - reach)
    assert aof.bank_warp_one_launch(q.params) == (q.path == 1, plan["lds"]), "the library's answer is the model's"
    assert (q.path == 2) == ("t_fallback_nodes_do_not_fit" in reach)
    if case["unbound_first"]:
        unbound_tick_first(aof, q, gpu_device)
    ea, eb = aof.FlowEngine(q.params, 0), aof.FlowEngine(q.params, 0)
    ea.set_bank_path(1), eb.set_bank_path(2)
    a, b = rig_of(aof, ea, q, gpu_device), rig_of(aof, eb, q, gpu_device)
    fill_staging(a.bank), fill_staging(b.bank)
    before_frames, before_state = stored(a)[tc.REFUSED].copy(), a.bank.state_bytes()[tc.REFUSED].copy()
    for k in range(q.shape.T):
        what = (case["id"], "tick", k)
        a.load(k), a.enqueue()
        b.load(k), b.enqueue()
        assert (ea.last_bank_path(), eb.last_bank_path()) == (q.path, 2), what
        check_step(aof, q, k, a.read(), what)
        frames = stored(a)
        for s, (kind, _, _, crop, _) in enumerate(q.want[k]):
            if kind == tc.FRAME:
                assert a.warped[0][s].tobytes() == crop.tobytes() and frames[s].tobytes() == crop.tobytes(), what + ("stored frame", s)
        same_rigs(a, b, what + ("the composed twin",))
    if burst:
        ka, kb = (rig_of(aof, e, q, gpu_device, K=tc.K, pad=37, bank=r.bank) for e, r in ((ea, a), (eb, b)))
        ka.load(q.burst_at, q.given), ka.enqueue()
        kb.load(q.burst_at, q.given), kb.enqueue()
        assert (ea.last_bank_path(), eb.last_bank_path()) == (q.path, 2), "burst"
        rounds = ka.read()
        last = {}
        for r in range(tc.K):
            check_step(aof, q, q.shape.T + r, rounds[r], (case["id"], "burst round", r))
            last.update({s: row[3] for s, row in enumerate(q.want[q.shape.T + r]) if row[0] == tc.FRAME})
        frames = stored(ka)
        assert len(last) >= 3 and all(frames[s].tobytes() == crop.tobytes() for s, crop in last.items()), "a stream's stored frame: its last round's crop"
        same_rigs(ka, kb, (case["id"], "burst", "the composed twin"))
    a.torch.cuda.synchronize()
    assert staging_untouched(a.bank) == (q.path == 1), "path 1 neither reads nor writes the staging region; the composed path stages its crops"
    assert not staging_untouched(b.bank)
    assert stored(a)[tc.REFUSED].tobytes() == before_frames.tobytes(), "the refused stream's stored frame"
    assert a.bank.state_bytes()[tc.REFUSED].tobytes() == before_state.tobytes(), "the refused stream's state"
    ea.close(), eb.close()
