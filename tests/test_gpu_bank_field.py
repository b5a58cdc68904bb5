"""The stream bank's motion field on the device (csrc/k_bank_field.hip behind aof_bank_field_device, include/aof.h "the stream
bank's motion field") against the numpy model (tests/bank_field_ref.py), byte for byte: designed block records and hand-made
tick records written straight into a bank at the public offsets for every geometry of field_ref.GEOMETRIES; real ticks of
the PX4 64 x 64 and the two-level 128 x 128 bank against the model fed the ORACLE's blocks; twin banks on the two bank paths;
behind the camera push, the warped one-launch tick and the IMU call; push + field in one captured graph; the refusals; and
OpticalFlowBank::enableField() through the rig's own handle on the facade library."""
import ctypes as C

import numpy as np
import pytest

import bank_field_ref as bf
import bank_field_rig as rig
import field_ref as fr
from bank_ref import FX, FY, make_run, oracle_chain
from bank_rig import time_limit   # noqa: F401  (this module's fixture too: every test under a limit of its own)

pytestmark = pytest.mark.gpu
SENTINEL, GUARD = 0xEE, 256


def up(dev, a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(dev)


def angle_of(aof):
    return lambda px, focal: np.float32(aof.lib.aof_flow_angle(px, focal))


class Outputs:
    """Tick records (input), state, output records and fields of S streams between guard zones of one allocation filled with
    a sentinel: after a launch nothing but the three outputs may have changed."""

    def __init__(self, torch, dev, S):
        sizes = dict(records=48 * S, state=64 * S, out=48 * S, fields=64 * S)
        self.at, off = {}, GUARD
        for k, v in sizes.items():
            self.at[k] = (off, off + v)
            off = (off + v + 255) // 256 * 256 + GUARD
        self.mem = torch.full((off,), SENTINEL, dtype=torch.uint8, device=dev)
        self.S = S

    def view(self, k):
        lo, hi = self.at[k]
        return self.mem[lo:hi].view(self.S, -1)

    def arm(self, records=None):
        """Sentinels into the two pure outputs, the tick records uploaded; remembers everything."""
        if records is not None:
            self.view("records").copy_(up(self.mem.device, np.frombuffer(records.tobytes(), np.uint8).reshape(self.S, 48)))
        self.view("out").fill_(SENTINEL)
        self.view("fields").fill_(SENTINEL)
        self.before = self.mem.cpu().numpy()

    def read(self, aof, fields=True):
        """(state, out, fields) as records; everything outside them must be as arm() left it."""
        after = self.mem.cpu().numpy()
        keep = np.ones(after.size, bool)
        for k in ("state", "out") + (("fields",) if fields else ()):
            keep[self.at[k][0]:self.at[k][1]] = False
        moved = np.flatnonzero((after != self.before) & keep)
        assert moved.size == 0, ("bytes outside the outputs written", moved[:8])
        cut = lambda k, dt: after[self.at[k][0]:self.at[k][1]].copy().view(dt)
        return cut("state", rig.STATE_DTYPE), cut("out", rig.RECORD_DTYPE), cut("fields", aof.FIELD_DTYPE)


def differing(got, want):
    return [(s, got[s], want[s]) for s in range(len(want)) if got[s].tobytes() != want[s].tobytes()][:2]


# ---- 1. synthetic arrays at every geometry -----------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", fr.GEOMETRIES, ids=[g[0] for g in fr.GEOMETRIES])
def test_designed_blocks_in_a_bank_equal_the_model(aof, gpu_device, geom):
    import torch
    p = fr.make_params(aof, geom)
    eng = aof.FlowEngine(p, 0)
    nb = eng.nblocks(0)
    assert nb == fr.NBLOCKS[geom[0]]
    S, T = (9 if nb <= 256 else 3), 4             # three workgroups of the wave form, the last holding one stream
    bound = nb % 2 == 1                           # per-stream focal lengths on the odd grids
    bp = aof.bank_params(S, focal_x=216.5, focal_y=180.25)
    L = aof.bank_layout(p, bp)
    at_b, at_s = rig.scratch_offsets(aof, p, L, S)
    assert at_b % 256 == 0 and (nb % 4 == 0 or (at_b + 4 * nb) % 16 != 0), "an odd grid misaligns stream 1's records"
    blocks, subdirs, records = bf.designed_run(p, S, T, seed=nb)
    focals = bf.focal_table(S, nb) if bound else np.tile(np.array([bp.focal_x, bp.focal_y], np.float32), (S, 1))
    if bound:
        streams = aof.bank_stream_from_params(bp, S)
        streams["focal_x"], streams["focal_y"] = focals[:, 0], focals[:, 1]
        eng.set_bank_streams(up(gpu_device, np.frombuffer(streams.tobytes(), np.uint8).copy()))
    bank = torch.full((L.total_bytes,), SENTINEL, dtype=torch.uint8, device=gpu_device)
    o = Outputs(torch, gpu_device, S)
    assert rig.reset(aof, eng, o.view("state")) == 0
    want_state = np.zeros(S, rig.STATE_DTYPE)
    angle = angle_of(aof)
    seen, pairs = set(), 0
    for t in range(T):
        bank[at_b:at_b + 4 * S * nb].copy_(up(gpu_device, np.frombuffer(blocks[t].tobytes(), np.uint8)))
        bank[at_s:at_s + S * nb].copy_(up(gpu_device, subdirs[t].reshape(-1)))
        before = bank.cpu().numpy()
        o.arm(records[t])
        state0 = o.view("state").clone()
        assert rig.device(aof, eng, bp, bank, o.view("records"), o.view("state"), o.view("out"), o.view("fields")) == 0, aof.lib.aof_last_error(eng._ctx)
        torch.cuda.synchronize()
        state, out, fields = o.read(aof)
        assert (bank.cpu().numpy() == before).all(), "the bank is only read"
        wf, wo = bf.step(p, focals, blocks[t], subdirs[t], records[t], want_state, angle)
        assert fields.tobytes() == wf.tobytes(), (t, differing(fields, wf))
        assert out.tobytes() == wo.tobytes(), (t, differing(out, wo))
        assert state.tobytes() == want_state.tobytes(), (t, differing(state, want_state))
        # the pair streams' fits are aof_field_batch_device's on the same records
        tb = bank[at_b:at_b + 4 * S * nb].view(torch.int32).view(S, nb)
        ts = bank[at_s:at_s + S * nb].view(S, nb) if p.subpixel else None
        flows = o.view("records")[:, 32:48].contiguous()
        batch = aof.fields_view(eng.field_batch(tb, flows, subdirs=ts))
        torch.cuda.synchronize()
        for s in range(S):
            if bf.ran_pair(records[t, s]):
                assert batch[s].tobytes() == fields[s].tobytes(), (t, s)
                pairs += 1
                seen.add(int(fields[s]["flags"]) & fr.VALID)
        # d_fields = NULL: the same records and state
        o.view("state").copy_(state0)
        o.arm()
        assert rig.device(aof, eng, bp, bank, o.view("records"), o.view("state"), o.view("out"), None) == 0
        torch.cuda.synchronize()
        state2, out2, untouched = o.read(aof, fields=False)
        assert state2.tobytes() == state.tobytes() and out2.tobytes() == out.tobytes()
        assert (untouched.view(np.uint8) == SENTINEL).all()
    assert seen == {0, fr.VALID} and pairs >= S, (seen, pairs)
    assert (want_state["published"] > 0).all()
    eng.close()


# ---- real ticks ----------------------------------------------------------------------------------------------------------------
class Device:
    """A bank, its field state and outputs on the device; tick(): push + field call, returns host copies."""

    def __init__(self, aof, eng, bp, dev, camera=None):
        import torch
        self.aof, self.eng, self.torch, self.dev = aof, eng, torch, dev
        self.bank = eng.bank_create(bp, dev, camera=camera)
        S = bp.n_streams
        self.state = torch.full((S, 64), SENTINEL, dtype=torch.uint8, device=dev)
        self.out = torch.zeros((S, 48), dtype=torch.uint8, device=dev)
        self.fields = torch.zeros((S, 64), dtype=torch.uint8, device=dev)
        assert rig.reset(aof, eng, self.state) == 0

    def field(self, records):
        rc = rig.device(self.aof, self.eng, self.bank.bp, self.bank.buffer, records, self.state, self.out, self.fields)
        assert rc == 0, self.aof.lib.aof_last_error(self.eng._ctx)

    def read(self):
        self.torch.cuda.synchronize()
        cut = lambda t, dt: t.cpu().numpy().reshape(-1).view(dt).copy()
        return cut(self.state, rig.STATE_DTYPE), cut(self.out, rig.RECORD_DTYPE), cut(self.fields, self.aof.FIELD_DTYPE)

    def tick(self, frames, times, active=None):
        d = self.dev
        self.records = self.eng.bank_push(self.bank, up(d, frames), up(d, times), None if active is None else up(d, active))
        self.field(self.records)
        return self.read()

    def scratch(self, p):
        """Host copies of the tick's block records [S, nb] and sub-directions [S, nb] as the bank holds them."""
        S = self.bank.n_streams
        nb = self.eng.nblocks(0)
        at_b, at_s = rig.scratch_offsets(self.aof, p, self.bank.layout, S)
        buf = self.bank.buffer
        return (buf[at_b:at_b + 4 * S * nb].cpu().numpy().view(fr.BLOCK_DTYPE).reshape(S, nb),
                buf[at_s:at_s + S * nb].cpu().numpy().reshape(S, nb))


class OracleModel:
    """The model fed one ORACLE chain per stream: pyoracle's calcFlow chain for the tick records, pyoracle's blocks for the fit."""

    def __init__(self, aof, orc, p, rates, focals):
        self.aof, self.orc, self.p, self.po = aof, orc, p, orc.params_from(p)
        self.rates, self.focals = rates, np.asarray(focals, np.float32)
        self.S = len(rates)
        self.nb = fr.coordinates(p)[0].size
        self.chains = [self.new_chain(s) for s in range(self.S)]
        self.state = np.zeros(self.S, rig.STATE_DTYPE)
        self.angle = angle_of(aof)

    def new_chain(self, s):
        return oracle_chain(self.aof, self.orc, self.p, self.rates[s], 0, 0, use_gyro=False, fx=float(self.focals[s, 0]), fy=float(self.focals[s, 1]))

    def reset(self, mask):
        for s in np.flatnonzero(mask):
            self.chains[s] = self.new_chain(int(s))
            self.state[s] = np.zeros((), rig.STATE_DTYPE)

    def tick(self, frames, times, active):
        S = self.S
        records = np.zeros(S, self.aof.TICK_DTYPE)
        blocks, subdirs = np.zeros((S, self.nb), fr.BLOCK_DTYPE), np.zeros((S, self.nb), np.uint8)
        for s in range(S):
            if active is not None and not active[s]:
                records[s]["quality"] = bf.IDLE
                continue
            prev = self.chains[s].prev
            if prev is not None:
                r = self.orc.flow_pair(self.po, prev, frames[s])
                blocks[s], subdirs[s] = r["blocks"], r["subdirs"]
            records[s], _ = self.chains[s].push(frames[s], times[s], np.zeros(4, np.float32))
        fields, out = bf.step(self.p, self.focals, blocks, subdirs, records, self.state, self.angle)
        return records, fields, out


def climbing(synth, w, h, T, s):
    """T frames of stream s: even streams climb (a steady zoom with a small pan), odd streams are chains of zooming and
    rotating pairs (prev, cur of make_warp_pair after one another)."""
    if s % 2 == 0:
        return synth.make_camera_sequence(w, h, T, seed=50 + s, max_step=1, zoom_q16=260 + 40 * s)[0]
    pairs = [synth.make_warp_pair(w, h, reach=2, pair_index=10 * s + k, noise=2) for k in range((T + 1) // 2)]
    return np.stack([f for q in pairs for f in (q[0], q[1])])[:T]


S2, T2 = 9, 12
FREE, FLAT, RESET, IDLER = 4, 5, 6, 1    # the stream without a limiter (own focal lengths), the featureless one, the one reset mid-run, the idle one


def px4_case(synth):
    rng = np.random.default_rng(77)
    frames = np.stack([climbing(synth, 64, 64, T2, s) for s in range(S2)], axis=1)          # [T, S, 64, 64]
    frames[:, FLAT] = 128
    times = np.cumsum(rng.integers(19000, 24000, (T2, S2)), axis=0).astype(np.int64)         # windows of three to four frames at 15 Hz
    active = np.ones((T2, S2), np.uint8)
    active[[2, 3, 7], IDLER] = 0
    rates = [15] * S2
    rates[FREE] = 0
    focals = np.tile(np.array([FX, FY], np.float32), (S2, 1))
    focals[FREE] = (310.5, 295.25)
    return frames, times, active, rates, focals


def run_px4_model(aof, orc, synth):
    frames, times, active, rates, focals = px4_case(synth)
    p = aof.px4flow_params(64, 64)
    m = OracleModel(aof, orc, p, rates, focals)
    ticks = []
    for t in range(T2):
        if t == 6:
            mask = np.zeros(S2, np.uint8)
            mask[RESET] = 1
            m.reset(mask)
        ticks.append(m.tick(frames[t], times[t], active[t]) + (m.state.copy(),))
    return p, ticks


def check_caps(ticks):
    """At most one stream without a valid fit -- the featureless one --; every other stream shows fits >= 1 in every
    published window that saw a pair."""
    fits = np.zeros(S2, np.int64)
    for _, fields, out, _ in ticks:
        fits += (fields["flags"] & fr.VALID) != 0
        for s in range(S2):
            if s != FLAT and int(out[s]["status"]) >= 0 and int(out[s]["pairs"]) > 0:
                assert int(out[s]["fits"]) >= 1, (s, out[s])
    assert fits[FLAT] == 0 and (np.delete(fits, FLAT) > 0).all(), fits
    assert sum(int((o["status"] >= 0).sum()) for _, _, o, _ in ticks) >= 3 * S2


def test_real_ticks_of_the_px4_bank_equal_the_model_on_the_oracles_blocks(aof, orc, synth, gpu_device):
    frames, times, active, rates, focals = px4_case(synth)
    p, ticks = run_px4_model(aof, orc, synth)
    check_caps(ticks)
    eng = aof.FlowEngine(p, 0)
    bp = aof.bank_params(S2, FX, FY, 15, 0, 1, 100, 0)
    streams = aof.bank_stream_from_params(bp, S2)
    streams["output_rate"][FREE] = 0
    streams["focal_x"], streams["focal_y"] = focals[:, 0], focals[:, 1]
    eng.set_bank_streams(up(gpu_device, np.frombuffer(streams.tobytes(), np.uint8).copy()))
    d = Device(aof, eng, bp, gpu_device)
    windows = set()
    for t in range(T2):
        if t == 6:
            mask = np.zeros(S2, np.uint8)
            mask[RESET] = 1
            eng.bank_reset(d.bank, up(gpu_device, mask))
            assert rig.reset(aof, eng, d.state, up(gpu_device, mask)) == 0
        state, out, fields = d.tick(frames[t], times[t], active[t])
        records, wf, wo, ws = ticks[t]
        assert aof.ticks_view(d.records).tobytes() == records.tobytes(), (t, "tick records")
        assert fields.tobytes() == wf.tobytes(), (t, differing(fields, wf))
        assert out.tobytes() == wo.tobytes(), (t, differing(out, wo))
        assert state.tobytes() == ws.tobytes(), (t, differing(state, ws))
        windows |= {int(o["pairs"]) for s, o in enumerate(out) if int(o["status"]) >= 0 and s != FREE}
    assert {3, 4} & windows and max(windows) <= 4, windows
    assert (out["status"][IDLER] != bf.IDLE) and int(state["published"][FREE]) == T2
    eng.close()


# ---- 3. twin banks on the two paths --------------------------------------------------------------------------------------------
def test_twin_banks_on_the_two_paths_publish_the_same_fields(aof, synth, gpu_device):
    frames, times, active, _, _ = px4_case(synth)
    rng = np.random.default_rng(3)
    frames = frames.copy()
    p = aof.px4flow_params(64, 64)
    eng = aof.FlowEngine(p, 0)
    bp = aof.bank_params(S2, FX, FY, 15, 0, 1, 100, 0)
    a, b = Device(aof, eng, bp, gpu_device), Device(aof, eng, bp, gpu_device)
    idle_blocks_differ = False
    for t in range(8):
        idle = np.flatnonzero(active[t] == 0)
        frames[t, idle] = rng.integers(0, 256, (len(idle), 64, 64), dtype=np.uint8)     # nobody's frames: noise
        got = []
        for dev, path in ((a, 1), (b, 2)):
            eng.set_bank_path(path)
            got.append(dev.tick(frames[t], times[t], active[t]))
            assert eng.last_bank_path() == path
        for x, y, what in zip(got[0], got[1], ("state", "records", "fields")):
            assert x.tobytes() == y.tobytes(), (t, what)
        for s in idle:
            assert int(got[0][1][s]["status"]) == bf.IDLE and not np.frombuffer(got[0][2][s].tobytes(), np.uint8).any()
            idle_blocks_differ |= a.scratch(p)[0][s].tobytes() != b.scratch(p)[0][s].tobytes()
    assert idle_blocks_differ, "the one-launch tick leaves an idle stream's blocks stale, the composed path computes them for nobody"
    assert int(got[0][0]["published"].sum()) > S2
    eng.close()


# ---- 4. two levels, sub-pixel refinement ------------------------------------------------------------------------------------------
def test_the_two_level_bank_brings_subdirections_and_predictors_to_the_fit(aof, orc, synth, gpu_device):
    S, T = 5, 6
    p = aof.px4flow_params(128, 128, pyramid_levels=2, mean_subtract=1)
    assert p.subpixel
    # a camera that pans up to six pixels a frame while it climbs: predictors from level 1, half-pixel matches at level 0
    frames = np.stack([synth.make_camera_sequence(128, 128, T, seed=300 + s, max_step=6, zoom_q16=300)[0] for s in range(S)], axis=1)
    times = np.cumsum(np.full((T, S), 30000), axis=0).astype(np.int64)
    eng = aof.FlowEngine(p, 0)
    d = Device(aof, eng, aof.bank_params(S, FX, FY, 15, 0, 1, 100, 0), gpu_device)
    m = OracleModel(aof, orc, p, [15] * S, np.tile(np.array([FX, FY], np.float32), (S, 1)))
    predicted = refined = valid = 0
    for t in range(T):
        state, out, fields = d.tick(frames[t], times[t])
        records, wf, wo = m.tick(frames[t], times[t], None)
        assert aof.ticks_view(d.records).tobytes() == records.tobytes(), t
        assert fields.tobytes() == wf.tobytes(), (t, differing(fields, wf))
        assert out.tobytes() == wo.tobytes() and state.tobytes() == m.state.tobytes(), (t, differing(out, wo))
        predicted += int(((records["pixel"]["pred_x"] != 0) | (records["pixel"]["pred_y"] != 0)).sum())
        refined += int((d.scratch(p)[1] < 8).sum()) if t else 0
        valid += int(((fields["flags"] & fr.VALID) != 0).sum())
    assert predicted > 0 and refined > 0 and valid >= S, (predicted, refined, valid)
    eng.close()


# ---- 5. behind the camera push and the warped one-launch tick; 6. behind the IMU call: the host twin on the device's blocks ----
def host_on_device_blocks(aof, p, d, records, state):
    """aof_bank_field_host on what the bank holds; `state` is stepped in place."""
    blocks, subdirs = d.scratch(p)
    rc, fields, out = rig.host(aof, p, d.bank.bp, blocks, subdirs, records, state)
    assert rc == 0
    return fields, out


@pytest.mark.parametrize("warped", [False, True], ids=["camera", "warped-one-launch"])
def test_behind_a_camera_push(aof, synth, gpu_device, warped):
    S, T, cw, ch = 4, 6, 96, 80
    p = aof.px4flow_params(64, 64)
    eng = aof.FlowEngine(p, 0)
    cam = aof.bank_camera_params(cw, ch, 64, 64, 0, 200000)
    d = Device(aof, eng, aof.bank_params(S, FX, FY, 15, 0, 1, 100, 0), gpu_device, camera=cam)
    if warped:
        meshes = np.stack([aof.warp_mesh_from_lens(p, 120.0 + 5 * s, 120.0, cw / 2, ch / 2, k1=-0.05 * s) for s in range(S)])
        eng.set_bank_warps(up(gpu_device, np.frombuffer(meshes.tobytes(), np.uint8).reshape(S, -1)), S)
        eng.set_bank_path(1)
    rng = np.random.default_rng(8)
    crops = np.stack([climbing(synth, 64, 64, T, s) for s in range(S)], axis=1)
    times = np.cumsum(rng.integers(19000, 24000, (T, S)), axis=0).astype(np.int64)
    state = np.zeros(S, rig.STATE_DTYPE)
    x0, y0 = cw // 2 - 32, ch // 2 - 32
    published = valid = 0
    for t in range(T):
        sensor = rng.integers(0, 256, (S, ch, cw), dtype=np.uint8)
        sensor[:, y0:y0 + 64, x0:x0 + 64] = crops[t]
        active = np.ones(S, np.uint8)
        active[2] = t != 3
        out = eng.bank_push_camera(d.bank, up(gpu_device, sensor), up(gpu_device, times[t]), up(gpu_device, active), None)
        if warped:
            assert eng.last_bank_path() == 1
        d.field(out["records"])
        got_state, got_out, got_fields = d.read()
        wf, wo = host_on_device_blocks(aof, p, d, aof.ticks_view(out["records"]), state)
        assert got_fields.tobytes() == wf.tobytes() and got_out.tobytes() == wo.tobytes() and got_state.tobytes() == state.tobytes(), t
        published += int((got_out["status"] >= 0).sum())
        valid += int(((got_fields["flags"] & fr.VALID) != 0).sum())
    assert published >= 2 * S and valid >= S, (published, valid)
    eng.close()


def test_behind_the_imu_call_dropped_records_close_the_window(aof, synth, gpu_device):
    import torch
    S, T, M = 5, 12, 2
    p = aof.px4flow_params(64, 64)
    eng = aof.FlowEngine(p, 0)
    bp = aof.bank_params(S, FX, FY, 15, 0, 1, 100, 0)
    behind, front = Device(aof, eng, bp, gpu_device), Device(aof, eng, bp, gpu_device)
    run = make_run(synth, 64, 64, S, T, 23, density=0.9, black=False)
    imu_state = torch.zeros((S, 64), dtype=torch.uint8, device=gpu_device)
    eng.bank_imu_reset(imu_state, offset0=0)
    rng = np.random.default_rng(4)
    clock = np.full(S, 10 ** 9, np.int64)
    state = np.zeros(S, rig.STATE_DTYPE)
    dropped = closed = 0
    for t in range(T):
        samples = np.zeros((M, S), aof.IMU_SAMPLE_DTYPE)
        counts = np.zeros(S, np.uint8)
        for s in range(1, S):                       # stream 0 never hears its IMU: what it publishes is dropped as stale
            counts[s] = 0 if (t + s) % 3 == 0 else M
            for j in range(counts[s]):
                clock[s] += int(rng.integers(2000, 3000))
                samples[j, s] = (clock[s], *rng.normal(0, 0.5, 3).astype(np.float32), 0)
        # the field call in front of the IMU call, on the limiter's own verdicts ...
        front.tick(run.frames[t], run.times[t], run.active[t])
        f_state, f_out, f_fields = front.read()
        # ... and behind it, on records the IMU call has rewritten
        records = eng.bank_push(behind.bank, up(gpu_device, run.frames[t]), up(gpu_device, run.times[t]), up(gpu_device, run.active[t]))
        eng.bank_imu(up(gpu_device, samples.view(np.uint8).reshape(M, S, 24)), up(gpu_device, run.times[t]), records, imu_state,
                     up(gpu_device, counts), records_out=records, mavlink=False)
        behind.field(records)
        b_state, b_out, b_fields = behind.read()
        recs = aof.ticks_view(records)
        wf, wo = host_on_device_blocks(aof, p, behind, recs, state)
        assert b_fields.tobytes() == wf.tobytes() and b_out.tobytes() == wo.tobytes() and b_state.tobytes() == state.tobytes(), t
        assert b_out.tobytes() == f_out.tobytes() and b_state.tobytes() == f_state.tobytes() and b_fields.tobytes() == f_fields.tobytes(), t
        drop = (recs["quality"] == bf.STALE_GYRO) | (recs["quality"] == bf.NO_OFFSET)
        dropped += int(drop.sum())
        closed += int((b_out["status"][drop] >= 0).sum())
        assert (b_out["dt_us"][drop] == recs["dt_us"][drop]).all()
    assert dropped >= 2 and closed == dropped, (dropped, closed)
    eng.close()


# ---- 7. push + field in one captured graph ------------------------------------------------------------------------------------------
def test_push_and_field_in_one_graph_replayed_six_times_equal_an_eager_twin(aof, synth, gpu_device):
    import torch
    frames, times, active, _, _ = px4_case(synth)
    S = S2
    p = aof.px4flow_params(64, 64)
    eng = aof.FlowEngine(p, 0)
    bp = aof.bank_params(S, FX, FY, 15, 0, 1, 100, 0)
    eager = Device(aof, eng, bp, gpu_device)
    want = [eager.tick(frames[t], times[t], active[t]) for t in range(7)]
    assert sum(int((w[1]["status"] >= 0).sum()) for w in want[1:]) >= S and sum(int(w[1]["fits"].sum()) for w in want) > S
    g = Device(aof, eng, bp, gpu_device)
    t_frames, t_times, t_active = up(gpu_device, frames[0]), up(gpu_device, times[0]), up(gpu_device, active[0])
    records = torch.zeros((S, 48), dtype=torch.uint8, device=gpu_device)

    def enqueue():
        eng.bank_push(g.bank, t_frames, t_times, t_active, records=records)
        g.field(records)

    enqueue()                                   # tick 0 eagerly: every kernel has run once before the capture
    torch.cuda.synchronize()
    first = g.read()
    for x, y in zip(first, want[0]):
        assert x.tobytes() == y.tobytes()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=gpu_device)
    bank0, state0 = g.bank.buffer.clone(), g.state.clone()
    with torch.cuda.graph(graph, stream=side):
        enqueue()
    g.bank.buffer.copy_(bank0)                  # (a capture enqueues nothing; the copies keep that visible)
    g.state.copy_(state0)
    for t in range(1, 7):
        t_frames.copy_(up(gpu_device, frames[t])), t_times.copy_(up(gpu_device, times[t])), t_active.copy_(up(gpu_device, active[t]))
        g.out.fill_(SENTINEL), g.fields.fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        got = g.read()
        for x, y, what in zip(got, want[t], ("state", "records", "fields")):
            assert x.tobytes() == y.tobytes(), (t, what)
    eng.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(aof, gpu_device):
    import torch
    S = 4
    p = aof.default_params(64, 64)
    eng = aof.FlowEngine(p, 0)
    bp, fp = aof.bank_params(S), aof.field_params()
    L = aof.bank_layout(p, bp)
    bank = torch.full((L.total_bytes + 256,), SENTINEL, dtype=torch.uint8, device=gpu_device)
    o = Outputs(torch, gpu_device, S)
    _, _, records = bf.designed_run(p, S, 1)
    o.view("state").fill_(0)
    o.arm(records[0])
    stream = torch.cuda.current_stream(gpu_device).cuda_stream
    lib = rig.bind(aof)
    ptr = lambda k: o.view(k).data_ptr()
    good = [eng._ctx, C.byref(bp), C.byref(fp), bank.data_ptr(), L.total_bytes, ptr("records"), ptr("state"), ptr("fields"), ptr("out"), stream]
    bad = []
    for i in (0, 1, 2, 3, 5, 6, 8):                                            # NULL ctx, bp, fp, bank, records, state, out
        a = list(good)
        a[i] = None
        bad.append((a, rig.EINVAL))
    bad.append((good[:1] + [C.byref(aof.bank_params(0))] + good[2:], rig.EINVAL))
    for kw in (dict(min_blocks=2), dict(passes=3), dict(exclude_reach=2), dict(gate_px=0.0), dict(gate_px=float("nan"))):
        bad.append((good[:2] + [C.byref(aof.field_params(**kw))] + good[3:], rig.EINVAL))
    bad.append((good[:3] + [bank.data_ptr() + 128] + good[4:], rig.EINVAL))                    # a bank that is not 256-byte aligned
    bad.append((good[:6] + [ptr("state") + 4] + good[7:], rig.EINVAL))                         # state not 8-byte aligned
    bad.append((good[:7] + [ptr("fields") + 4] + good[8:], rig.EINVAL))                        # fields not 8-byte aligned
    bad.append((good[:4] + [L.total_bytes - 1] + good[5:], rig.ENOSPC))                        # a bank smaller than its layout
    for a, code in bad:
        assert lib.aof_bank_field_device(*a) == code, (a, code)
    # a stream table bound for another n_streams
    table = up(gpu_device, np.frombuffer(aof.bank_stream_from_params(bp, S + 1).tobytes(), np.uint8).copy())
    eng.set_bank_streams(table, S + 1)
    assert lib.aof_bank_field_device(*good) == rig.EINVAL and b"aof_set_bank_streams" in aof.lib.aof_last_error(eng._ctx)
    eng.set_bank_streams(None)
    # a geometry the fit does not serve
    wide = aof.FlowEngine(aof.default_params(8192, 2048), 0)
    assert lib.aof_bank_field_device(*([wide._ctx] + good[1:])) == rig.EINVAL
    wide.close()
    # the reset's own
    assert lib.aof_bank_field_reset_device(None, S, None, ptr("state"), stream) == rig.EINVAL
    assert lib.aof_bank_field_reset_device(eng._ctx, S, None, None, stream) == rig.EINVAL
    assert lib.aof_bank_field_reset_device(eng._ctx, 0, None, ptr("state"), stream) == rig.EINVAL
    assert lib.aof_bank_field_reset_device(eng._ctx, S, None, ptr("state") + 4, stream) == rig.EINVAL
    torch.cuda.synchronize()
    state, out, fields = o.read(aof)
    assert not state.view(np.uint8).any() and (out.view(np.uint8) == SENTINEL).all() and (fields.view(np.uint8) == SENTINEL).all()
    assert (bank.cpu().numpy() == SENTINEL).all()
    # and the call they all refused runs; a masked reset zeroes the masked streams alone
    assert lib.aof_bank_field_device(*good) == 0
    mask = up(gpu_device, np.array([0, 1, 0, 1], np.uint8))
    o.view("state").fill_(0x11)
    assert lib.aof_bank_field_reset_device(eng._ctx, S, mask.data_ptr(), ptr("state"), stream) == 0
    torch.cuda.synchronize()
    st = o.view("state").cpu().numpy()
    assert not st[[1, 3]].any() and (st[[0, 2]] == 0x11).all()
    eng.close()


# ---- 9. the facade ----------------------------------------------------------------------------------------------------------------------
def entries_of(entries):
    return [(int(e["stream"]), int(e["mavlink_len"]), e["mavlink"][:int(e["mavlink_len"])].tobytes(), e["record"].tobytes()) for e in entries]


@pytest.mark.parametrize("form", ["plain", "camera", "imu"])
def test_the_facade_with_enable_field_equals_the_c_abi_chain(aof, synth, gpu_device, form):
    """A: an OpticalFlowBank with enableField(); B: one without, fed the same; C: the C ABI, push + field call on the crops.
    A's field records and fits are C's entry by entry on raw bytes -- the field call runs in front of the IMU call and reads
    no gyro, so one chain serves the three forms --, a masked reset() restarts the masked streams' windows, and A publishes
    byte for byte what B publishes."""
    S, T, W, cw, ch = 4, 10, 128, 160, 144
    run = make_run(synth, W, W, S, T, 41, density=0.9, black=False)
    x0, y0 = cw // 2 - W // 2, ch // 2 - W // 2
    rng = np.random.default_rng(12)
    a, b = aof.OpticalFlowBank(FX, FY, 15, W, W, S), aof.OpticalFlowBank(FX, FY, 15, W, W, S)
    assert a.engineOk() and b.engineOk(), a.lastError()
    assert rig.field_records(aof, a) is None and rig.fields(aof, a) is None, "no enableField() yet"
    bad = aof.field_params(min_blocks=2)
    assert rig.enable_field(aof, a, bad) == rig.EINVAL and a.engineOk() and rig.field_records(aof, a) is None
    for bank in (a, b):
        if form == "camera":
            assert bank.enableCamera(cw, ch, 1700, 1, 30000) == 0, bank.lastError()
        if form == "imu":
            assert bank.enableImu(2, 1_650_000_000_000_000) == 0, bank.lastError()
        bank.setStreamFocalLength(1, 300.0, 280.0)
    assert rig.enable_field(aof, a) == 0, a.lastError()
    assert rig.enable_field(aof, a) == rig.EINVAL and "already" in a.lastError() and a.engineOk()
    p = aof.px4flow_params(W, W, pyramid_levels=2, mean_subtract=1)
    assert a.getPyramidLevels() == 2
    eng = aof.FlowEngine(p, 0)
    bp = aof.bank_params(S, FX, FY, 15, 0, 1, 100, 0)
    streams = aof.bank_stream_from_params(bp, S)
    streams["focal_x"][1], streams["focal_y"][1] = 300.0, 280.0
    eng.set_bank_streams(up(gpu_device, np.frombuffer(streams.tobytes(), np.uint8).copy()))
    c = Device(aof, eng, bp, gpu_device)
    clock = np.full(S, 5 * 10 ** 8, np.int64)
    published = 0
    for t in range(T):
        if t == 5:
            mask = np.array([0, 1, 1, 0], np.uint8)
            assert a.reset(mask) == 0 and b.reset(mask) == 0
            eng.bank_reset(c.bank, up(gpu_device, mask))
            assert rig.reset(aof, eng, c.state, up(gpu_device, mask)) == 0
        if form == "imu":
            for s in range(S):
                clock[s] += 2500
                for bank in (a, b):
                    assert bank.pushImu(s, int(clock[s]), 0.01 * s, -0.02, 0.005 * t) == 0
        if form == "camera":
            sensor = rng.integers(0, 256, (S, ch, cw), dtype=np.uint8)
            sensor[:, y0:y0 + W, x0:x0 + W] = run.frames[t]
            (na, ea), (nb, eb) = (bank.pushCamera(sensor, run.times[t], run.active[t], run.gyro[t]) for bank in (a, b))
        else:
            (na, ea), (nb, eb) = (bank.push(run.frames[t], run.times[t], run.active[t], run.gyro[t]) for bank in (a, b))
        assert na == nb >= 0 and entries_of(ea) == entries_of(eb), (t, a.lastError())
        state, out, fields = c.tick(run.frames[t], run.times[t], run.active[t])
        got_out, got_fields = rig.field_records(aof, a), rig.fields(aof, a)
        assert got_out.tobytes() == out.tobytes(), (t, differing(got_out, out))
        assert got_fields.tobytes() == fields.tobytes(), (t, differing(got_fields, fields))
        assert rig.field_records(aof, b) is None
        published += int((out["status"] >= 0).sum())
        if form != "imu":            # (with the IMU form a published record may be dropped behind the field call)
            assert sorted(int(e["stream"]) for e in ea) == [s for s in range(S) if int(out[s]["status"]) >= 0]
    assert published >= 2 * S and int(state["published"].min()) >= 1
    a.close(), b.close(), eng.close()
