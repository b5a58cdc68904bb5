"""The stream bank's outbox (aof_bank_collect_device, include/aof.h) and the facade's OpticalFlowBank: the dense, ordered,
host-pollable list of what a push published must equal, byte for byte, the host-side compaction of tests/outbox_ref.py
-- of the device's own outputs, of the oracle chain's records and wire frames, of K single ticks on a twin bank.
Every outbox is pre-filled with 0xEE, and every byte behind the stored entries (guard bytes behind the outbox included)
must still be 0xEE."""
import numpy as np
import pytest

import bank_ref as ref
import outbox_ref as ob
from bank_cases import Case
from bank_ref import FX, FY
from bank_rig import EINVAL, EIO, ENOSPC, OFFSET, BankRig, Guarded, params_of, same
from bank_rig import time_limit   # (this module's fixture too: every test under a limit of its own)

pytestmark = pytest.mark.gpu



class Box(Guarded):
    """A device outbox of the given capacities, 0xEE-filled, with guard bytes behind it."""

    def __init__(self, aof, gpu_device, cap_m, cap_e=0):
        self.total = aof.outbox_layout(cap_m, cap_e).total_bytes
        super().__init__(gpu_device, (self.total,), fill=ob.FILL)

    bytes = Guarded.read      # host copy of the outbox (synchronises); the guard must be untouched


def collect(aof, eng, gpu_device, records, wire, lens, exposure, derotated, cap_m, cap_e=0, tag=1):
    box = Box(aof, gpu_device, cap_m, cap_e)
    eng.bank_collect(records, wire, lens, exposure, derotated, cap_m, cap_e, outbox=box.tensor, tag=tag)
    return box.bytes()


@pytest.fixture(scope="module")
def recipe(aof, orc, synth):
    return ob.recipe_run(aof, orc, synth)


@pytest.mark.parametrize("path", [1, 2])
def test_every_tick_of_the_recipe_equals_the_compaction_of_the_oracle_chain(aof, recipe, gpu_device, path):
    run, recs, wire, lens, frames = recipe
    S = run.S
    eng = aof.FlowEngine(aof.px4flow_params(64, 64), 0)
    eng.set_bank_path(path)
    dev = BankRig(aof, eng, run, aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0), gpu_device)
    census = []
    for k in range(run.T):
        dev.load(k)
        dev.enqueue()
        got = collect(aof, eng, gpu_device, dev.records, dev.wire, dev.lens, None, None, S, tag=k + 1)
        same(got, ob.compact(dev.records, dev.wire, dev.lens, None, None, S, 0, tag=k + 1), ("device outputs", k))
        same(got, ob.compact(recs[k], frames[k], lens[k], None, None, S, 0, tag=k + 1), ("oracle chain", k))
        header, messages, _ = aof.outbox_view(got)
        census.append(int(header["n_messages"]))
        assert int(header["tag"]) == k + 1
        assert [bytes(m["mavlink"][:m["mavlink_len"]]) for m in messages] == [w for w in wire[k] if w]
    assert census == ob.CENSUS_15HZ and census[10] == 0, "tick 10 publishes nothing, its tag is written all the same"
    eng.close()


def test_overflow_stores_the_first_entries_and_counts_all(aof, recipe, gpu_device):
    run, recs, wire, lens, frames = recipe
    S, cap = run.S, 8
    eng = aof.FlowEngine(aof.px4flow_params(64, 64), 0)
    dev = BankRig(aof, eng, run, aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0), gpu_device)
    over = 0
    for k in range(run.T):
        dev.load(k)
        dev.enqueue()
        got = collect(aof, eng, gpu_device, dev.records, dev.wire, dev.lens, None, None, cap)
        header, messages, _ = aof.outbox_view(got, cap)
        assert int(header["messages_found"]) == ob.CENSUS_15HZ[k] and int(header["n_messages"]) == min(ob.CENSUS_15HZ[k], cap)
        same(got, ob.compact(recs[k], frames[k], lens[k], None, None, cap, 0), ("oracle chain", k))
        assert list(messages["stream"]) == list(np.flatnonzero(recs[k]["quality"] >= 0)[:cap])
        assert (got[64 + 128 * len(messages):] == ob.FILL).all()
        over += ob.CENSUS_15HZ[k] > cap
    assert over == 8
    eng.close()


@pytest.mark.parametrize("camera", [False, True], ids=["plain", "camera"])
def test_a_burst_collects_what_k_single_ticks_on_a_twin_bank_leave(aof, orc, synth, gpu_device, camera):
    """K = 5: both lists against compact() of K single ticks' outputs on a twin bank; `round` is filled; NULL d_mavlink,
    NULL d_exposure and NULL d_derotated each once."""
    c = Case(aof, orc, synth, cfg="px4-64", K=5, seed=21 if camera else 1, camera=camera)
    K, S, n = c.K, c.S, c.K * c.S
    eng, eng_t = c.engine(), c.engine()
    dev, twin = c.burst_device(eng, gpu_device), c.tick_device(eng_t, gpu_device)
    rounds, exposures = set(), 0
    for j in range(c.B):
        sensors = c.sensors(j)
        dev.load(j, c.given, sensors)
        dev.enqueue()
        expo, derot = (dev.exposure, dev.derotated) if camera else (None, None)
        got = collect(aof, eng, gpu_device, dev.records, dev.wire, dev.lens, expo, derot, n, n, tag=j + 7)
        tick = dict(records=[], wire=[], lens=[], exposure=[], derotated=[])
        for k in range(K):
            twin.push(j * K + k, sensors=sensors[k] if camera else None)
            for name in tick:
                tick[name].append(getattr(twin, name).cpu().numpy())
        t = {name: np.stack(v) for name, v in tick.items()}
        want = ob.compact(t["records"], t["wire"], t["lens"], t.get("exposure") if camera else None,
                          t.get("derotated") if camera else None, n, n, tag=j + 7)
        same(got, want, ("K single ticks", j))
        header, messages, exps = aof.outbox_view(got, n, n)
        assert int(header["n_messages"]) == int((c.want[j * K:(j + 1) * K]["quality"] >= 0).sum())
        rounds |= set(messages["round"].tolist())
        exposures += len(exps)
        if camera:
            assert int(header["n_exposures"]) == int(c.due[j * K:(j + 1) * K].sum()) and (exps["exposure"]["due"] == 1).all()
        if j == 1:      # each optional input left out once
            for drop in ("wire", "exposure", "derotated") if camera else ("wire",):
                a = dict(wire=dev.wire, lens=dev.lens, exposure=expo, derotated=derot)
                a[drop] = None
                if drop == "wire":
                    a["lens"] = None
                got = collect(aof, eng, gpu_device, dev.records, a["wire"], a["lens"], a["exposure"], a["derotated"], n, n)
                same(got, ob.compact(dev.records, a["wire"], a["lens"], a["exposure"], a["derotated"], n, n), ("without", drop, j))
                header, messages, exps = aof.outbox_view(got, n, n)
                if drop == "wire":
                    assert len(messages) and not messages["mavlink_len"].any() and not messages["mavlink"].any()
                if drop == "exposure":
                    assert int(header["exposures_found"]) == 0 and len(exps) == 0
                if drop == "derotated":
                    assert not messages["derotated"].any()
            got = collect(aof, eng, gpu_device, dev.records, None, dev.lens, expo, derot, n, n)      # lengths without frames
            same(got, ob.compact(dev.records, None, dev.lens, expo, derot, n, n), ("lengths without frames", j))
    assert rounds == set(range(K)) and (exposures > 0) == camera
    eng.close(), eng_t.close()


SHAPES = {1: (1, 1), 63: (7, 9), 64: (1, 64), 65: (5, 13), 255: (15, 17), 256: (16, 16), 257: (1, 257), 4095: (15, 273),
          4096: (16, 256), 4097: (1, 4097), 16 * 16384: (16, 16384)}


def synthetic(n, share, seed):
    """Random [K][S] outputs of a push that never ran: qualities in {-2, -1, 0..255}, random `due`, random frames with
    lengths 0..56, random bytes everywhere else."""
    rng = np.random.default_rng(seed)
    K, S = SHAPES[n]
    recs = rng.integers(0, 256, (K, S, 48), dtype=np.uint8)
    pick = np.ones(n, bool) if share == 1 else rng.random(n) < share
    q = np.where(pick, rng.integers(0, 256, n), rng.integers(-2, 0, n)).astype("<i4")
    recs.reshape(n, 48)[:, :4] = q.view(np.uint8).reshape(n, 4)
    expo = rng.integers(0, 256, (K, S, 48), dtype=np.uint8)
    pick_e = np.ones(n, bool) if share == 1 else rng.random(n) < share
    due = np.where(pick_e, rng.choice(np.array([1, 1, 2, 0x80000000], np.uint32), n), 0).astype("<u4")
    expo.reshape(n, 48)[:, 44:] = due.view(np.uint8).reshape(n, 4)
    wire = rng.integers(0, 256, (K, S, 56), dtype=np.uint8)
    lens = rng.integers(0, 57, (K, S)).astype(np.uint8)
    derot = rng.integers(0, 256, (K, S, 8), dtype=np.uint8)
    return recs, wire, lens, expo, derot


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_the_scan_on_synthetic_arrays(aof, gpu_device, n):
    """The call does not care where its input came from: exact equality with compact() at every size around the wave,
    workgroup and tile boundaries, selected shares 0, about 1/5 and 1, capacities above and below what is found."""
    import torch
    eng = aof.FlowEngine(aof.px4flow_params(64, 64), 0)
    for share in (0, 0.2, 1):
        arrays = synthetic(n, share, 1000 + n % 997)
        found_m, found_e = (len(x) for x in ob.selected(arrays[0], arrays[3]))
        if share == 0:
            assert found_m == found_e == 0
        elif share == 1:
            assert found_m == found_e == n
        elif n >= 255:
            assert 0 < found_m < n // 3 and 0 < found_e < n // 3
        dev = [torch.from_numpy(a).to(gpu_device) for a in arrays]
        for cap_m, cap_e in {(n, n), (found_m // 2, found_e // 3), (max(found_m - 1, 0), found_e + 5)}:
            got = collect(aof, eng, gpu_device, *dev, cap_m, cap_e, tag=0xABCD0000 + n)
            same(got, ob.compact(*arrays, cap_m, cap_e, tag=0xABCD0000 + n), (n, share, cap_m, cap_e))
            header = aof.outbox_view(got, cap_m, cap_e)[0]
            assert (int(header["messages_found"]), int(header["exposures_found"])) == (found_m, found_e)
            assert (int(header["n_messages"]), int(header["n_exposures"])) == (min(found_m, cap_m), min(found_e, cap_e))
    eng.close()


@pytest.mark.parametrize("n", [65, 4097])
def test_sources_that_are_only_four_byte_aligned(aof, gpu_device, n):
    """Records, exposure records and de-rotated pairs need 4-byte alignment, frames none: the same bytes."""
    import torch
    eng = aof.FlowEngine(aof.px4flow_params(64, 64), 0)
    arrays = synthetic(n, 0.2, 77)

    def shifted(a, by):
        t = torch.zeros(a.size + 64, dtype=torch.uint8, device=gpu_device)
        v = t[by:by + a.size]
        v.copy_(torch.from_numpy(a.reshape(-1)))
        return v.view(a.shape)

    dev = [shifted(arrays[0], 4), shifted(arrays[1], 3), shifted(arrays[2], 1), shifted(arrays[3], 12), shifted(arrays[4], 4)]
    assert dev[0].data_ptr() % 16 == 4 and dev[1].data_ptr() % 8 == 3
    got = collect(aof, eng, gpu_device, *dev, n, n)
    same(got, ob.compact(*arrays, n, n), n)
    assert aof.outbox_view(got, n, n)[0]["n_messages"] > 0
    eng.close()


def test_the_host_polls_the_tag_without_a_stream_synchronisation(aof, recipe, gpu_device):
    import torch
    run, recs, wire, lens, frames = recipe
    S = run.S
    eng = aof.FlowEngine(aof.px4flow_params(64, 64), 0)
    host = aof.HostOutbox(S)
    assert host.nbytes == 64 + 128 * S and host.ptr % 64 == 0
    for k, tag in ((1, 0x1111), (8, 0x2222222222)):          # two calls, two tags, two inputs
        d = [torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device) for a in (recs[k].view(np.uint8).reshape(S, 48), frames[k], lens[k])]
        want = collect(aof, eng, gpu_device, d[0], d[1], d[2], None, None, S, tag=tag)       # the device outbox of the same input
        torch.cuda.synchronize()
        host.array[:] = ob.FILL
        eng.bank_collect(d[0], d[1], d[2], capacity_messages=S, outbox=host, tag=tag)
        assert host.wait(tag, timeout_s=5.0), ("the tag did not arrive", hex(host.tag))      # a deadline: fail, never hang
        got = host.array.copy()                                                                # (no synchronisation in front)
        same(got, want, ("host outbox", k))
        header, messages, _ = aof.outbox_view(host)
        assert int(header["tag"]) == tag and len(messages) == ob.CENSUS_15HZ[k] > 0
    torch.cuda.synchronize()
    host.close()
    eng.close()


def test_a_captured_tick_and_collect_carry_a_fresh_tag_on_every_replay(aof, recipe, gpu_device):
    """One linear graph (one stream, no parallel branches): tick + collect with d_tag; the tag tensor is updated between
    replays, and every replay's outbox equals the eager one."""
    import torch
    run, recs, wire, lens, frames = recipe
    S = run.S
    eng = aof.FlowEngine(aof.px4flow_params(64, 64), 0)
    bp = aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0)
    eager = BankRig(aof, eng, run, bp, gpu_device)
    outs = []
    for k in range(run.T):
        eager.load(k)
        eager.enqueue()
        outs.append(collect(aof, eng, gpu_device, eager.records, eager.wire, eager.lens, None, None, S, tag=500 + k))
    dev = BankRig(aof, eng, run, bp, gpu_device)
    box = Box(aof, gpu_device, S)
    tag = torch.zeros(1, dtype=torch.int64, device=gpu_device)
    dev.push(0)                                   # (every kernel has run once before the capture)
    eng.bank_reset(dev.bank)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dev.enqueue()
        eng.bank_collect(dev.records, dev.wire, dev.lens, capacity_messages=S, outbox=box.tensor, tag=0, tag_tensor=tag)
    for k in range(run.T):
        dev.load(k)
        tag.fill_(500 + k)
        box.refill()
        g.replay()
        torch.cuda.synchronize()
        same(box.bytes(), outs[k], ("replay", k))
    eng.close()


def test_what_the_collect_call_refuses_leaves_the_outbox_untouched(aof, synth, gpu_device):
    import torch
    eng = aof.FlowEngine(aof.px4flow_params(64, 64), 0)
    S, K = 8, 2
    n = S * K
    arrays = [torch.from_numpy(a).to(gpu_device) for a in synthetic(4096, 1, 5)]
    recs, wire, lens, expo, derot = (a.reshape(-1)[:n * w].contiguous() for a, w in zip(arrays, (48, 56, 1, 48, 8)))
    box = Box(aof, gpu_device, n, n)
    tagword = torch.ones(1, dtype=torch.int64, device=gpu_device)
    stream = torch.cuda.current_stream().cuda_stream
    call = aof.lib.aof_bank_collect_device

    def args(**kw):
        return [kw.get("ctx", eng._ctx), kw.get("S", S), kw.get("K", K), kw.get("recs", recs.data_ptr()), kw.get("wire", wire.data_ptr()),
                kw.get("lens", lens.data_ptr()), kw.get("expo", expo.data_ptr()), kw.get("derot", derot.data_ptr()), kw.get("cap_m", n),
                kw.get("cap_e", n), kw.get("box", box.tensor.data_ptr()), kw.get("bytes", box.total), kw.get("tag", 9),
                kw.get("d_tag", None), stream]

    refused = [
        (dict(ctx=None), EINVAL), (dict(recs=None), EINVAL), (dict(box=None), EINVAL), (dict(S=0), EINVAL), (dict(S=-3), EINVAL),
        (dict(K=0), EINVAL), (dict(K=aof.BANK_BURST_MAX + 1), EINVAL), (dict(box=box.tensor.data_ptr() + 16), EINVAL),
        (dict(box=box.tensor.data_ptr() + 32), EINVAL), (dict(lens=None), EINVAL),            # d_mavlink without its lengths
        (dict(tag=0), EINVAL),                                                                 # tag 0 with no d_tag
        (dict(bytes=box.total - 1), ENOSPC), (dict(cap_m=n + 1), ENOSPC), (dict(cap_e=n + 1), ENOSPC),
        (dict(recs=recs.data_ptr() + 2), EINVAL), (dict(cap_m=1 << 31), EINVAL),
    ]
    for kw, code in refused:
        assert call(*args(**kw)) == code, kw
    torch.cuda.synchronize()
    assert bool((box.alloc == ob.FILL).all()), "a refused call must write nothing"
    assert b"collect" in aof.lib.aof_last_error(eng._ctx) or b"outbox" in aof.lib.aof_last_error(eng._ctx)
    # the context is still usable; tag 0 is fine with a tag word
    assert call(*args(tag=0, d_tag=tagword.data_ptr())) == 0
    torch.cuda.synchronize()
    same(box.bytes(), ob.compact(recs.view(K, S, 48), wire, lens, expo.view(K, S, 48), derot, n, n, tag=1), "after the refusals")
    eng.close()


def test_a_faulted_context_collects_nothing(aof, synth, gpu_device):
    """The context's sticky device-side condition (raised as tests/test_gpu_bank_burst.py raises it): -EIO before the
    launch, the outbox keeps its bytes."""
    import torch
    p = aof.default_params(640, 480)
    hp, hc, _ = synth.make_batch(640, 480, 8, 4, 4300)
    idx = np.arange(256) % 8
    eng = aof.FlowEngine(p, 0)
    eng.set_search_mode(aof.SEARCH_EXHAUSTIVE)
    eng.set_reduce_fusion(True)
    eng.debug_vote_deadline_ticks(0)
    eng.flow_batch(torch.from_numpy(hp[idx]).to(gpu_device), torch.from_numpy(hc[idx]).to(gpu_device))
    torch.cuda.synchronize()
    recs = torch.from_numpy(synthetic(64, 1, 3)[0]).to(gpu_device)
    box = Box(aof, gpu_device, 64)
    with pytest.raises(aof.AofError) as e:
        eng.bank_collect(recs[0], capacity_messages=64, outbox=box.tensor)
    assert e.value.code == EIO and "deadline" in str(e.value)
    torch.cuda.synchronize()
    assert (box.bytes() == ob.FILL).all()
    eng.close()


def test_the_facade_bank_equals_one_opencv_object_per_stream(aof, synth, gpu_device):
    """OpticalFlowBank against S OpticalFlowOpenCV objects fed the same frames and (uint32_t) times: per stream the same
    sequence of (push index, quality, dt_us, flow_x, flow_y), bit for bit; with an offset set, the MAVLink frames of
    the engine's own bank."""
    S, T = 9, 20
    run = ref.make_run(synth, 128, 128, S, T, 12, wrap=True)
    bank = aof.OpticalFlowBank(FX, FY, 15, 128, 128, S)
    assert bank.engineOk() and bank.lastError() == "ok"
    singles = [aof.OpticalFlowOpenCV(FX, FY, 15, 128, 128) for _ in range(S)]
    assert bank.getPyramidLevels() == singles[0].getPyramidLevels() == 2
    # the engine's own bank with the same configuration, for the wire frames
    p = params_of(aof, "opencv-128")
    eng = aof.FlowEngine(p, 0)
    dev = BankRig(aof, eng, run, aof.bank_params(S, FX, FY, 15, OFFSET, 1, 100, 0), gpu_device)
    got, want = [[] for _ in range(S)], [[] for _ in range(S)]
    empty = published = 0
    n, entries = bank.push(run.frames[0], run.times[0], run.active[0], run.gyro[0])
    assert n == len(entries) > 0 and not entries["mavlink_len"].any() and not entries["mavlink"].any(), "no offset yet: no frames"
    assert bank.reset(None) == 0
    bank.setTimestampOffset(OFFSET)
    for k in range(T):
        n, entries = bank.push(run.frames[k], run.times[k], run.active[k], run.gyro[k])
        assert n == len(entries) >= 0, (n, bank.lastError())
        drecs, dwire, _, _ = dev.push(k)
        assert list(entries["stream"]) == sorted(entries["stream"]) and not entries["round"].any()
        for e in entries:
            s, r = int(e["stream"]), e["record"]
            got[s].append((k, int(r["quality"]), int(r["dt_us"]), r["flow_x"].tobytes(), r["flow_y"].tobytes()))
            assert r.tobytes() == drecs[s].tobytes(), ("the engine's own bank", k, s)
            assert bytes(e["mavlink"][:e["mavlink_len"]]) == dwire[s] != b"", ("wire frame", k, s)
        for s in range(S):
            if run.active[k, s]:
                q, dt, fx, fy = singles[s].calcFlow(run.frames[k, s], int(run.times[k, s]) & 0xFFFFFFFF)
                if q >= 0:
                    want[s].append((k, q, dt, np.float32(fx).tobytes(), np.float32(fy).tobytes()))
        empty += n == 0
        published += n
    assert got == want
    assert published == 31 and empty == 3, (published, empty)
    assert bank.reset(None) == 0
    n, entries = bank.push(run.frames[0], run.times[0], None, None)
    assert n == S and (entries["record"]["quality"] == 0).all() and (entries["record"]["frame"] == 1).all()   # first frames again
    for f in singles:
        f.close()
    bank.close()
    eng.close()
