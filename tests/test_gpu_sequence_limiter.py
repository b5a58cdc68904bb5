"""The sequence limiter's chain -- k_limit_next, k_limit_double and k_sequence_emit of k_sequence.hip under
aof_sequence_device -- against the host model of tests/sequence_limiter_ref.py at every edge of its arithmetic: chain
lengths of 4^r - 1, 4^r and 4^r + 1 (a round more or less of the pointer quadrupling), node counts that fill a workgroup,
gaps of exactly 4096 and 4097 frames (the scan window), recordings that end inside a window, frames that stall WITHOUT
being on the chain, the period's edge and the 32-bit time arithmetic.  There is no tolerance: status, counts, every record
byte and every wire frame equal the model's, the device flows equal the oracle's, and what lies behind the last record in
the caller's workspace is untouched.  The model itself is held to the oracle's calcFlow chain and every design to its
census in tests/test_sequence_limiter_ref.py, without a device.

The recording is PX4 64 x 64, sensor == crop: frame k is base[k % 64] of one synth.make_sequence with a few dark stretches,
so the oracle computes at most 64 textured pairs plus the ones with a dark frame, once for the whole module."""
import numpy as np
import pytest

import sequence_limiter_ref as lr
from bank_rig import time_limit   # (this module's fixture too: every test under a limit of its own)

pytestmark = pytest.mark.gpu

FX, FY = 216.6677, 216.2457
OFFSET = 5_000_000
FILL = 0xA5
W = H = 64
MAX_FRAMES = 257 * 256 + 1 + 256          # the longest strided design
EDGES = lr.period_edges()
DARK_SEGMENTS = ((28, 41), (100, 103))    # every-third: the segments (30, 33], (33, 36] and (36, 39] are dark throughout


class Rig:
    def __init__(self, aof, orc, synth, device):
        import torch
        self.aof, self.orc, self.device = aof, orc, device
        self.p = aof.px4flow_params(W, H)
        self.po = orc.params_from(self.p)
        self.base, _ = synth.make_sequence(W, H, 64, 4, seed=31, max_step=3)
        self.base_dev = torch.from_numpy(lr.frames_of(self.base, np.arange(lr.DARK + 1))).to(device)
        self.gyro = lr.gyro_of(MAX_FRAMES)
        self.gyro_dev = torch.from_numpy(self.gyro).to(device)
        self.memo = {}
        self.eng = aof.FlowEngine(self.p, 0)

    def params(self, rate, offset=OFFSET, first_seq=250):
        return self.aof.sequence_params(W, H, W, H, FX, FY, rate, offset, 1, 100, first_seq)

    def inputs(self, times, dark=None):
        """(frame ids, camera tensor [n, 64, 64], time-stamp tensor) of a recording."""
        import torch
        ids = lr.frame_ids(len(times), dark)
        return ids, self.base_dev[torch.from_numpy(ids).to(self.device)], torch.from_numpy(np.asarray(times, np.int64)).to(self.device)

    def model(self, times, ids, rate, offset, first_seq):
        n = len(times)
        flows = lr.flows_of(self.orc, self.po, self.base, ids, self.memo)
        recs, status = lr.limiter_model(times, flows, self.gyro[:n], rate, FX, FY, angle=self.orc.angle)
        return flows, recs, status, lr.wire_of(recs, times, offset, first_seq)

    def check(self, ws, L, n, want, offset):
        """Everything aof_sequence_device left in the 0xA5 workspace against the model's (flows, recs, status, wire)."""
        flows, recs, status, wire = want
        region = lambda off, size: ws[off:off + size].cpu().numpy()
        count = region(L.count, 16).view(np.uint32)
        got = region(L.records, 32 * n).view(lr.RECORD_DTYPE)
        frames = region(L.frames, 56 * n).reshape(n, 56)
        lens = region(L.frame_len, n)
        c = int(count[0])
        print(f"n={n} status={int(count[2])} (model {status}) records={c} (model {len(recs)}) frames_sent={int(count[1])} (model {len(wire)})")
        assert c == len(recs), "record count"
        assert int(count[1]) == len(wire), "frames_sent"
        assert int(count[3]) == 0
        if got[:c].tobytes() != recs.tobytes():
            m = next(m for m in range(c) if got[m].tobytes() != recs[m].tobytes())
            raise AssertionError(f"record {m}: device {got[m]} model {recs[m]}")
        if offset:
            for m in range(c):
                assert frames[m, :lens[m]].tobytes() == wire[m], ("wire frame", m)
        else:
            assert not lens[:c].any(), "vehicle time not known: nothing is sent"
        assert (got[c:].view(np.uint8) == FILL).all(), "records behind count[0] were written"
        assert (frames[c:] == FILL).all(), "frames behind count[0] were written"
        assert (lens[c:] == FILL).all(), "frame_len behind count[0] was written"
        assert region(L.flows, 16 * (n - 1)).tobytes() == flows.tobytes(), "device flows differ from the oracle's"
        assert int(count[2]) == status, "status (everything else equals the model's)"
        return recs

    def run(self, times, rate, status=None, records=None, dark=None, offset=OFFSET, first_seq=250):
        """One recording through aof_sequence_device into a workspace pre-filled with 0xA5, against the model.  status and
        records: what the design was built for -- asserted on the model before the device runs."""
        import torch
        n = len(times)
        ids, cam, tt = self.inputs(times, dark)
        want = self.model(times, ids, rate, offset, first_seq)
        assert status is None or want[2] == status
        assert records is None or len(want[1]) == records
        sp = self.params(rate, offset, first_seq)
        L = self.aof.sequence_layout(self.p, sp, n)
        ws = torch.full((L.total_bytes,), FILL, dtype=torch.uint8, device=self.device)
        self.eng.sequence(sp, cam, tt, self.gyro_dev[:n], workspace=ws)
        torch.cuda.synchronize()
        return self.check(ws, L, n, want, offset)

    def run_design(self, d, **kw):
        return self.run(d.times, d.rate, status=d.status, records=d.census["records"], **kw)


@pytest.fixture(scope="module")
def rig(aof, orc, synth, gpu_device):
    r = Rig(aof, orc, synth, gpu_device)
    yield r
    r.eng.close()


# ---- frame counts, every frame publishing ------------------------------------------------------------------------------
COUNTS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385)
SCANNED = (1, 2, 5, 16, 17, 255, 256, 257, 1024, 4097, 16384, 16385)      # also at 15 Hz: through the scan, not the shortcut


@pytest.mark.parametrize("n", COUNTS)
def test_every_frame_publishes_without_a_rate(rig, n):
    """rate = 0: n records, the END node n hops from the start -- the most the rounds of sequence_rounds(n) must cover."""
    d = lr.every_frame(n)
    recs = rig.run(d.times, 0, status=0, records=n)
    assert recs["frame"].tolist() == list(range(n))


@pytest.mark.parametrize("n", SCANNED)
def test_every_frame_publishes_through_the_scan(rig, n):
    recs = rig.run_design(lr.every_frame(n))
    assert recs["frame"].tolist() == list(range(n))


# ---- strides -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 2, 3, 4])
@pytest.mark.parametrize("g", [2, 3, 5, 7, 64, 255, 256, 257])
def test_a_publication_every_g_frames(rig, g, r):
    """Chains of 4^r - 1, 4^r and 4^r + 1 records with 0, 1 and g - 1 unpublished frames behind the last."""
    for records in (4 ** r - 1, 4 ** r, 4 ** r + 1):
        for tail in (0, 1, g - 1):
            d = lr.strided(g, records, tail)
            recs = rig.run_design(d)
            assert recs["frame"].tolist() == [0] + d.chain and d.census["tail"] == tail


# ---- the scan window ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 37], ids=["from-the-start", "mid-chain"])
@pytest.mark.parametrize("design", ["gap-4096-found", "gap-4097-stalled", "window-reaches-the-end", "one-frame-beyond-the-window"])
def test_scan_window(rig, design, i):
    d = {"gap-4096-found": lambda: lr.gap(i, 4096, 3), "gap-4097-stalled": lambda: lr.gap(i, 4097, 3),
         "window-reaches-the-end": lambda: lr.held_to_end(i, 4096), "one-frame-beyond-the-window": lambda: lr.held_to_end(i, 4097)}[design]()
    assert d.status == (lr.STALLED if design in ("gap-4097-stalled", "one-frame-beyond-the-window") else 0)
    recs = rig.run_design(d)
    assert int(recs["frame"][-1]) == (i + 4098 if design == "gap-4096-found" else i), "the records end where the chain ends"


def test_frames_that_are_not_on_the_chain_do_not_raise_stalled(rig):
    """154 frames off the chain find no successor inside their own window; every chain node does.  STALLED means that the
    CHAIN ended (include/aof.h): status 0 and all 1711 records."""
    d = lr.off_chain_stall()
    assert d.status == 0 and d.census["records"] == 1711
    rig.run_design(d)


# ---- the period's edge and the time arithmetic -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EDGES))
def test_period_edges_and_time_arithmetic(rig, name):
    d = EDGES[name]
    recs = rig.run_design(d, dark=DARK_SEGMENTS)                      # (first_seq = 250: the sequence number wraps)
    if name in ("backwards-step", "jump-2-to-31", "u32-wrap"):
        assert (recs["dt_us"] < 0).sum() == 1
    if name == "every-third":
        dark = recs[(recs["frame"] >= 33) & (recs["frame"] <= 39)]
        assert len(dark) == 3 and (dark["quality"] == 0).all(), "whole segments of dark frames: published, quality 0"


@pytest.mark.parametrize("name", ["every-third", "rate-0"])
def test_nothing_is_sent_while_the_vehicle_time_is_unknown(rig, name):
    d = EDGES[name]
    rig.run_design(d, dark=DARK_SEGMENTS, offset=0)


# ---- irregular gaps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeded_irregular_gaps(rig, seed):
    d = lr.irregular(seed)
    assert len(d.times) == 9000
    rig.run_design(d)


# ---- a captured graph --------------------------------------------------------------------------------------------------
def test_a_captured_graph_follows_the_time_stamps(rig):
    """One capture, replayed with the time-stamp tensor rewritten: a stalled pattern, a clean one, the off-chain one."""
    import torch
    n = 6000
    stalled, clean, off_chain = lr.gap(37, 4097, n - 37 - 4097), lr.strided(3, 2000, 2), lr.off_chain_stall()
    assert [len(d.times) for d in (stalled, clean, off_chain)] == [n] * 3
    assert (stalled.status, clean.status, off_chain.status) == (lr.STALLED, 0, 0)
    ids, cam, tt = rig.inputs(stalled.times)
    sp = rig.params(lr.RATE)
    L = rig.aof.sequence_layout(rig.p, sp, n)
    ws = torch.full((L.total_bytes,), FILL, dtype=torch.uint8, device=rig.device)
    gy = rig.gyro_dev[:n]
    rig.eng.sequence(sp, cam, tt, gy, workspace=ws)
    torch.cuda.synchronize()
    rig.check(ws, L, n, rig.model(stalled.times, ids, lr.RATE, OFFSET, 250), OFFSET)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rig.eng.sequence(sp, cam, tt, gy, workspace=ws)
    for d in (stalled, clean, off_chain):
        tt.copy_(torch.from_numpy(d.times))
        ws.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        want = rig.model(d.times, ids, lr.RATE, OFFSET, 250)
        assert want[2] == d.status and len(want[1]) == d.census["records"]
        rig.check(ws, L, n, want, OFFSET)
