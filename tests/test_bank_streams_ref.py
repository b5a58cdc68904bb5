"""The per-stream records of the stream bank (aof_bank_stream, include/aof.h) without a device: the struct's layout,
aof_bank_stream_from_params, what aof_set_bank_streams refuses without a context, the limiter's period as one float
division, and the conditions on the INPUT of tests/test_gpu_bank_streams.py -- a table whose streams never hold, never
publish or all share one angle could not tell a per-stream bank from a scalar one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bank_ref as ref
import bank_streams_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
FIELDS = [("focal_x", 0, 4), ("focal_y", 4, 4), ("output_rate", 8, 4), ("system_id", 12, 1), ("component_id", 13, 1),
          ("first_seq", 14, 1), ("reserved0", 15, 1), ("offset_timestamp_usec", 16, 8), ("reserved1", 24, 8)]


def test_struct_is_32_bytes_with_the_header_s_offsets(aof, tmp_path):
    assert C.sizeof(aof.BankStream) == 32 and aof.BANK_STREAM_DTYPE.itemsize == 32
    for name, off, size in FIELDS:
        f = getattr(aof.BankStream, name)
        assert (f.offset, f.size) == (off, size), name
        assert aof.BANK_STREAM_DTYPE.fields[name][1] == off and aof.BANK_STREAM_DTYPE.fields[name][0].itemsize == size, name
    assert [n for n, _ in aof.BankStream._fields_] == [n for n, _, _ in FIELDS] == list(aof.BANK_STREAM_DTYPE.names)
    # and the header itself, through a C compiler
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "aof.h"\nint main(void) { printf("%zu", sizeof(aof_bank_stream));\n'
                   + "".join(f'printf(" %zu", offsetof(aof_bank_stream, {n}));\n' for n, _, _ in FIELDS) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [32] + [off for _, off, _ in FIELDS]


def test_from_params_gives_the_fields_it_was_given(aof):
    for fx, fy, rate, offset, sysid, compid, seq in sref.TABLE + [sref.DECOY]:
        bp = aof.bank_params(7, fx, fy, rate, offset, sysid, compid, seq, frame_stride=4096 + 16)
        r = aof.bank_stream_from_params(bp)
        assert r.dtype == aof.BANK_STREAM_DTYPE
        assert r["focal_x"] == np.float32(fx) and r["focal_y"] == np.float32(fy) and r["output_rate"] == rate
        assert (r["system_id"], r["component_id"], r["first_seq"]) == (sysid, compid, seq)
        assert r["offset_timestamp_usec"] == offset and r["reserved0"] == 0 and r["reserved1"] == 0
        assert r.tobytes() == sref.records(aof, 1, [(fx, fy, rate, offset, sysid, compid, seq)]).tobytes()
        many = aof.bank_stream_from_params(bp, 5)
        assert many.shape == (5,) and all(m.tobytes() == r.tobytes() for m in many)
    out = aof.BankStream()
    assert aof.lib.aof_bank_stream_from_params(None, C.byref(out)) == EINVAL
    assert aof.lib.aof_bank_stream_from_params(C.byref(aof.bank_params(1)), None) == EINVAL
    assert aof.lib.aof_set_bank_streams(None, None, 0) == EINVAL


def test_the_period_is_one_float_division(aof, orc, synth):
    """float32(1e6) / float32(rate) is the oracle limiter's period: the oracle publishes a stream's second frame iff the
    (float) time since publication 0 exceeds it -- the integer time floor(period) is held, floor(period) + 1 published."""
    p = aof.px4flow_params(64, 64)
    frames, _ = synth.make_sequence(64, 64, 2, 4, seed=5, max_step=2)
    rates = sorted({r[2] for r in sref.TABLE if r[2] > 0})
    assert rates == [10, 15, 30, 200]
    for rate in rates:
        period = np.float32(1e6) / np.float32(rate)
        assert period == np.float32(np.float64(1e6) / rate), "correctly rounded: the double quotient rounded once"
        edge = int(np.floor(period))
        assert np.float32(edge) <= period < np.float32(edge + 1)
        for t, published in ((edge, False), (edge + 1, True)):
            o = orc.Px4(orc.params_from(p), ref.FX, ref.FY, rate)
            assert o.calc_flow(frames[0], 0)[0] == 0
            assert (o.calc_flow(frames[1], t)[0] >= 0) == published, (rate, t)


@pytest.mark.parametrize("cfg", ["px4-64", "opencv-128"])
def test_the_table_s_run_holds_publishes_and_tells_the_focal_lengths_apart(aof, orc, synth, cfg):
    """The census on the input of the parity test, on the oracle's records."""
    p = aof.px4flow_params(64, 64) if cfg == "px4-64" else aof.px4flow_params(128, 128, pyramid_levels=2, mean_subtract=1)
    run = ref.make_run(synth, p.width, p.height, 6, 48, 71 if cfg == "px4-64" else 72)
    want, wire = sref.expected(aof, orc, p, run)
    pub, held, idle = ref.census(want)
    assert sref.LIMITED_STREAMS == [0, 1, 3, 4]
    for s in sref.LIMITED_STREAMS:          # the project's LIMITED thresholds (tests/test_gpu_bank.py)
        assert pub[s] >= 3 and held[s] >= 10, (s, pub, held)
    for s in (2, 5):                        # no limiter, and a rate above the frame rate: every active frame publishes
        assert held[s] == 0 and pub[s] == run.active[:, s].sum() >= 30, (s, pub, held)
    # frames: every stream with an offset sends one per published record, stream 3 none, each with its own identity and
    # a sequence number that counts from its own first_seq.  (Stream 1 starts at 250: at 10 Hz, 48 ticks of 9..18 ms end
    # at 254 or 255; the wrap through 255 is met where a stream publishes every frame, in the rewrite test on the device.)
    for s in range(6):
        sent = [w[s] for w in wire if w[s]]
        assert len(sent) == (0 if s == 3 else pub[s]), s
        if sent:
            assert all(f[5:7] == bytes(sref.TABLE[s][4:6]) for f in sent), s
            assert [f[4] for f in sent] == [(sref.TABLE[s][6] + m) & 0xFF for m in range(len(sent))], s
    # streams 0, 1 and 4: one pixel flow, three angles; stream 4's focal length lies below real pixel flows (|y| > x)
    for px in (0.5, 1.25, -3.0):
        angles = {aof.flow_angle(px, sref.TABLE[s][0]) for s in (0, 1, 4)}
        assert len(angles) == 3, px
    rec4 = want[:, 4][(want[:, 4]["quality"] > 0)]
    assert (np.abs(np.tan(rec4["flow_x"].astype(np.float64))) > 1.0).any(), "a published flow above the focal length"
