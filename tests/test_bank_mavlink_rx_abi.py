"""The structures and entry points of the stream bank's MAVLink receive (include/aof.h): sizes and offsets as a C
compiler lays the header out, the binding's dtypes, every refusal -- each returns its code and writes nothing, on the
host function and, where no device is needed, on the device entries' argument checks -- and the header as C99 and
C++11.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mavlink_rx_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22

STATE_FIELDS = ("bytes", "frames", "imu_samples", "bad_check", "overflowed", "skipped", "rejected_flags", "in_progress")
PARAM_FIELDS = ("n_streams", "n_rounds", "max_bytes", "max_samples")


def test_structs_have_the_headers_sizes_and_offsets(aof, tmp_path):
    fmt, args = [], []
    for struct, fields in (("aof_mavlink_rx_state", STATE_FIELDS), ("aof_mavlink_rx_params", PARAM_FIELDS)):
        fmt.append("%zu")
        args.append(f"sizeof({struct})")
        for f in fields:
            fmt.append("%zu")
            args.append(f"offsetof({struct}, {f})")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "aof.h"\n'
           'int main(void) { printf("%s %%d\\n", %s, AOF_MAVLINK_RX_BYTES_MAX); return 0; }\n' % (" ".join(fmt), ", ".join(args)))
    f = tmp_path / "sizes.c"
    f.write_text(src)
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    dtype = aof.MAVLINK_RX_STATE_DTYPE
    assert dtype.names == STATE_FIELDS and tuple(n for n, _ in aof.MavlinkRxParams._fields_) == PARAM_FIELDS
    want = [dtype.itemsize] + [dtype.fields[n][1] for n in STATE_FIELDS]
    want += [C.sizeof(aof.MavlinkRxParams)] + [getattr(aof.MavlinkRxParams, n).offset for n in PARAM_FIELDS]
    want += [aof.MAVLINK_RX_BYTES_MAX]
    assert got == want
    assert got[:9] == [128, 0, 8, 12, 16, 20, 24, 28, 32] and got[9:14] == [16, 0, 4, 8, 12] and got[-1] == 4096
    # the model restates the layout on its own
    assert aof.MAVLINK_RX_STATE_DTYPE == ref.STATE_DTYPE and aof.IMU_SAMPLE_DTYPE == ref.SAMPLE_DTYPE


def test_the_binding_exposes_the_feature(aof):
    for name in ("aof_bank_mavlink_rx_reset_device", "aof_bank_mavlink_rx_device", "aof_bank_mavlink_rx_host"):
        assert name in aof.EXPORTS and hasattr(aof.lib, name)
    assert callable(aof.FlowEngine.bank_mavlink_rx_reset) and callable(aof.FlowEngine.bank_mavlink_rx)
    assert callable(aof.bank_mavlink_rx_host) and callable(aof.mavlink_rx_states_view)
    for name in ("enableMavlinkRx", "pushMavlink"):
        assert callable(getattr(aof.OpticalFlowBank, name))
    assert aof.lib.aof_version() == 102, "the feature adds entry points; the version stays"


def test_the_header_says_that_the_text_is_the_contract():
    hdr = open(os.path.join(ROOT, "include", "aof.h")).read()
    section = hdr[hdr.index("the stream bank's MAVLink receive"):hdr.index("AOF_MAVLINK_RX_BYTES_MAX")]
    assert "mavlink_parse_char is not pinned" in " ".join(section.replace(" * ", " ").split())
    assert "oracle" not in hdr.lower()


class Call:
    """One valid call of aof_bank_mavlink_rx_host on sentinel-filled memory; host() changes arguments and reports the
    code and whether not one byte was written."""

    K, S, B, M = 2, 5, 272, 3

    def __init__(self, aof):
        self.aof = aof
        K, S, B, M = self.K, self.S, self.B, self.M
        (data, lengths), = ref.coverage_family(1, S, K, B)
        self.rp = aof.mavlink_rx_params(S, K, B, M)
        # every buffer inside one 16-byte aligned block, so that a misaligned pointer still points into owned memory
        self.raw = {n: np.zeros(size + 48, np.uint8) for n, size in
                    (("bytes", K * S * B), ("len", 2 * K * S), ("states", 128 * S), ("samples", 24 * K * M * S), ("counts", K * S))}
        self.buf = {}
        for n, raw in self.raw.items():
            off = -raw.ctypes.data % 16
            self.buf[n] = raw[off:off + raw.size - 32]
        self.buf["bytes"][:K * S * B] = data.ravel()
        self.buf["len"][:2 * K * S] = lengths.view(np.uint8).ravel()
        for n in ("samples", "counts"):
            self.buf[n][:] = 0xA5
        self.written = ("states", "samples", "counts")

    def args(self, **change):
        a = dict(rp=C.byref(self.rp), **{n: b.ctypes.data for n, b in self.buf.items()})
        a.update(change)
        return [a[n] for n in ("rp", "bytes", "len", "states", "samples", "counts")]

    def host(self, **change):
        before = {n: self.buf[n].copy() for n in self.written}
        rc = self.aof.lib.aof_bank_mavlink_rx_host(*self.args(**change))
        return rc, all((self.buf[n] == before[n]).all() for n in self.written)


def test_the_valid_call_is_accepted(aof):
    c = Call(aof)
    rc, untouched = c.host()
    assert rc == 0 and not untouched
    assert Call(aof).host(len=None)[0] == 0
    for B in (16, 4096):                             # the ends of the range (one stream, one round: the lengths keep the
        c = Call(aof)                                # reads inside the block)
        c.rp.max_bytes, c.rp.n_streams, c.rp.n_rounds = B, 1, 1
        c.buf["len"][:2] = np.array([300], np.uint16).view(np.uint8)
        assert c.host()[0] == 0, B
    for M, K in ((1, 1), (16, 1), (1, 16)):
        c = Call(aof)
        c.rp.max_samples, c.rp.n_rounds, c.rp.n_streams = M, K, 1
        c.rp.max_bytes = 16
        assert c.host()[0] == 0, (M, K)


REFUSALS = {
    "null params": dict(rp=None),
    "null bytes": dict(bytes=None),
    "null state": dict(states=None),
    "null samples": dict(samples=None),
    "null counts": dict(counts=None),
    "n_streams 0": dict(n_streams=0),
    "n_streams negative": dict(n_streams=-3),
    "n_rounds 0": dict(n_rounds=0),
    "n_rounds above the maximum": dict(n_rounds=17),
    "max_bytes 0": dict(max_bytes=0),
    "max_bytes below 16": dict(max_bytes=8),
    "max_bytes no multiple of 16": dict(max_bytes=264),
    "max_bytes above the maximum": dict(max_bytes=4112),
    "max_samples 0": dict(max_samples=0),
    "max_samples above the maximum": dict(max_samples=17),
    "bytes at 8 mod 16": dict(bytes=+8),
    "states at 4 mod 8": dict(states=+4),
    "samples at 4 mod 8": dict(samples=+4),
    "lengths at 1 mod 2": dict(len=+1),
}


def apply(c, spec):
    change = {}
    for key, v in spec.items():
        if key in PARAM_FIELDS:
            setattr(c.rp, key, v)
        elif v is None:
            change[key] = None
        else:
            change[key] = c.buf[key].ctypes.data + v
    return change


@pytest.mark.parametrize("name", list(REFUSALS))
def test_the_host_function_refuses_and_writes_nothing(aof, name):
    c = Call(aof)
    rc, untouched = c.host(**apply(c, REFUSALS[name]))
    assert rc == EINVAL and untouched


@pytest.mark.parametrize("name", list(REFUSALS))
def test_device_calls_without_a_context_are_refused_first(aof, name):
    """No context can exist without a device: the context check comes first and answers -EINVAL whatever else is passed
    (the ladder behind it is the host function's: both forms share one argument check)."""
    c = Call(aof)
    before = {n: c.buf[n].copy() for n in c.written}
    device, reset = aof.lib.aof_bank_mavlink_rx_device, aof.lib.aof_bank_mavlink_rx_reset_device
    assert device(None, *c.args(**apply(c, REFUSALS[name])), None) == EINVAL
    assert device(None, *c.args(), None) == EINVAL
    assert reset(None, c.S, None, c.buf["states"].ctypes.data, None) == EINVAL
    assert reset(None, 0, None, None, None) == EINVAL
    assert all((c.buf[n] == before[n]).all() for n in c.written)


def test_header_is_valid_c99_and_cxx11(tmp_path):
    src = ('#include "aof.h"\n'
           'int use(aof_ctx *ctx, const unsigned char *b, const uint16_t *n, aof_mavlink_rx_state *s, aof_imu_sample *m,\n'
           '        unsigned char *c) {\n'
           '    aof_mavlink_rx_params rp = {1, AOF_BANK_BURST_MAX, AOF_MAVLINK_RX_BYTES_MAX, AOF_IMU_SLOTS_MAX};\n'
           '    if (aof_bank_mavlink_rx_host(&rp, b, n, s, m, c)) return 1;\n'
           '    if (s->bytes + s->frames + s->imu_samples + s->bad_check + s->overflowed + s->skipped + s->rejected_flags) return 2;\n'
           '    if (aof_bank_mavlink_rx_reset_device(ctx, 1, 0, s, 0)) return 3;\n'
           '    return aof_bank_mavlink_rx_device(ctx, &rp, b, n, s, m, c, 0) + (int)sizeof(*s) + (int)sizeof(s->in_progress);\n'
           '}\n')
    for cc, name, std in (("cc", "t.c", "-std=c99"), ("g++", "t.cpp", "-std=c++11")):
        assert shutil.which(cc), cc
        f = tmp_path / name
        f.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(f)], check=True)
